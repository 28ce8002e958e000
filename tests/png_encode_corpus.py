"""Frames that put png.Encode on the GPU (csrc/ipx_png.hip) at the edges of its coders, for tests/test_encode_edge_corpus.py (CPU: every
case has the property it is there for) and tests/test_png_encode_edges_gpu.py (GPU: every case byte for byte against tests/png_model.py
and, independently, inflated by zlib to the filtered rows of plain_filter() below).  Everything is built from seeds; nothing large is
committed.  `python tests/png_encode_corpus.py --search` is the CPU search (with png_model) that found the committed seeds and sizes;
`--report` prints every case's measured figures.  No search runs at test time.

What the cases reach (the figures are asserted by the CPU test):
  * the limiting loop of huff_build for the literal/length tree (limit 15) and for the code-length code (limit 7), in segments that go
    out dynamic.  NOT reached by any frame: the limit of the distance tree (the same huff_build call with nsym = 30).  Depth 16 needs
    the counts of 17 distance classes close to a Fibonacci series (1, 1, 2, 3 ... 987, about 2 600 matches), and the greedy parse
    decides which planted copies become tokens: a 30000 x 1 row of planted copies with Fibonacci-weighted distance classes stayed at
    depth 12, and it was not chased further.  The CPU test asserts that the corpus' deepest distance tree stays within the limit.
  * dynamic blocks without a match (hdist == 2, both distance symbols forced) and with exactly one used distance symbol;
  * the smallest frames that still go out dynamic (chunks shorter than 256 bytes: idle lanes in the CRC split);
  * the window: 2 * stride == 32768 (kept) and 32774 (dropped), stride == 32767 (kept) and 32770 (dropped), a token at distance 32768;
  * stored segments of a whole number of 65535-byte blocks (the empty block behind them at b == nblk) and their neighbours, a stored
    last segment behind a dynamic one;
  * matches capped by the segment's end, ending at it with length 258, and reaching back across a segment boundary;
  * every filter winning a row, every tie between neighbours of Go's order Up, Paeth, None, Sub, Average, the cases of png_kats.json.
"""
import functools
import json
import os
import zlib

import numpy as np

import png_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the independent filter reference ------------------------------------------------------------------------------------------------
# One byte at a time from the PNG specification (section 9: None, Sub, Up, Average, Paeth over the byte bpp to the left, the byte above
# and the byte above-left, zero outside the image) and Go's writer: colour type 2 for an opaque *image.RGBA, else 6 with the
# un-premultiplied colour; per row the filter with the smallest sum of |int8(filtered byte)|, tried in the order Up, Paeth, None, Sub,
# Average, the first strict minimum winning.  Shares nothing with png_model.filter_rows.
GO_ORDER = (2, 4, 0, 1, 3)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def _raw(rgba):
    h, w = rgba.shape[:2]
    flat = rgba.reshape(h, w * 4).tolist()
    opaque = all(a == 255 for row in flat for a in row[3::4])
    rows = []
    for row in flat:
        out = []
        for x in range(w):
            r, g, b, a = row[4 * x:4 * x + 4]
            if opaque:
                out += [r, g, b]
            elif a == 0:
                out += [0, 0, 0, 0]
            elif a == 255:
                out += [r, g, b, a]
            else:                                           # uint32 arithmetic in Go: nothing here reaches 2^32
                out += [((c * 0x101 * 0xFFFF) // (a * 0x101) >> 8) & 0xFF for c in (r, g, b)] + [a]
        rows.append(out)
    return (3 if opaque else 4), rows


def filter_scores(cur, prev, bpp):
    """-> ({filter type: score}, {filter type: filtered bytes}) of one raw row (lists of ints)"""
    n = len(cur)
    left = [0] * bpp + cur[:n - bpp]
    upleft = [0] * bpp + prev[:n - bpp]
    out = {0: cur,
           1: [(x - a) & 0xFF for x, a in zip(cur, left)],
           2: [(x - b) & 0xFF for x, b in zip(cur, prev)],
           3: [(x - ((a + b) >> 1)) & 0xFF for x, a, b in zip(cur, left, prev)],
           4: [(x - _paeth(a, b, c)) & 0xFF for x, a, b, c in zip(cur, left, prev, upleft)]}
    return {t: sum(d if d < 128 else 256 - d for d in out[t]) for t in range(5)}, out


def plain_filter(rgba, want_scores=False):
    """-> (bpp, filter type per row, the bytes png.Encode hands zlib) [, scores per row]"""
    bpp, rows = _raw(np.ascontiguousarray(rgba, dtype=np.uint8))
    prev = [0] * len(rows[0])
    types, stream, scores = [], bytearray(), []
    for cur in rows:
        score, out = filter_scores(cur, prev, bpp)
        best = None
        for t in GO_ORDER:
            if best is None or score[t] < score[best]:
                best = t
        types.append(best)
        scores.append(score)
        stream.append(best)
        stream += bytes(out[best])
        prev = cur
    return (bpp, types, bytes(stream), scores) if want_scores else (bpp, types, bytes(stream))


def inflate(stream):
    """(IHDR fields, the inflated IDAT data) of a PNG stream; the CRCs are checked by read_chunks, the Adler-32 by zlib"""
    chunks = pm.read_chunks(stream)
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    assert all(k == b"IDAT" for k, _ in chunks[1:-1])
    return chunks[0][1], zlib.decompress(b"".join(d for k, d in chunks if k == b"IDAT"))


def check_stream(stream, rgba):
    """the independent check of one stream: zlib inflates it to the plain loop's filtered rows, and the header says what they are"""
    import struct
    h, w = rgba.shape[:2]
    bpp, _, want = reference(rgba)
    ihdr, data = inflate(stream)
    assert ihdr == struct.pack(">IIBBBBB", w, h, 8, 2 if bpp == 3 else 6, 0, 0, 0)
    assert data == want


_REF = {}


def reference(rgba):
    """plain_filter, computed once per frame (the frames of the corpus are built once too: see frame())"""
    key = id(rgba)
    if key not in _REF:
        _REF[key] = (rgba, plain_filter(rgba))
    return _REF[key][1]


def model_stream(rgba):
    """png_model.png_encode, computed once per frame"""
    key = ("model", id(rgba))
    if key not in _REF:
        _REF[key] = (rgba, pm.png_encode(rgba))
    return _REF[key][1]


# ---- frames ----------------------------------------------------------------------------------------------------------------------
def _fib(k):
    a, b = 1, 1
    out = []
    for _ in range(k):
        out.append(a)
        a, b = b, a + b
    return np.array(out, np.float64)


def _opaque(rgb):
    f = np.empty(rgb.shape[:2] + (4,), np.uint8)
    f[..., :3] = rgb
    f[..., 3] = 255
    return f


def _build(kind, w, h, seed):
    rng = np.random.default_rng([seed, w, h, len(kind)])
    if kind == "fib":               # bytes from a Fibonacci-weighted alphabet of 18..25 random byte values
        k = 18 + seed % 8
        alphabet = rng.choice(256, k, replace=False)
        wt = _fib(k)
        return _opaque(alphabet[rng.choice(k, (h, w, 3), p=wt / wt.sum())])
    if kind == "levels":            # a few grey levels k * 40 in one short row: the seeds kept have no match at all
        return _opaque(np.repeat(rng.integers(0, 6 + seed % 2, (h, w, 1)) * 40, 3, axis=2))
    if kind == "const":
        return _opaque(np.broadcast_to(np.array([seed * 37 % 256, seed * 101 % 256, seed * 53 % 256]), (h, w, 3)))
    if kind == "noise":
        return _opaque(rng.integers(0, 256, (h, w, 3)))
    if kind == "aba":               # random rows A B A B A ...: rows 3 and 4 filter to what rows 1 and 2 filtered to
        ab = rng.integers(0, 256, (2, w, 3))
        return _opaque(ab[np.arange(h) % 2])
    if kind == "ramp":              # row y = row y - 1 + D (mod 256), D small: Up wins every row after the first and leaves D, so row y
        d = rng.integers(-20, 21, (1, w, 3))                # of the filtered stream repeats row y - 1 at distance stride exactly
        r0 = rng.integers(0, 256, (1, w, 3))
        return _opaque((r0 + d * np.arange(h)[:, None, None]) % 256)
    if kind == "checks":            # 16 x 16 checks: long matches at distance 1, bpp, stride; more than one segment when tall enough
        yy, xx = np.mgrid[0:h, 0:w]
        rgb = np.empty((h, w, 3), np.int64)
        rgb[..., 0] = np.where((xx // 16 + yy // 16) % 2 == 0, 200, 30)
        rgb[..., 1] = 90
        rgb[..., 2] = (yy // 64) * 40 % 256
        return _opaque(rgb)
    if kind == "flat+noise":        # constant rows, then noise from the row where the last segment starts: dynamic, then stored
        stride = 1 + 3 * w
        rps = -(-pm.SEG_MIN // stride)
        rgb = np.full((h, w, 3), 77, np.int64)
        y0 = (max(1, h // rps) - 1) * rps
        rgb[y0:] = rng.integers(0, 256, (h - y0, w, 3))
        return _opaque(rgb)
    if kind == "alpha":             # gradients with alpha 0, 1..254 and 255: colour type 6
        yy, xx = np.mgrid[0:h, 0:w]
        f = np.empty((h, w, 4), np.int64)
        f[..., 0] = xx * 255 // max(w - 1, 1)
        f[..., 1] = yy * 255 // max(h - 1, 1)
        f[..., 2] = (xx + yy) * 3 % 256
        f[..., 3] = np.where(rng.random((h, w)) < 0.5, rng.integers(0, 256, (h, w)), 255)
        f[..., :3] = f[..., :3] * f[..., 3:4] // 255
        return f.astype(np.uint8)
    if kind == "tiny":              # w x h opaque, values of 0..3 around a base: rows whose filter scores tie
        base = rng.integers(0, 4, 3) * (seed % 3)
        return _opaque(base + rng.integers(0, 4, (h, w, 3)))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def frame(kind, w, h, seed):
    """H x W x 4 uint8 as an *image.RGBA holds it (premultiplied); built once, read-only"""
    f = np.ascontiguousarray(_build(kind, w, h, seed), dtype=np.uint8)
    f.setflags(write=False)
    return f


def kat_frames():
    with open(os.path.join(HERE, "golden", "png_kats.json")) as fh:
        cases = json.load(fh)["cases"]
    return [(c, np.array(c["rgba"], np.uint8).reshape(c["h"], c["w"], 4)) for c in cases]


# ---- what the model does with a frame --------------------------------------------------------------------------------------------
class Segment:
    """one segment as png_model codes it: tokens, the depths the three trees would have without a limit, stored or dynamic"""


def report(rgba):
    """[Segment] of a frame, through png_model"""
    bpp, w, h, data = pm.filtered_stream(rgba)
    best_len, best_dist, segs = pm.best_matches(data, w, bpp)
    out = []
    for k, (s, e) in enumerate(segs):
        g = Segment()
        g.start, g.end = s, e
        g.pos = pm.parse(best_len, s, e)
        g.len = best_len[g.pos]
        g.dist = np.where(g.len > 0, best_dist[g.pos], 0)
        is_m = g.len >= pm.MIN_MATCH
        g.nmatch, g.nlit = int(is_m.sum()), int((~is_m).sum())
        lsym = np.where(is_m, 257 + pm._LEN_SYM[g.len], data[g.pos])
        lfreq = np.bincount(lsym, minlength=286)
        lfreq[256] += 1
        dfreq = np.bincount(pm._DIST_SYM[g.dist[is_m]], minlength=30)
        g.dist_used = int((dfreq > 0).sum())
        llen, dlen = pm.huffman_lengths(lfreq, pm.LIMIT_LITLEN), pm.huffman_lengths(dfreq, pm.LIMIT_LITLEN)
        hlit = max(257, max(q for q in range(286) if llen[q]) + 1)
        g.hdist = max(1, max(q for q in range(30) if dlen[q]) + 1)
        cfreq = np.bincount([c for c, _, _ in pm.rle_code_lengths(llen[:hlit] + dlen[:g.hdist])], minlength=19)
        g.depth_lit = max(pm.huffman_lengths(lfreq, 64))
        g.depth_dist = max(pm.huffman_lengths(dfreq, 64))
        g.depth_cl = max(pm.huffman_lengths(cfreq, 64))
        first, last = k == 0, k == len(segs) - 1
        g.chunk = pm.deflate_segment(data, best_len, best_dist, s, e, first, last)
        g.dynamic = (g.chunk[2 if first else 0] >> 1) & 3 == 2
        g.stored_bytes = pm.stored_bytes(e - s, first)
        g.max_dist = int(g.dist.max()) if g.nmatch else 0
        g.data = data
        g.stride = 1 + w * bpp
        out.append(g)
    return out


# ---- the cases: (name, (kind, w, h, seed), property) -------------------------------------------------------------------------------
# PROPERTIES[property](segments of the frame) -> (holds, the measured figure as text)
def _limit_lit(segs):
    d = [g.depth_lit for g in segs if g.dynamic]
    return bool(d) and max(d) > pm.LIMIT_LITLEN, "literal/length depth without the limit %s" % d


def _limit_cl(segs):
    d = [g.depth_cl for g in segs if g.dynamic]
    return bool(d) and max(d) > pm.LIMIT_CL, "code-length code depth without the limit %s" % d


def _no_match(segs):
    g = segs[0]
    return len(segs) == 1 and g.dynamic and g.nmatch == 0 and g.hdist == 2, "%d literals, %d matches, hdist %d" % (g.nlit, g.nmatch, g.hdist)


def _one_dist(segs):
    g = segs[0]
    return len(segs) == 1 and g.dynamic and g.nmatch > 0 and g.dist_used == 1, "%d matches over %d distance symbol" % (g.nmatch, g.dist_used)


def _small_dynamic(segs):
    g = segs[0]
    return len(segs) == 1 and g.dynamic and len(g.chunk) + 4 < 256, "dynamic, %d bytes of chunk data (stored: %d)" % (len(g.chunk), g.stored_bytes)


def _narrow_dynamic(segs):
    g = segs[0]
    return len(segs) == 1 and g.dynamic and g.stored_bytes - len(g.chunk) <= 1, "dynamic at %d bytes, stored would be %d" % (len(g.chunk), g.stored_bytes)


def _dist(n):
    def prop(segs):
        m = max(g.max_dist for g in segs)
        cnt = sum(int((g.dist == n).sum()) for g in segs)
        long = sum(int(((g.dist == n) & (g.len == pm.MAX_MATCH)).sum()) for g in segs)
        return m == n and long > 0 and all(g.dynamic for g in segs), "largest distance %d (%d tokens, %d of length 258)" % (m, cnt, long)
    return prop


def _stride_dropped(segs):
    """the row above is there to copy (rows 1 and 2 of the filtered stream are equal), but stride is past the window: no token takes it"""
    g = segs[0]
    n = g.stride
    same = bool((g.data[n:2 * n] == g.data[2 * n:3 * n]).all())
    at = int((g.dist == n).sum())
    long = int((g.len == pm.MAX_MATCH).sum())
    ok = len(segs) == 1 and n > pm.WINDOW and same and at == 0 and g.nmatch > 0 and g.max_dist <= pm.WINDOW
    return ok, "stride %d, row 2 equals row 1: %s, tokens at distance stride %d, largest distance %d, tokens of length 258: %d" % (n, same, at, g.max_dist, long)


def _all_stored_no_match(segs):
    return all(not g.dynamic and g.nmatch == 0 for g in segs), "%d matches, %s" % (sum(g.nmatch for g in segs), ["dynamic" if g.dynamic else "stored" for g in segs])


def _stored_blocks(whole):
    def prop(segs):
        n = [g.end - g.start for g in segs]
        ok = all(not g.dynamic for g in segs) and any(v % 65535 == 0 for v in n) == whole
        return ok, "stored, " + ", ".join("%d bytes = %d * 65535 + %d" % (v, v // 65535, v % 65535) for v in n)
    return prop


def _dynamic_then_stored(segs):
    kinds = ["dynamic" if g.dynamic else "stored" for g in segs]
    return len(segs) > 1 and all(g.dynamic for g in segs[:-1]) and not segs[-1].dynamic, " ".join(kinds)


def _ends_258(segs):
    g = segs[0]
    ok = len(segs) > 1 and g.dynamic and g.len[-1] == pm.MAX_MATCH and g.pos[-1] + pm.MAX_MATCH == g.end
    return ok, "last token of segment 0: length %d at %d, segment ends at %d" % (g.len[-1], g.pos[-1], g.end)


def _cut_short(segs):
    g = segs[0]
    p, ln, d = int(g.pos[-1]), int(g.len[-1]), int(g.dist[-1])
    ok = len(segs) > 1 and g.dynamic and pm.MIN_MATCH <= ln < pm.MAX_MATCH and p + ln == g.end and g.data[g.end] == g.data[g.end - d]
    return ok, "last token of segment 0: length %d at %d = end - %d, the data goes on matching" % (ln, p, g.end - p)


def _reaches_back(segs):
    g = segs[1] if len(segs) > 1 else segs[0]
    back = (g.len >= pm.MIN_MATCH) & (g.pos - g.dist < g.start)
    return len(segs) > 1 and g.dynamic and bool(back.any()), "%d tokens of segment 1 copy from segment 0" % int(back.sum())


PROPERTIES = {
    "lit limit": _limit_lit, "cl limit": _limit_cl, "no match": _no_match, "one distance symbol": _one_dist,
    "small dynamic": _small_dynamic, "narrow dynamic": _narrow_dynamic,
    "distance 32768": _dist(32768), "distance 32767": _dist(32767), "stride dropped": _stride_dropped,
    "no match, stored": _all_stored_no_match,
    "whole stored blocks": _stored_blocks(True), "partial stored block": _stored_blocks(False), "dynamic then stored": _dynamic_then_stored,
    "ends with 258": _ends_258, "cut short": _cut_short, "reaches back": _reaches_back,
}

CASES = [
    # two frames per limit (found by --search); 252 x 172 reaches both
    ("lit limit a", ("fib", 109, 286, 0), "lit limit"),
    ("lit limit b", ("fib", 252, 172, 0), "lit limit"),
    ("cl limit a", ("fib", 252, 172, 0), "cl limit"),
    ("cl limit b", ("fib", 300, 100, 0), "cl limit"),
    ("no match a", ("levels", 29, 1, 1), "no match"),
    ("no match b", ("levels", 36, 1, 2), "no match"),
    ("one distance symbol", ("const", 300, 1, 3), "one distance symbol"),
    ("small dynamic a", ("const", 1, 5, 1), "small dynamic"),
    ("small dynamic b", ("levels", 1, 5, 0), "small dynamic"),
    ("small dynamic c", ("const", 5, 1, 1), "small dynamic"),
    ("small dynamic d", ("const", 8, 8, 1), "small dynamic"),                # chosen, not searched: a square flat frame
    ("dynamic at the stored size a", ("levels", 5, 1, 0), "narrow dynamic"),
    ("dynamic at the stored size b", ("levels", 6, 1, 0), "narrow dynamic"),
    ("2 * stride == 32768", ("aba", 5461, 5, 1), "distance 32768"),
    ("2 * stride == 32774", ("aba", 5462, 5, 1), "no match, stored"),
    ("stride == 32767", ("ramp", 10922, 3, 1), "distance 32767"),
    ("stride == 32770", ("ramp", 10923, 3, 1), "stride dropped"),
    ("stored, 2 * 65535", ("noise", 171, 255, 1), "whole stored blocks"),
    ("stored, one row less", ("noise", 171, 254, 1), "partial stored block"),
    ("stored, one row more", ("noise", 171, 256, 1), "partial stored block"),
    ("stored last segment", ("flat+noise", 171, 300, 1), "dynamic then stored"),
    ("match ends the segment at 258", ("checks", 57, 765, 0), "ends with 258"),
    ("match cut short by the segment", ("checks", 20, 2151, 0), "cut short"),
    ("match across the boundary", ("checks", 57, 765, 0), "reaches back"),
]

# (name, (kind, w, h, seed), row, the filters that share the row's smallest score, in Go's order: the first takes the row); --search
FILTER_CASES = [
    ("Average", ("tiny", 3, 2, 0), 1, (3,)),
    ("Up", ("tiny", 4, 3, 1), 1, (2,)),
    ("Paeth", ("tiny", 4, 3, 1), 2, (4,)),
    ("Up = Paeth", ("tiny", 4, 2, 4), 1, (2, 4)),
    ("Sub", ("tiny", 4, 3, 7), 2, (1,)),
    ("Sub = Average", ("tiny", 3, 3, 27), 1, (1, 3)),
    ("None", ("tiny", 3, 3, 27), 2, (0,)),
    ("None = Sub", ("tiny", 3, 3, 57), 2, (0, 1)),
    ("Paeth = None", ("tiny", 3, 2, 126), 1, (4, 0)),
]

# frames of one shape for the batch entry: (w, h, [(kind, seed)]).  The first mixes colour types 2 and 6, stored and dynamic segments
# and a frame that reaches the literal/length limit; the test runs it tightly packed and with padded rows and frames.
BATCHES = [
    (109, 286, [("fib", 0), ("noise", 1), ("alpha", 1), ("const", 3), ("checks", 0)]),
    (29, 1, [("levels", 1), ("levels", 4), ("const", 3), ("alpha", 2), ("noise", 1)]),
    (5, 1, [("const", 1), ("levels", 0), ("noise", 1), ("alpha", 1)]),
]


def cases():
    return [(name, frame(*rec), prop) for name, rec, prop in CASES]


def recipes():
    """the frames of CASES and FILTER_CASES, each once"""
    return sorted({rec for _, rec, _ in CASES} | {rec for _, rec, _, _ in FILTER_CASES})


def batch_frames(k):
    w, h, members = BATCHES[k]
    return [frame(kind, w, h, seed) for kind, seed in members]


def lay_out(frames, extra_stride, extra_frame):
    """frames of one shape -> (bytes of the allocation, stride, frame stride); the padding is 0xA5, alpha included, so that a kernel
    reading it would show"""
    h, w = frames[0].shape[:2]
    stride = 4 * w + extra_stride
    fs = h * stride + extra_frame
    buf = np.full(len(frames) * fs, 0xA5, np.uint8)
    for i, f in enumerate(frames):
        buf[i * fs:i * fs + h * stride].reshape(h, stride)[:, :4 * w] = f.reshape(h, 4 * w)
    return buf, stride, fs


# ---- the search ------------------------------------------------------------------------------------------------------------------
def _search():
    def first(label, prop, recs, want=1):
        got = []
        for rec in recs:
            ok, fig = PROPERTIES[prop](report(frame(*rec))) if isinstance(prop, str) else prop(rec)
            if ok:
                got.append(rec)
                print("%-28s %r  # %s" % (label, rec, fig), flush=True)
                if len(got) == want:
                    break
        if len(got) < want:
            print("%-28s only %d of %d found" % (label, len(got), want))
        return got
    sizes = [(109, 286), (252, 172), (150, 200), (200, 180), (120, 230), (300, 100)]
    fibs = [("fib", w, h, s) for s in range(40) for w, h in sizes]
    first("lit limit", "lit limit", fibs, 2)
    first("cl limit", "cl limit", fibs, 2)
    first("no match", "no match", [("levels", w, 1, s) for s in range(10) for w in range(29, 58, 7)], 3)
    first("one distance symbol", "one distance symbol", [("const", w, 1, 3) for w in (300, 100, 30)], 1)
    small = [(k, w, h, s) for w in range(1, 12) for h in range(1, 12) for k, s in (("const", 1), ("levels", 0), ("levels", 1))]
    small.sort(key=lambda r: r[1] * r[2])
    first("small dynamic", "small dynamic", small, 4)
    first("narrow dynamic", "narrow dynamic", [("levels", w, h, s) for s in range(6) for w in range(3, 40) for h in (1, 2, 3)], 2)
    # the sizes the window and the stored blocks ask for: the first seed that has the property
    for prop, kind, w, h in (("distance 32768", "aba", 5461, 5), ("no match, stored", "aba", 5462, 5), ("distance 32767", "ramp", 10922, 3),
                             ("stride dropped", "ramp", 10923, 3), ("whole stored blocks", "noise", 171, 255),
                             ("partial stored block", "noise", 171, 254), ("partial stored block", "noise", 171, 256),
                             ("dynamic then stored", "flat+noise", 171, 300)):
        first(prop, prop, [(kind, w, h, seed) for seed in range(1, 6)], 1)
    # 16 x 16 checks over two segments and a row: the light test looks at segment 0's last token only, the property confirms
    def last_token(rec):
        bpp, w, _, data = pm.filtered_stream(frame(*rec))
        best_len, _, segs = pm.best_matches(data, w, bpp)
        pos = pm.parse(best_len, *segs[0])
        return int(best_len[pos[-1]]), int(segs[0][1] - pos[-1])
    caps = [("checks", w, 2 * (-(-pm.SEG_MIN // (1 + 3 * w))) + 1, 0) for w in range(20, 140)]
    kept = first("ends with 258", "ends with 258", (r for r in caps if last_token(r) == (pm.MAX_MATCH, pm.MAX_MATCH)), 1)
    kept += first("cut short", "cut short", (r for r in caps if pm.MIN_MATCH <= last_token(r)[0] == last_token(r)[1] < pm.MAX_MATCH), 1)
    first("reaches back", "reaches back", kept, 1)          # among the frames just kept
    # filter winners and ties among tiny frames
    names = {0: "None", 1: "Sub", 2: "Up", 3: "Average", 4: "Paeth"}
    wanted = [(t,) for t in range(5)] + [(GO_ORDER[i], GO_ORDER[i + 1]) for i in range(4)]
    found = {}
    for seed in range(60000):
        if len(found) == len(wanted):
            break
        w, h = 3 + seed % 3, 2 + seed % 2
        rec = ("tiny", w, h, seed)
        _, types, _, scores = plain_filter(frame(*rec), want_scores=True)
        for y in range(1, h):
            lo = min(scores[y].values())
            tie = tuple(t for t in GO_ORDER if scores[y][t] == lo)
            if tie in wanted and tie not in found:
                found[tie] = (rec, y)
                print("    (%r, %r, %d, %r)," % (" = ".join(names[t] for t in tie), rec, y, tie), flush=True)
    frame.cache_clear()


def _report():
    for name, f, prop in cases():
        ok, fig = PROPERTIES[prop](report(f))
        print("%-34s %-5s %s" % (name, ok, fig))


if __name__ == "__main__":
    import sys
    _search() if "--search" in sys.argv else _report()
