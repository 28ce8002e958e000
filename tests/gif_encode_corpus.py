"""Frames that put gif.Encode on the GPU (csrc/ipx_gif.hip) at the edges of its LZW coder and of its dither, for
tests/test_encode_edge_corpus.py (CPU: every case has the property it is there for) and tests/test_gif_encode_edges_gpu.py (GPU: every
case byte for byte against tests/gif_model.py and, independently, decoded by gif_decode_model.lzw_decode and by Pillow to the indices).
Everything is built from rules and seeds; nothing large is committed.  `python tests/gif_encode_corpus.py --search` is the CPU search
(with trace_lzw below) that found the committed run lengths and prefix lengths; `--report` prints every case's figures.

All 256 Plan 9 colours are distinct, and a pixel that IS a palette colour leaves no error behind (alpha included: every entry has alpha
0xffff).  So an opaque frame made of palette colours dithers to exactly the indices one chooses, and every LZW input can be fed through
the public entries: index_frame() builds such a frame.

The LZW cases: the hand-derived known answers of golden/gif_kats.json; prefixes of the "no repeats" sequence, in which every index goes
out as a literal code, so that hi after Close is 257 + N (N = 255: the last incHi reaches 512 and EOF is 10 bits wide; N = 3838: it
reaches 4095, a clear goes out before EOF and EOF is 9 bits wide); a run in front of that sequence, which delays the 4095 clear to the
last index of the 4096-index staging chunk and to the first of the next; frames of exactly 4096, 4097 and 8192 pixels; data that ends on
a full 255-byte sub-block, one byte into a new one and one byte short of one; the longest dictionary chains (one index 65535 times).

The dither cases (each small enough for gif_model.dither_scalar): colours and alpha at both ends of the range next to mid values, so that
the error terms push the sums below 0 and above 0xffff; colours at equal distance from two palette entries, where the first minimum
decides; frames 1, 2, 3 and 5 pixels wide over more rows than one band holds; heights at and around the wave of 64 rows.
The alpha sum cannot pass 0xffff: the alpha error of every pixel is (clamped sum) - 0xffff <= 0, so only its lower clamp can fire.
"""
import functools
import json
import os

import numpy as np

import gif_model as gm
from png_encode_corpus import lay_out  # noqa: F401  (the GPU test lays its batches out with it)

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 4096            # kLzwChunk of ipx_gif.hip: indices staged in LDS at a time
HEADER = len(gm.header(1, 1))


def index_frame(idx):
    """h x w indices -> the opaque h x w x 4 frame of their Plan 9 colours"""
    idx = np.asarray(idx, np.uint8)
    f = np.empty(idx.shape + (4,), np.uint8)
    f[..., :3] = gm.PLAN9[idx]
    f[..., 3] = 255
    return f


@functools.lru_cache(maxsize=None)
def kats():
    with open(os.path.join(HERE, "golden", "gif_kats.json")) as fh:
        return json.load(fh)["cases"]


@functools.lru_cache(maxsize=None)
def no_repeats():
    """5000 indices in which no pair of neighbours occurs twice (golden/make_gif_kats.py): the dictionary never matches"""
    seq = next(c for c in kats() if c["name"].startswith("no repeats"))["index"]
    assert len({(a, b) for a, b in zip(seq, seq[1:])}) == len(seq) - 1
    return np.array(seq, np.uint8)


# ---- a tracing copy of the coder -------------------------------------------------------------------------------------------------
def trace_lzw(index):
    """compress/lzw's writer (LSB, literal width 8) over the indices, as a list of events only -> dict:
    nbits / nbytes of the data, clears: the 0-based index being consumed when each 4095 clear went out (len(index) for the one of Close),
    final_hi: what the incHi of Close raised hi to, eof_width, codes: how many codes went out, longest: the longest string of a code"""
    data = [int(v) for v in np.asarray(index).reshape(-1)]
    width, hi, overflow = 9, 257, 512
    nbits, ncodes, clears, table, length = 9, 1, [], {}, {}

    def inc_hi(at):
        nonlocal width, hi, overflow, nbits, ncodes
        hi += 1
        reached = hi
        if hi == overflow:
            width += 1
            overflow <<= 1
        if hi == 4095:
            nbits += width
            ncodes += 1
            clears.append(at)
            width, hi, overflow = 9, 257, 512
            table.clear()
            length.clear()
            return False, reached
        return True, reached
    code, longest = data[0], 1
    for at in range(1, len(data)):
        key = (code, data[at])
        if key in table:
            code = table[key]
            continue
        nbits += width
        ncodes += 1
        ok, _ = inc_hi(at)
        if ok:
            table[key] = hi
            length[hi] = length.get(code, 1) + 1
            longest = max(longest, length[hi])
        code = data[at]
    nbits += width
    ncodes += 1
    _, final_hi = inc_hi(len(data))
    eof_width = width
    nbits += width
    ncodes += 1
    return {"nbits": nbits, "nbytes": (nbits + 7) // 8, "clears": clears, "final_hi": final_hi, "eof_width": eof_width,
            "codes": ncodes, "longest": longest}


def lzw_payload(stream, w, h):
    """the sub-blocks of a one-frame stream of gif.Encode -> (LZW data, sub-block sizes); header, terminator and trailer are checked"""
    stream = bytes(stream)
    assert stream[:HEADER] == gm.header(w, h)
    p, data, sizes = HEADER, bytearray(), []
    while stream[p]:
        n = stream[p]
        data += stream[p + 1:p + 1 + n]
        assert len(stream) > p + 1 + n
        sizes.append(n)
        p += 1 + n
    assert stream[p:] == b"\x00\x3b"
    assert all(n == 255 for n in sizes[:-1])
    return bytes(data), sizes


def check_stream(stream, idx):
    """the independent check of one stream: the reader of compress/lzw and Pillow both return the indices"""
    import io

    from PIL import Image

    import gif_decode_model as gd
    h, w = idx.shape
    data, _ = lzw_payload(stream, w, h)
    pix, how, used = gd.lzw_decode(data, 8, w * h)
    assert how == "eof" and used == len(data)
    assert pix == idx.tobytes()
    im = Image.open(io.BytesIO(stream))
    assert im.format == "GIF" and im.mode == "P" and im.size == (w, h)
    assert im.getpalette()[:768] == gm.PLAN9.reshape(-1).tolist()
    np.testing.assert_array_equal(np.array(im), idx)


# ---- the LZW cases: (name, indices h x w, property) ------------------------------------------------------------------------------------
RUN_FOR_4095 = 281      # a run of index 200 this long in front of the no-repeats sequence: the clear goes out while index 4095 is consumed
RUN_FOR_4096 = 282      # ... while index 4096, the first of the second staged chunk, is consumed
RESIDUE_PREFIX = {0: 431, 1: 432, 254: 832}     # data length mod 255 -> the prefix of the no-repeats sequence that gives it


def run_then_no_repeats(run, n):
    return np.concatenate([np.full(run, 200, np.uint8), no_repeats()[:n - run]])


def _shape(seq, how):
    seq = np.asarray(seq, np.uint8)
    if how == "row":
        return seq.reshape(1, -1)
    if how == "col":
        return seq.reshape(-1, 1)
    return seq.reshape(how[1], how[0])


def _p_final(hi, width, clears_at_close):
    def prop(t, n):
        ok = t["final_hi"] == hi and t["eof_width"] == width and (t["clears"] == [n]) == clears_at_close
        return ok, "final hi %d, EOF %d bits wide, 4095 clears at %s" % (t["final_hi"], t["eof_width"], t["clears"])
    return prop


def _p_clear_at(at):
    def prop(t, n):
        return t["clears"][:1] == [at] and n > at + 1, "4095 clear while index %s of %d is consumed" % (t["clears"], n)
    return prop


def _p_residue(r):
    def prop(t, n):
        return t["nbytes"] % 255 == r and t["nbytes"] > 255, "%d bytes of LZW data = %d * 255 + %d" % (t["nbytes"], t["nbytes"] // 255, t["nbytes"] % 255)
    return prop


def _p_npix(npix):
    def prop(t, n):
        return n == npix, "%d pixels, %d codes, 4095 clears at %s" % (n, t["codes"], t["clears"])
    return prop


def _p_longest(t, n):
    return n == 65535 and t["longest"] >= 361, "longest dictionary string %d, %d codes" % (t["longest"], t["codes"])


def _p_bound(t, n):
    total = HEADER + t["nbytes"] + -(-t["nbytes"] // 255) + 2
    return total <= gm.size_bound(50, 100) and len(t["clears"]) == 1, "stream of %d bytes, bound %d" % (total, gm.size_bound(50, 100))


def _p_kat(t, n):
    return True, "%d bytes of LZW data, %d codes" % (t["nbytes"], t["codes"])


@functools.lru_cache(maxsize=None)
def lzw_cases():
    nr = no_repeats()
    rng = np.random.default_rng(20261018)
    out = []
    for c in kats():
        out.append(("kat: " + c["name"], _shape(c["index"], "row"), _p_kat))
    widths = {254: 9, 255: 10, 256: 10, 766: 10, 767: 11, 768: 11, 1790: 11, 1791: 12, 1792: 12, 3837: 12, 3838: 9, 3839: 9}
    for k, (n, wd) in enumerate(widths.items()):
        hi = 257 + n if n <= 3838 else 258
        out.append(("no repeats, %d" % n, _shape(nr[:n], "row" if k % 2 else "col"), _p_final(hi, wd, n == 3838)))
    out.append(("clear on the last index of a chunk", _shape(run_then_no_repeats(RUN_FOR_4095, 4200), "row"), _p_clear_at(CHUNK - 1)))
    out.append(("clear on the first index of a chunk", _shape(run_then_no_repeats(RUN_FOR_4096, 4200), (60, 70)), _p_clear_at(CHUNK)))
    for w, h in ((64, 64), (17, 241), (128, 64)):
        out.append(("%d pixels" % (w * h), rng.integers(0, 256, (h, w), dtype=np.uint8), _p_npix(w * h)))
    for r, n in sorted(RESIDUE_PREFIX.items()):
        out.append(("data length = %d mod 255" % r, _shape(nr[:n], "row" if r else "col"), _p_residue(r)))
    out.append(("one index along 65535 x 1", np.full((1, 65535), 5, np.uint8), _p_longest))
    out.append(("one index along 1 x 65535", np.full((65535, 1), 5, np.uint8), _p_longest))
    out.append(("size bound, no repeats 50 x 100", _shape(nr[:5000], (50, 100)), _p_bound))
    for _, idx, _ in out:
        idx.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lzw_batches():
    """index frames of one shape for the batch entry: [(w, h, [indices h x w])]"""
    nr = no_repeats()
    rng = np.random.default_rng(7)
    a = [run_then_no_repeats(RUN_FOR_4095, 4200), run_then_no_repeats(RUN_FOR_4096, 4200), nr[:4200], rng.integers(0, 256, 4200, dtype=np.uint8),
         np.full(4200, 9, np.uint8), nr[800:5000]]
    b = [nr[:3838], nr[1:3839], rng.integers(0, 4, 3838, dtype=np.uint8), nr[:3838][::-1].copy()]
    return [(70, 60, [_shape(v, (70, 60)) for v in a]), (1, 3838, [_shape(v, "col") for v in b])]


# ---- the dither cases ------------------------------------------------------------------------------------------------------------
def trace_dither(rgba):
    """drawPaletted's Floyd-Steinberg loop (image/draw), one pixel at a time, written for this module -> (indices, clamps: how often
    each channel's sum was below 0 / above 0xffff before the clamp, ties: pixels whose minimum two or more palette entries share)"""
    h, w = rgba.shape[:2]
    pal = (gm.PLAN9.astype(np.int64) * 0x101).tolist()
    src = rgba.astype(np.int64) * 0x101
    cur = np.zeros((w + 2, 4), np.int64)
    out = np.zeros((h, w), np.uint8)
    low, high, ties = [0] * 4, [0] * 4, 0
    palv = np.array(pal, np.int64)
    for y in range(h):
        nxt = np.zeros((w + 2, 4), np.int64)
        for x in range(w):
            q = cur[x + 1]
            e = src[y, x] + np.sign(q) * (np.abs(q) // 16)            # Go's / truncates toward zero
            for c in range(4):
                low[c] += int(e[c] < 0)
                high[c] += int(e[c] > 0xFFFF)
            e = np.clip(e, 0, 0xFFFF)
            d = (((e[:3] - palv) & 0xFFFFFFFF) ** 2 & 0xFFFFFFFF) >> 2   # sqDiff in uint32; the alpha term is the same for every entry
            s = d.sum(axis=1)
            best = int(np.argmin(s))
            ties += int((s == s[best]).sum() > 1)
            out[y, x] = best
            err = e - np.array(pal[best] + [0xFFFF], np.int64)
            nxt[x] += 3 * err
            nxt[x + 1] += 5 * err
            nxt[x + 2] += err
            cur[x + 2] += 7 * err
        cur = nxt
    return out, {"low": low, "high": high}, ties


def _premultiplied(rgb, a):
    f = np.empty(rgb.shape[:2] + (4,), np.int64)
    f[..., :3] = rgb * a[..., None] // 255
    f[..., 3] = a
    return f.astype(np.uint8)


def _noisy(w, h, seed):
    """gradients, noise and alpha of every value in places (premultiplied)"""
    rng = np.random.default_rng([seed, w, h])
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 3 % 256], axis=2) + rng.integers(-40, 41, (h, w, 3))
    a = np.where(rng.random((h, w)) < 0.4, rng.integers(0, 256, (h, w)), 255)
    return _premultiplied(rgb.clip(0, 255), a)


def _extremes(w, h, kind):
    """0 / 255 next to mid values (100 picks 0x66 from above, 200 picks 0xbb from below), alpha 0, 1, 254, 255 in blocks"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "checker":
        v = np.where((xx + yy) % 2 == 0, np.where(yy % 4 < 2, 0, 255), np.where(xx % 4 < 2, 100, 200))
    else:
        v = np.array([0, 100, 255, 200, 0, 200, 255, 100])[xx % 8]
    rgb = np.stack([v, np.roll(v, 1, axis=1), 255 - v], axis=2)
    a = np.array([255, 254, 0, 1, 255, 0, 254, 255])[(xx // 3 + yy // 2) % 8]
    return _premultiplied(rgb, a)


@functools.lru_cache(maxsize=None)
def tie_colours():
    """opaque colours at exactly the same distance from two palette entries, with no third entry nearer: the first of the two wins.
    Midpoints of pairs of entries whose components differ by even amounts, kept when the pair is the minimum."""
    p = gm.PLAN9.astype(np.int64)
    out = []
    for i in range(256):
        for j in range(i + 1, 256):
            if ((p[i] + p[j]) % 2).any():
                continue
            c = (p[i] + p[j]) // 2
            s = ((((c - p) * 0x101) ** 2) >> 2).sum(axis=1)
            if s[i] == s[j] == s.min() and (s == s.min()).sum() == 2:
                out.append((tuple(int(v) for v in c), i, j))
    return out


# (name, frame, IPX_GIF_WAVES or None)
@functools.lru_cache(maxsize=None)
def dither_cases():
    out = [("extremes, checker 24 x 24", _extremes(24, 24, "checker"), None),
           ("extremes, stripes 31 x 17", _extremes(31, 17, "stripes"), None),
           ("1 x 130, one wave", _noisy(1, 130, 1), "1"),
           ("2 x 200, one wave", _noisy(2, 200, 2), "1"),
           ("3 x 1030, 16 waves", _noisy(3, 1030, 3), "16"),
           ("5 x 1024, 16 waves", _noisy(5, 1024, 4), "16"),
           ("9 x 64", _noisy(9, 64, 5), None),
           ("9 x 65", _noisy(9, 65, 6), None),
           ("7 x 128", _noisy(7, 128, 7), None)]
    ties = tie_colours()
    grid = np.array([c for c, _, _ in ties[:121]], np.uint8).reshape(11, 11, 3)
    out.append(("tie colours 11 x 11", _premultiplied(grid.astype(np.int64), np.full((11, 11), 255)), None))
    for _, f, _ in out:
        f.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dither_reference(k):
    """gm.dither_scalar of dither case k, computed once"""
    idx = gm.dither_scalar(dither_cases()[k][1])
    idx.setflags(write=False)
    return idx


def tie_frames():
    """one 1 x 1 frame per tie colour (no error reaches the pixel), and the index the first minimum gives"""
    t = tie_colours()
    f = np.empty((len(t), 1, 1, 4), np.uint8)
    f[:, 0, 0, :3] = [c for c, _, _ in t]
    f[..., 3] = 255
    return f, np.array([i for _, i, _ in t], np.uint8)


# ---- the search ------------------------------------------------------------------------------------------------------------------
def _search():
    for target, name in ((CHUNK - 1, "RUN_FOR_4095"), (CHUNK, "RUN_FOR_4096")):
        for run in range(2, 700):
            t = trace_lzw(run_then_no_repeats(run, 4200))
            if t["clears"][:1] == [target]:
                print("%s = %d" % (name, run))
                break
        else:
            print("%s: not found" % name)
    nr = no_repeats()
    found = {}
    for n in range(300, 3000):
        r = trace_lzw(nr[:n])["nbytes"] % 255
        if r in (0, 1, 254) and r not in found:
            found[r] = n
    print("RESIDUE_PREFIX = %r" % found)
    print("%d tie colours" % len(tie_colours()))


def _report():
    for name, idx, prop in lzw_cases():
        print("%-40s %s" % (name, prop(trace_lzw(idx), idx.size)))
    for name, f, waves in dither_cases():
        _, clamps, ties = trace_dither(f)
        print("%-40s clamps %s, %d ties" % (name, clamps, ties))


if __name__ == "__main__":
    import sys
    _search() if "--search" in sys.argv else _report()
