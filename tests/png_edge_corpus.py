"""PNG files whose zlib streams use what zlib never writes (tests/deflate_writer.py): distances 32507 .. 32768, Go-style code-length
sequences whose repeats cross HLIT, 15-bit literal / length / distance codes on the symbols actually used, stored blocks of every length
up to 65535 at every bit offset, empty stored blocks, hundreds of one-symbol blocks, fixed blocks after dynamic ones; and raw lengths of
k * 16384 - 1, k * 16384 and k * 16384 + 1 (also through zlib's Z_RLE, Z_HUFFMAN_ONLY and Z_FIXED).

Every file is built from the filtered stream the test chose, so the test knows the frame it expects: corpus() -> [Case] with the file,
the filtered stream (what zlib.decompress and png_decode_model.inflate must give) and the frame in the layout of the type Go returns."""
import struct
import zlib
from dataclasses import dataclass

import numpy as np

import deflate_writer as dw
import png_corpus as pc
import png_decode_model as dm

FAR = (32768, 32767, 32507, 32600, 32700)
NEAR = (1, 2, 3, 64, 65)
# one distance per distance symbol (the middle of its range)
EVERY_DIST = tuple(dw.DIST_BASE[s] + (1 << dw.DIST_EXTRA[s]) // 2 for s in range(30))


@dataclass
class Case:
    name: str
    data: bytes          # the PNG file
    raw: bytes           # the filtered stream
    frame: np.ndarray    # Go's Pix, h x (w * bytes per pixel)
    w: int
    h: int
    kind: int
    stream: bytes        # the zlib stream


def source(n, row, seed, dists=FAR + NEAR, p_copy=0.6, alphabet=256):
    """n bytes of segments (20 .. 300 bytes) that are fresh random bytes or copies from one of `dists` back; then every row start
    (a multiple of `row`) is set to 0: filter None on every row"""
    rng = np.random.default_rng(seed)
    buf = np.zeros(n, np.uint8)
    i = 0
    while i < n:
        seg = min(int(rng.integers(20, 300)), n - i)
        cands = [d for d in dists if d <= i]
        if cands and rng.random() < p_copy:
            d = int(cands[int(rng.integers(0, len(cands)))])
            if d >= seg:
                buf[i:i + seg] = buf[i - d:i - d + seg]
            else:
                buf[i:i + seg] = np.resize(buf[i - d:i], seg)
        else:
            buf[i:i + seg] = rng.integers(0, alphabet, seg)
        i += seg
    buf[::row] = 0
    return buf.tobytes()


def _file(raw, w, h, ctype, depth, stream, plte=None):
    out = dm.SIG + pc.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
    if plte is not None:
        out += pc.chunk(b"PLTE", bytes(np.asarray(plte, np.uint8).ravel()))
    return out + pc.chunk(b"IDAT", stream) + pc.chunk(b"IEND", b"")


def case(name, raw, w, h, ctype, depth, blocks, plte=None):
    """the file of the filtered stream `raw` written as `blocks`; the frame from raw's rows (every filter byte 0)"""
    bpp, rowbytes = dm.geometry(ctype, depth, w)
    assert len(raw) == h * rowbytes and not any(raw[::rowbytes])
    stream = dw.write(blocks, raw)
    rows = np.frombuffer(raw, np.uint8).reshape(h, rowbytes)[:, 1:]
    frame = dm.convert(rows, ctype, depth, w, h, None)
    return Case(name, _file(raw, w, h, ctype, depth, stream, plte), raw, frame, w, h, dm.kind_of(ctype, depth, False), stream)


def long_lit(tok, k_lit=6, k_len=3):
    """explicit literal / length lengths: 15 bits on the block's k_lit most frequent literals and k_len most frequent length symbols"""
    ls, _ = tok.symbols()
    f = np.bincount(ls, minlength=286)[:286]
    f[256] += 1
    order = [int(s) for s in np.argsort(-f, kind="stable") if f[s] > 0]
    lits = [s for s in order if s < 256][:k_lit]
    lens = [s for s in order if s > 256][:k_len]
    rest = order + [s for s in range(286) if f[s] == 0]                  # unused symbols take what is left of the Kraft sum
    return dw.complete_lengths(rest, lits + lens, 286)


def long_dist(tok, fixed=None):
    """explicit distance lengths over all 30 symbols: 15 bits on every symbol the block uses (or `fixed` {symbol: length}); the
    unused ones get the short codes"""
    _, ds = tok.symbols()
    f = np.bincount(ds[ds >= 0], minlength=30)[:30]
    used = [s for s in range(30) if f[s]]
    fixed = fixed if fixed is not None else {s: 15 for s in used}
    order = [s for s in range(30) if s not in fixed]
    return dw.complete_lengths(order, fixed, 30)


def dynamic(tok, codegen="zlib", lit=None, dist=None):
    return {"kind": "dynamic", "tokens": tok, "codegen": codegen, "lit": lit, "dist": dist}


def far_case(name, w, h, ctype, depth, seed, nblocks=6, dists=FAR + NEAR):
    """matches up to 32768 back; dynamic blocks alternating zlib / Go code-length sequences, computed / explicit long codes, with a
    fixed block among them"""
    bpp, rowbytes = dm.geometry(ctype, depth, w)
    raw = source(h * rowbytes, rowbytes, seed, dists + (rowbytes,))
    tok = dw.match(raw, dists + (rowbytes,))
    blocks = []
    for k, t in enumerate(tok.split(nblocks)):
        style = ("go", "zlib")[k % 2]
        if k % 3 == 2:
            blocks.append({"kind": "fixed", "tokens": t})
        elif k % 3 == 1:
            d = long_dist(t)
            blocks.append(dynamic(t, style, _cross(long_lit(t), d, seed % 2 == 0) if style == "go" else long_lit(t), d))
        else:
            blocks.append(dynamic(t, style))
    return case(name, raw, w, h, ctype, depth, blocks)


def every_dist_case(name, seed):
    """every distance symbol used; each block puts lengths 9 .. 15 on eight of the symbols it uses (those no block had yet first),
    Go's code-length sequence with a repeat across HLIT"""
    w, h = 511, 200                                                      # gray 8, 512-byte rows
    raw = source(w * h + h, w + 1, seed, EVERY_DIST, p_copy=0.8)
    tok = dw.match(raw, EVERY_DIST)
    blocks = []
    todo = list(range(30))
    for b, t in enumerate(tok.split(5)):
        _, ds = t.symbols()
        used = set(ds[ds >= 0].tolist())
        pick = [s for s in todo if s in used][:8]
        pick += [s for s in range(30) if s not in pick][:8 - len(pick)]
        todo = [s for s in todo if s not in pick]
        longs = {s: L for s, L in zip(pick, (9, 10, 11, 12, 13, 14, 15, 15))}
        dist = long_dist(t, longs)
        lit = long_lit(t)
        blocks.append(dynamic(t, "go", _cross(lit, dist), dist))
    return case(name, raw, w, h, 0, 8, blocks)


def _cross(lit, dist, span=True):
    """lit with lengths swapped so that its last symbol (span: its last two) has distance symbol 0's length and the one before
    does not (span: the one before those): Go's one run-length sequence then has a repeat across HLIT (span) or a repeat code 16
    at HLIT that repeats the last literal / length length into the distance code (zlib's two sequences never do either)"""
    lit = list(lit)
    last = max(s for s in range(286) if lit[s])
    want = dist[0]
    same = (last - 1, last) if span else (last,)
    for t in same:
        if lit[t] != want:
            s = next((s for s in range(last - 2) if lit[s] == want), None)
            if s is not None:
                lit[s], lit[t] = lit[t], lit[s]
    t = last - len(same)
    if lit[t] == want:
        s = next((s for s in range(last - 2) if lit[s] and lit[s] != want), None)
        if s is not None:
            lit[s], lit[t] = lit[t], lit[s]
    return lit


def stored_case(name, seed):
    """stored blocks of 65535, 0 (between compressed blocks), 1, 8191 .. 8193 and 16383 .. 16385 bytes, and stored headers at all
    eight bit offsets (each behind a fixed block of literals whose 9-bit codes set the offset)"""
    w, h = 1023, 200                                                     # gray 8, 1024-byte rows: 204800 bytes
    rowbytes = w + 1
    raw = bytearray(source(w * h + h, rowbytes, seed, FAR + NEAR))
    blocks, p = [], 0

    def stored(n):
        nonlocal p
        blocks.append({"kind": "stored", "data": bytes(raw[p:p + n])})
        p += n

    def fixed_to(offset):
        """a fixed block of literals after a byte-aligned point: 10 + 9 m + 8 t bits, so the next header sits at (2 + m) mod 8"""
        nonlocal p
        q, m = 0, 0
        while True:
            q += 1
            m += raw[p + q - 1] >= 144
            if (2 + m) % 8 == offset:
                break
        blocks.append({"kind": "fixed", "tokens": dw.literals(raw[p:p + q])})
        p += q

    stored(65535)
    for off in range(8):
        fixed_to(off)
        stored((1, 8191, 8192, 8193, 16383, 16384, 16385, 300)[off])
    t = dw.match(bytes(raw), FAR + NEAR, p, p + 20000)
    blocks.append(dynamic(t))
    p += 20000
    stored(0)                                                            # what a sync flush writes
    stored(0)
    t = dw.match(bytes(raw), FAR + NEAR, p, len(raw) - 100)
    blocks.append(dynamic(t, "go"))
    p = len(raw) - 100
    stored(100)
    assert p == len(raw)
    return case(name, bytes(raw), w, h, 0, 8, blocks)


def tiny_blocks_case(name, seed):
    """hundreds of one-symbol blocks: dynamic (two codes of length 1) and fixed in turn, so the fixed tables are rebuilt after every
    dynamic block; then the rest as one block"""
    w, h = 63, 40
    rowbytes = w + 1
    raw = source(w * h + h, rowbytes, seed, NEAR)
    tok = dw.match(raw, NEAR)
    blocks = []
    for k in range(400):
        t = dw.Tokens(tok.lit[k:k + 1], tok.length[k:k + 1], tok.dist[k:k + 1])
        blocks.append(dynamic(t, ("go", "zlib")[k % 3 == 0]) if k % 2 == 0 else {"kind": "fixed", "tokens": t})
    rest = dw.Tokens(tok.lit[400:], tok.length[400:], tok.dist[400:])
    blocks.append({"kind": "fixed", "tokens": rest})
    return case(name, raw, w, h, 0, 8, blocks)


# raw lengths at and either side of k * 16384 (gray 8: rowbytes x h)
UNIT_EDGES = [(128, 127), (127, 128), (144, 113), (216, 151), (255, 128), (98, 331)]


def unit_edge_cases(seed):
    """the writer's far / long-code stream and zlib's Z_RLE, Z_HUFFMAN_ONLY and Z_FIXED streams of each length"""
    out = []
    for k, (w, h) in enumerate(UNIT_EDGES):
        n = (w + 1) * h
        c = far_case("raw %d (%d x %d) writer" % (n, w, h), w, h, 0, 8, seed + k, nblocks=3)
        out.append(c)
        for sname, strat in (("rle", zlib.Z_RLE), ("huffman", zlib.Z_HUFFMAN_ONLY), ("fixed", zlib.Z_FIXED)):
            rows = np.frombuffer(c.raw, np.uint8).reshape(h, w + 1)[:, 1:]
            f = pc.write(rows, 0, 8, filters=(k % 5, 4, 2, 3), strategy=strat, level=9)
            out.append(_from_file("raw %d (%d x %d) zlib %s" % (n, w, h, sname), f, rows, 0, 8))
    return out


def _from_file(name, f, samples, ctype, depth):
    """a Case of a png_corpus file: the frame from the samples the test chose"""
    st, fields = dm.parse(f)
    assert st == dm.OK
    stream = b"".join(fields["idat"])
    w, h = fields["w"], fields["h"]
    rows = pc.pack_rows(np.asarray(samples), ctype, depth)
    return Case(name, f, zlib.decompress(stream), dm.convert(rows, ctype, depth, w, h, None), w, h,
                dm.kind_of(ctype, depth, False), stream)


def corpus(seed=11):
    """the CPU corpus: every edge the coverage test asks for, raw lengths of at most ~200 KiB"""
    out = [far_case("far gray8 500x160", 500, 160, 0, 8, seed),
           far_case("far rgb8 200x120", 200, 120, 2, 8, seed + 1),
           far_case("far rgba8 97x150", 97, 150, 6, 8, seed + 2, nblocks=9),
           every_dist_case("every distance symbol", seed + 3),
           stored_case("stored", seed + 4),
           tiny_blocks_case("one-symbol blocks", seed + 5)]
    return out + unit_edge_cases(seed + 10)


def large(seed=21):
    """GPU-only frames: 1920 x 1080 RGB 8 and 1024 x 768 RGBA 8 with the far matches and long codes"""
    return [far_case("far rgb8 1920x1080", 1920, 1080, 2, 8, seed, nblocks=24),
            far_case("far rgba8 1024x768", 1024, 768, 6, 8, seed + 1, nblocks=12)]
