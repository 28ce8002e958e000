"""Writes png_dec_kats.json: hand-derived PNG files and what png.Decode (as restated in DESIGN.md section 4.10) answers for each, for
tests/test_png_decode_model.py.  Written without the model: the deflate bits are laid down by hand (stored blocks, fixed codes, dynamic
codes from explicit code lengths), rows mostly use filter None so the pixels are the bytes written, and the filtered and converted
answers are spelled out.  Only the library's zlib.crc32 / zlib.adler32 are used, for the checksums.

  python tests/golden/make_png_dec_kats.py      # rewrites tests/golden/png_dec_kats.json"""
import json
import os
import struct
import zlib

OK, INVALID, UNSUPPORTED = 0, -1, -4
GRAY, NRGBA, RGBA, PALETTED, GRAY16, RGBA64, NRGBA64 = range(7)
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(t, d, crc=None):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) if crc is None else crc)


def ihdr(w, h, depth, ctype, comp=0, filt=0, il=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, comp, filt, il))


class BW:
    """deflate bits: fields LSB first, Huffman codes most significant bit first"""

    def __init__(self):
        self.b = []

    def put(self, v, n):
        self.b += [(v >> k) & 1 for k in range(n)]

    def code(self, c, n):
        self.b += [(c >> k) & 1 for k in range(n - 1, -1, -1)]

    def fixed_lit(self, v):
        if v < 144:
            self.code(0x30 + v, 8)
        elif v < 256:
            self.code(0x190 + v - 144, 9)
        elif v < 280:
            self.code(v - 256, 7)
        else:
            self.code(0xC0 + v - 280, 8)

    def align(self):
        while len(self.b) % 8:
            self.b.append(0)

    def bytes(self):
        self.align()
        return bytes(sum(self.b[i + k] << k for k in range(8)) for i in range(0, len(self.b), 8))


def codes(lengths):
    """deflate's canonical codes (RFC 1951 3.2.2): symbol -> (code, length)"""
    bl = [0] * 16
    for n in lengths:
        if n:
            bl[n] += 1
    nxt, code = [0] * 16, 0
    for L in range(1, 16):
        code = (code + bl[L - 1]) << 1
        nxt[L] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def zwrap(deflate, data, header=b"\x78\x01", adler=None):
    return header + deflate + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def stored(data, final=1):
    return bytes([final]) + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def zstored(data):
    return zwrap(stored(data), data)


def png(w, h, depth, ctype, stream, pre=b"", idat_split=None, post=b""):
    parts = [stream] if idat_split is None else [stream[i:i + idat_split] for i in range(0, len(stream), idat_split)]
    return SIG + ihdr(w, h, depth, ctype) + pre + b"".join(chunk(b"IDAT", p) for p in parts) + post + chunk(b"IEND", b"")


def rows_none(rows):
    """filter byte 0 in front of every row"""
    return b"".join(b"\x00" + bytes(r) for r in rows)


CASES = []


def case(name, data, status, kind=None, w=None, h=None, pix=None, palette=None):
    c = {"name": name, "data": data.hex(), "status": status}
    if status == OK:
        c.update(kind=kind, w=w, h=h, pix=bytes(pix).hex())
        if palette is not None:
            c["palette"] = bytes(palette).hex()
    CASES.append(c)


def pal_bytes(entries, alphas=()):
    """256 x RGBA: the PLTE entries, tRNS alphas on the first ones, opaque black after"""
    out = bytearray()
    for k in range(256):
        if k < len(entries):
            out += bytes(entries[k]) + bytes([alphas[k] if k < len(alphas) else 255])
        else:
            out += b"\x00\x00\x00\xff"
    return out


# ---- one valid file per row of the type table (stored blocks, filter None) ----------------------------------------------------
# gray 1, 3 x 2: rows 0b101_00000, 0b010_00000 -> 255 0 255 / 0 255 0
raw = rows_none([[0xA0], [0x40]])
case("gray1 3x2", png(3, 2, 1, 0, zstored(raw)), OK, GRAY, 3, 2, [255, 0, 255, 0, 255, 0])
# gray 2, 5 x 1: samples 0 1 2 3 1 -> x 0x55: 0 85 170 255 85; bytes 0b00011011, 0b01_000000
case("gray2 5x1 odd width", png(5, 1, 2, 0, zstored(rows_none([[0x1B, 0x40]]))), OK, GRAY, 5, 1, [0, 85, 170, 255, 85])
# gray 4, 3 x 1: 0x1F, 0x80 -> 1, 15, 8 -> x 0x11: 17 255 136
case("gray4 3x1", png(3, 1, 4, 0, zstored(rows_none([[0x1F, 0x80]]))), OK, GRAY, 3, 1, [17, 255, 136])
case("gray8 2x2", png(2, 2, 8, 0, zstored(rows_none([[1, 2], [3, 4]]))), OK, GRAY, 2, 2, [1, 2, 3, 4])
# gray 8 + tRNS 0x0002: the 2 gets alpha 0 (keeps its colour)
case("gray8 trns", png(2, 1, 8, 0, zstored(rows_none([[1, 2]])), pre=chunk(b"tRNS", b"\x00\x02")), OK, NRGBA, 2, 1,
     [1, 1, 1, 255, 2, 2, 2, 0])
case("gray-alpha8", png(1, 2, 8, 4, zstored(rows_none([[9, 100], [7, 0]]))), OK, NRGBA, 1, 2, [9, 9, 9, 100, 7, 7, 7, 0])
case("rgb8 trns", png(2, 1, 8, 2, zstored(rows_none([[1, 2, 3, 4, 5, 6]])), pre=chunk(b"tRNS", b"\x00\x04\x00\x05\x00\x06")), OK, NRGBA,
     2, 1, [1, 2, 3, 255, 4, 5, 6, 0])
case("rgba8", png(1, 1, 8, 6, zstored(rows_none([[10, 20, 30, 40]]))), OK, NRGBA, 1, 1, [10, 20, 30, 40])
case("rgb8", png(2, 1, 8, 2, zstored(rows_none([[10, 20, 30, 40, 50, 60]]))), OK, RGBA, 2, 1, [10, 20, 30, 255, 40, 50, 60, 255])
case("rgb8 ignores PLTE", png(1, 1, 8, 2, zstored(rows_none([[7, 8, 9]])), pre=chunk(b"PLTE", b"\x01\x02\x03")), OK, RGBA, 1, 1,
     [7, 8, 9, 255])
E = [(200, 0, 0), (0, 200, 0), (0, 0, 200)]
# palette 1, 9 x 1: bits 1 0 1 1 0 0 0 1 | 1 -> 0xB1, 0x80
case("pal1 9x1", png(9, 1, 1, 3, zstored(rows_none([[0xB1, 0x80]])), pre=chunk(b"PLTE", bytes(sum(E[:2], ())))), OK, PALETTED, 9, 1,
     [1, 0, 1, 1, 0, 0, 0, 1, 1], pal_bytes(E[:2]))
# palette 2, index 3 past the 3 entries: stays 3, the palette pads it with opaque black
case("pal2 index past PLTE", png(4, 1, 2, 3, zstored(rows_none([[0b00011011]])), pre=chunk(b"PLTE", bytes(sum(E, ())))), OK, PALETTED,
     4, 1, [0, 1, 2, 3], pal_bytes(E))
case("pal4 trns", png(2, 1, 4, 3, zstored(rows_none([[0x21]])), pre=chunk(b"PLTE", bytes(sum(E, ()))) + chunk(b"tRNS", b"\x10\x20")),
     OK, PALETTED, 2, 1, [2, 1], pal_bytes(E, (0x10, 0x20)))
case("pal8 out-of-range index", png(2, 1, 8, 3, zstored(rows_none([[2, 200]])), pre=chunk(b"PLTE", bytes(sum(E, ())))), OK, PALETTED,
     2, 1, [2, 200], pal_bytes(E))
case("gray16", png(2, 1, 16, 0, zstored(rows_none([[1, 2, 3, 4]]))), OK, GRAY16, 2, 1, [1, 2, 3, 4])
case("rgb16", png(1, 1, 16, 2, zstored(rows_none([[1, 2, 3, 4, 5, 6]]))), OK, RGBA64, 1, 1, [1, 2, 3, 4, 5, 6, 255, 255])
case("gray16 trns", png(2, 1, 16, 0, zstored(rows_none([[1, 2, 3, 4]])), pre=chunk(b"tRNS", b"\x03\x04")), OK, NRGBA64, 2, 1,
     [1, 2, 1, 2, 1, 2, 255, 255, 3, 4, 3, 4, 3, 4, 0, 0])
case("gray-alpha16", png(1, 1, 16, 4, zstored(rows_none([[1, 2, 3, 4]]))), OK, NRGBA64, 1, 1, [1, 2, 1, 2, 1, 2, 3, 4])
case("rgb16 trns", png(1, 1, 16, 2, zstored(rows_none([[1, 2, 3, 4, 5, 6]])), pre=chunk(b"tRNS", b"\x01\x02\x03\x04\x05\x06")), OK,
     NRGBA64, 1, 1, [1, 2, 3, 4, 5, 6, 0, 0])
case("rgba16", png(1, 1, 16, 6, zstored(rows_none([[1, 2, 3, 4, 5, 6, 7, 8]]))), OK, NRGBA64, 1, 1, [1, 2, 3, 4, 5, 6, 7, 8])

# ---- rows ----------------------------------------------------------------------------------------------------------------------
# gray 8, 3 x 3: None [100 50 200]; Average [1 2 3] -> 51 52 129; Paeth [4 5 6] -> 55 60 135 (worked in DESIGN.md 4.10)
raw = b"\x00" + bytes([100, 50, 200]) + b"\x03" + bytes([1, 2, 3]) + b"\x04" + bytes([4, 5, 6])
case("filters none average paeth", png(3, 3, 8, 0, zstored(raw)), OK, GRAY, 3, 3, [100, 50, 200, 51, 52, 129, 55, 60, 135])
# Sub [10 5] -> 10 15; Up [1 1] -> 11 16
raw = b"\x01" + bytes([10, 5]) + b"\x02" + bytes([1, 1])
case("filters sub up", png(2, 2, 8, 0, zstored(raw)), OK, GRAY, 2, 2, [10, 15, 11, 16])
# Sub on RGB 8 works per channel (bpp 3): [1 2 3 1 1 1] -> 1 2 3 2 3 4
case("filter sub bpp 3", png(2, 1, 8, 2, zstored(b"\x01" + bytes([1, 2, 3, 1, 1, 1]))), OK, RGBA, 2, 1, [1, 2, 3, 255, 2, 3, 4, 255])
# sub-byte rows filter bytewise with bpp 1: gray 4, 4 x 1, Sub [0x12 0x11] -> 0x12 0x23 -> 1 2 2 3 (x 17)
case("filter sub at depth 4", png(4, 1, 4, 0, zstored(b"\x01\x12\x11")), OK, GRAY, 4, 1, [17, 34, 34, 51])
case("filter type 5", png(2, 1, 8, 0, zstored(b"\x05\x01\x02")), INVALID)

# ---- zlib / flate ---------------------------------------------------------------------------------------------------------------
ONE = rows_none([[7, 7, 7, 7, 7]])                    # gray 8, 5 x 1
G = dict(w=5, h=1, depth=8, ctype=0)


def gpng(stream, **kw):
    return png(5, 1, 8, 0, stream, **kw)


case("zlib CM 7", gpng(zwrap(stored(ONE), ONE, header=b"\x77\x09")), INVALID)
case("zlib CINFO 8", gpng(zwrap(stored(ONE), ONE, header=b"\x88\x1c")), INVALID)
case("zlib FCHECK", gpng(zwrap(stored(ONE), ONE, header=b"\x78\x02")), INVALID)
case("zlib FDICT", gpng(zwrap(b"\x00\x00\x00\x00" + stored(ONE), ONE, header=b"\x78\x20")), INVALID)
case("zlib CINFO 0 window is accepted", gpng(zwrap(stored(ONE), ONE, header=b"\x08\x1d")), OK, GRAY, 5, 1, [7] * 5)
case("bad adler", gpng(zwrap(stored(ONE), ONE, adler=1)), INVALID)
case("block type 3", gpng(zwrap(b"\x07", ONE)), INVALID)
case("stored LEN vs NLEN", gpng(zwrap(b"\x01" + struct.pack("<HH", 6, 6) + ONE, ONE)), INVALID)
case("stored, empty stored block first", gpng(zwrap(stored(b"", 0) + stored(ONE), ONE)), OK, GRAY, 5, 1, [7] * 5)
# fixed: literal 0 (filter), literal 7, then <length 4, distance 1> = 7 7 7 7, end of block
bw = BW()
bw.put(1, 1); bw.put(1, 2)
bw.fixed_lit(0); bw.fixed_lit(7); bw.fixed_lit(258); bw.code(0, 5); bw.fixed_lit(256)
case("fixed block with an overlapping match", gpng(zwrap(bw.bytes(), ONE)), OK, GRAY, 5, 1, [7] * 5)
for sym, nm in ((286, "literal symbol 286"), (287, "literal symbol 287")):
    bw = BW()
    bw.put(1, 1); bw.put(1, 2)
    bw.fixed_lit(0); bw.fixed_lit(7); bw.fixed_lit(sym)
    case("fixed " + nm, gpng(zwrap(bw.bytes() + b"\x00\x00", ONE)), INVALID)
for dc in (30, 31):
    bw = BW()
    bw.put(1, 1); bw.put(1, 2)
    bw.fixed_lit(0); bw.fixed_lit(7); bw.fixed_lit(258); bw.code(dc, 5); bw.fixed_lit(256)
    case("fixed distance code %d" % dc, gpng(zwrap(bw.bytes(), ONE)), INVALID)
bw = BW()
bw.put(1, 1); bw.put(1, 2)
bw.fixed_lit(0); bw.fixed_lit(258); bw.code(1, 5); bw.fixed_lit(256)       # distance 2 with 1 byte produced
case("distance beyond the bytes produced", gpng(zwrap(bw.bytes(), ONE)), INVALID)
bw = BW()
bw.put(1, 1); bw.put(1, 2)
bw.fixed_lit(0); bw.fixed_lit(7); bw.fixed_lit(259); bw.code(0, 5); bw.fixed_lit(256)   # 1 + 1 + 5 = 7 bytes for 6
case("too much pixel data", gpng(zwrap(bw.bytes(), ONE + b"\x07")), INVALID)
case("not enough pixel data", gpng(zstored(ONE[:-1])), INVALID)
case("stream ends early", gpng(zstored(ONE)[:-6]), INVALID)
case("bytes after the Adler-32", gpng(zstored(ONE) + b"\x00"), UNSUPPORTED)
case("an empty IDAT after the stream", gpng(zstored(ONE), post=chunk(b"IDAT", b"")), UNSUPPORTED)
case("IDAT split at every byte", gpng(zstored(ONE), idat_split=1), OK, GRAY, 5, 1, [7] * 5)


def dynamic(lit_lens, dist_lens, clen_lens, syms, hclen=19, final=1, raw_lens=None):
    """a dynamic block: the three code-length lists, then the symbols (literal/length symbol, or (length symbol, extra, dist, extra))"""
    bw = BW()
    bw.put(final, 1); bw.put(2, 2)
    bw.put(len(lit_lens) - 257, 5); bw.put(len(dist_lens) - 1, 5); bw.put(hclen - 4, 4)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    for k in range(hclen):
        bw.put(clen_lens[order[k]], 3)
    cc = codes(clen_lens)
    for item in (raw_lens if raw_lens is not None else [(n,) for n in lit_lens + dist_lens]):
        bw.code(*cc[item[0]])
        if len(item) > 1:
            bw.put(item[1], item[2])
    lc, dcd = codes(lit_lens), codes(dist_lens)
    for s in syms:
        if isinstance(s, tuple):
            ls, le, ds, de = s
            bw.code(*lc[ls])
            bw.put(*le)
            bw.code(*dcd[ds])
            bw.put(*de)
        else:
            bw.code(*lc[s])
    return bw.bytes()


# literal/length code: symbols 0, 7, 256, 258 of length 2 (complete); code-length code: lengths 0 and 2 of length 1 (complete)
LIT = [0] * 258
LIT[0] = LIT[7] = LIT[256] = LIT[257] = 2
LIT = LIT + [0]                                         # HLIT 259: symbol 258 present with length 0 here
LIT[257] = 0
LIT[258] = 2
CL = [0] * 19
CL[0], CL[1], CL[2] = 1, 2, 2
DIST1 = [1]                                             # one distance code of length 1: Go's single-code exception
st = dynamic(LIT, DIST1, CL, [0, 7, (258, (0, 0), 0, (0, 0)), 256])
case("dynamic, single distance code of length 1", gpng(zwrap(st, ONE)), OK, GRAY, 5, 1, [7] * 5)
st = dynamic(LIT, [0], CL, [0, 7, 7, 7, 7, 7, 256])
case("dynamic, empty distance code, literals only", gpng(zwrap(st, ONE)), OK, GRAY, 5, 1, [7] * 5)
bw_lit = [0] * 259
bw_lit[0] = bw_lit[7] = bw_lit[256] = 2
bw_lit[258] = 3                                          # 2 + 2 + 2 + 3: incomplete (7/8 of the space)
CL3 = [0] * 19
CL3[0] = CL3[2] = CL3[3] = 2
CL3[1] = 2
case("dynamic, incomplete literal code", gpng(zwrap(dynamic(bw_lit, DIST1, CL3, [0]), ONE)), INVALID)
CLover = [0] * 19
CLover[0] = CLover[2] = CLover[1] = 1                   # three codes of length 1: over-subscribed
case("dynamic, over-subscribed code-length code", gpng(zwrap(dynamic(LIT, DIST1, CLover, [], raw_lens=[]), ONE)), INVALID)
CL16 = [0] * 19
CL16[16] = CL16[0] = 1
case("dynamic, repeat 16 first", gpng(zwrap(dynamic(LIT, DIST1, CL16, [], raw_lens=[(16, 0, 2)]), ONE)), INVALID)
CL18 = [0] * 19
CL18[18] = CL18[0] = 1
case("dynamic, repeat past HLIT + HDIST", gpng(zwrap(dynamic(LIT, DIST1, CL18, [], raw_lens=[(18, 127, 7), (18, 127, 7), (18, 127, 7)]),
                                                      ONE)), INVALID)
bw = BW()
bw.put(1, 1); bw.put(2, 2); bw.put(30, 5); bw.put(0, 5); bw.put(15, 4)
case("dynamic, HLIT 287", gpng(zwrap(bw.bytes() + b"\x00" * 16, ONE)), INVALID)
bw = BW()
bw.put(1, 1); bw.put(2, 2); bw.put(0, 5); bw.put(30, 5); bw.put(15, 4)
case("dynamic, HDIST 31", gpng(zwrap(bw.bytes() + b"\x00" * 16, ONE)), INVALID)

# ---- container ------------------------------------------------------------------------------------------------------------------
good = gpng(zstored(ONE))
case("valid reference file", good, OK, GRAY, 5, 1, [7] * 5)
case("bad signature", b"\x89PNG\r\n\x1a\x0b" + good[8:], INVALID)
case("truncated before IEND", good[:-1], INVALID)
case("bytes after IEND are ignored", good + b"garbage", OK, GRAY, 5, 1, [7] * 5)
b = bytearray(good)
b[8 + 8 + 13] ^= 1
case("bad IHDR CRC", bytes(b), INVALID)
b = bytearray(good)
b[-1] ^= 1
case("bad IEND CRC", bytes(b), INVALID)
b = bytearray(good)
b[-13] ^= 1
case("bad IDAT CRC", bytes(b), INVALID)
z = zstored(ONE)
tail = b"".join([chunk(b"IDAT", z), chunk(b"IEND", b"")])
case("IHDR length 12", SIG + chunk(b"IHDR", struct.pack(">IIBBBB", 5, 1, 8, 0, 0, 0)) + tail, INVALID)
case("IHDR width 0", SIG + ihdr(0, 1, 8, 0) + tail, INVALID)
case("IHDR width 2^31", SIG + ihdr(1 << 31, 1, 8, 0) + tail, INVALID)
case("IHDR compression 1", SIG + ihdr(5, 1, 8, 0, comp=1) + tail, INVALID)
case("IHDR filter method 1", SIG + ihdr(5, 1, 8, 0, filt=1) + tail, INVALID)
case("IHDR interlace 2", SIG + ihdr(5, 1, 8, 0, il=2) + tail, INVALID)
case("IHDR gray depth 3", SIG + ihdr(5, 1, 3, 0) + tail, INVALID)
case("IHDR rgb depth 4", SIG + ihdr(5, 1, 4, 2) + tail, INVALID)
case("IHDR colour type 5", SIG + ihdr(5, 1, 8, 5) + tail, INVALID)
case("Adam7", SIG + ihdr(5, 1, 8, 0, il=1) + tail, UNSUPPORTED)
case("IDAT before IHDR", SIG + tail, INVALID)
case("unknown chunk before IHDR", SIG + chunk(b"teXt", b"a") + ihdr(5, 1, 8, 0) + tail, UNSUPPORTED)
case("second IHDR", SIG + ihdr(5, 1, 8, 0) + ihdr(5, 1, 8, 0) + tail, INVALID)
case("unknown ancillary chunks", SIG + ihdr(5, 1, 8, 0) + chunk(b"gAMA", b"\x00\x00\xb1\x8f") + chunk(b"IDAT", z) +
     chunk(b"tEXt", b"k\x00v") + chunk(b"IEND", b""), OK, GRAY, 5, 1, [7] * 5)
case("unknown critical chunk", SIG + ihdr(5, 1, 8, 0) + chunk(b"ABCD", b"") + tail, UNSUPPORTED)
case("IDAT, ancillary, IDAT", SIG + ihdr(5, 1, 8, 0) + chunk(b"IDAT", z[:4]) + chunk(b"tEXt", b"k\x00v") + chunk(b"IDAT", z[4:]) +
     chunk(b"IEND", b""), UNSUPPORTED)
case("IEND before IDAT", SIG + ihdr(5, 1, 8, 0) + chunk(b"IEND", b""), INVALID)
case("IEND length 1", SIG + ihdr(5, 1, 8, 0) + chunk(b"IDAT", z) + chunk(b"IEND", b"\x00"), INVALID)
P3 = bytes(sum(E, ()))
praw = zstored(rows_none([[0, 1]]))
case("palette without PLTE", SIG + ihdr(2, 1, 8, 3) + chunk(b"IDAT", praw) + chunk(b"IEND", b""), INVALID)
case("PLTE length 4", png(2, 1, 8, 3, praw, pre=chunk(b"PLTE", b"\x01\x02\x03\x04")), INVALID)
case("PLTE empty", png(2, 1, 8, 3, praw, pre=chunk(b"PLTE", b"")), INVALID)
case("PLTE 3 entries at depth 1", png(2, 1, 1, 3, zstored(rows_none([[0x40]])), pre=chunk(b"PLTE", P3)), INVALID)
case("PLTE 257 entries", png(2, 1, 8, 3, praw, pre=chunk(b"PLTE", b"\x01" * 771)), INVALID)
case("PLTE on gray", png(5, 1, 8, 0, z, pre=chunk(b"PLTE", P3)), INVALID)
case("PLTE after tRNS", png(2, 1, 8, 3, praw, pre=chunk(b"tRNS", b"\x01") + chunk(b"PLTE", P3)), INVALID)
case("PLTE after IDAT", png(2, 1, 8, 3, praw, pre=chunk(b"PLTE", P3), post=chunk(b"PLTE", P3)), INVALID)
case("tRNS gray length 3", png(5, 1, 8, 0, z, pre=chunk(b"tRNS", b"\x00\x07\x00")), INVALID)
case("tRNS rgb length 2", png(1, 1, 8, 2, zstored(rows_none([[1, 2, 3]])), pre=chunk(b"tRNS", b"\x00\x07")), INVALID)
case("tRNS on RGBA", png(1, 1, 8, 6, zstored(rows_none([[1, 2, 3, 4]])), pre=chunk(b"tRNS", b"\x00\x01\x00\x02\x00\x03")), INVALID)
case("tRNS on gray-alpha", png(1, 1, 8, 4, zstored(rows_none([[1, 2]])), pre=chunk(b"tRNS", b"\x00\x01")), INVALID)
case("tRNS longer than PLTE", png(2, 1, 8, 3, praw, pre=chunk(b"PLTE", P3) + chunk(b"tRNS", b"\x01\x02\x03\x04")), UNSUPPORTED)
case("tRNS 257 bytes", png(2, 1, 8, 3, praw, pre=chunk(b"PLTE", b"\x01" * 768) + chunk(b"tRNS", b"\x01" * 257)), INVALID)
case("second tRNS", png(5, 1, 8, 0, z, pre=chunk(b"tRNS", b"\x00\x07") + chunk(b"tRNS", b"\x00\x07")), INVALID)
case("tRNS after IDAT", png(5, 1, 8, 0, z, post=chunk(b"tRNS", b"\x00\x07")), INVALID)
case("tRNS on rgb after PLTE", png(1, 1, 8, 2, zstored(rows_none([[1, 2, 3]])), pre=chunk(b"PLTE", P3) +
                                   chunk(b"tRNS", b"\x00\x01\x00\x02\x00\x03")), UNSUPPORTED)
case("tRNS on sub-byte gray", png(3, 2, 1, 0, zstored(rows_none([[0xA0], [0x40]])), pre=chunk(b"tRNS", b"\x00\x01")), UNSUPPORTED)
case("tRNS gray sample 256 at depth 8", png(5, 1, 8, 0, z, pre=chunk(b"tRNS", b"\x01\x07")), UNSUPPORTED)
case("tRNS rgb sample 256 at depth 8", png(1, 1, 8, 2, zstored(rows_none([[1, 2, 3]])), pre=chunk(b"tRNS", b"\x00\x01\x01\x02\x00\x03")),
     UNSUPPORTED)

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "png_dec_kats.json"), "w") as f:
    json.dump(CASES, f, separators=(",", ":"))
print("%d cases" % len(CASES))
