"""Writes png_adam7_kats.json: hand-derived Adam7-interlaced PNG files and what png.Decode (as restated in DESIGN.md section 4.10)
answers for each with IPX_PNG_ADAM7=1 ("status") and without it ("status_off"), for tests/test_png_adam7_model.py and
tests/test_png_adam7_gpu.py.  Written without the model: the bytes of every pass and the pixels of every frame are spelled out here,
the zlib streams are stored blocks, and only the library's zlib.crc32 / zlib.adler32 are used, for the checksums.

  python tests/golden/make_png_adam7_kats.py      # rewrites tests/golden/png_adam7_kats.json

The passes, as (xFactor, yFactor, xOffset, yOffset): 1 (8,8,0,0)  2 (8,8,4,0)  3 (4,8,0,4)  4 (4,4,2,0)  5 (2,4,0,2)  6 (2,2,1,0)
7 (1,2,0,1).  A pass with no column or no row in the frame has no bytes at all."""
import json
import os
import struct
import zlib

OK, INVALID, UNSUPPORTED = 0, -1, -4
GRAY, NRGBA, RGBA, PALETTED, GRAY16, RGBA64, NRGBA64 = range(7)
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))


def zstored(data):
    return b"\x78\x01" + b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data + struct.pack(">I", zlib.adler32(data))


def png(w, h, depth, ctype, stream, pre=b"", post=b""):
    return SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1)) + pre + chunk(b"IDAT", stream) + post + chunk(b"IEND", b"")


def rows(*rr):
    """the rows of one pass: (filter type, bytes ...) each"""
    return b"".join(bytes(r) for r in rr)


def b(s):
    """a byte from its bits, most significant first; spaces and underscores are for the eye"""
    s = s.replace(" ", "").replace("_", "")
    assert len(s) == 8
    return int(s, 2)


CASES = []


def case(name, data, status, kind=None, w=None, h=None, pix=None, palette=None):
    c = {"name": name, "data": data.hex(), "status": status, "status_off": UNSUPPORTED}     # the IHDR decides with the switch off
    if status == OK:
        c.update(kind=kind, w=w, h=h, pix=bytes(pix).hex())
        if palette is not None:
            c["palette"] = bytes(palette).hex()
    CASES.append(c)


def pal_bytes(entries, alphas=()):
    out = bytearray()
    for k in range(256):
        if k < len(entries):
            out += bytes(entries[k]) + bytes([alphas[k] if k < len(alphas) else 255])
        else:
            out += b"\x00\x00\x00\xff"
    return out


# ---- 8 x 8 gray 8, pixel (x, y) = 8y + x, filter None everywhere: the order of the stream ------------------------------------------
P1 = rows([0, 0])
P2 = rows([0, 4])
P3 = rows([0, 32, 36])
P4 = rows([0, 2, 6], [0, 34, 38])
P5 = rows([0, 16, 18, 20, 22], [0, 48, 50, 52, 54])
P6 = rows([0, 1, 3, 5, 7], [0, 17, 19, 21, 23], [0, 33, 35, 37, 39], [0, 49, 51, 53, 55])
P7 = rows([0, 8, 9, 10, 11, 12, 13, 14, 15], [0, 24, 25, 26, 27, 28, 29, 30, 31], [0, 40, 41, 42, 43, 44, 45, 46, 47],
          [0, 56, 57, 58, 59, 60, 61, 62, 63])
RAW8 = P1 + P2 + P3 + P4 + P5 + P6 + P7
assert len(RAW8) == 2 + 2 + 3 + 6 + 10 + 20 + 36
case("8x8 gray8 pass order", png(8, 8, 8, 0, zstored(RAW8)), OK, GRAY, 8, 8, list(range(64)))

# ---- small frames: empty passes have no filter byte ----------------------------------------------------------------------------
# 1 x 1: pass 1 only, 2 bytes
case("1x1 gray8", png(1, 1, 8, 0, zstored(rows([0, 77]))), OK, GRAY, 1, 1, [77])
# 3 x 2, pixels 1 2 3 / 4 5 6: pass 1 (0,0); 2 none (x 4); 3 none (y 4); 4 (2,0); 5 none (y 2); 6 (1,0); 7 row 1
case("3x2 gray8 skips passes 2 3 5", png(3, 2, 8, 0, zstored(rows([0, 1]) + rows([0, 3]) + rows([0, 2]) + rows([0, 4, 5, 6]))), OK, GRAY,
     3, 2, [1, 2, 3, 4, 5, 6])
# 2 x 5, pixel (x, y) = 10y + x: pass 1 (0,0); 2 none; 3 (0,4); 4 none (x 2); 5 (0,2); 6 x 1 of rows 0 2 4; 7 rows 1 3
case("2x5 gray8 skips passes 2 4", png(2, 5, 8, 0, zstored(rows([0, 0]) + rows([0, 40]) + rows([0, 20]) + rows([0, 1], [0, 21], [0, 41]) +
                                                            rows([0, 10, 11], [0, 30, 31]))), OK, GRAY, 2, 5,
     [0, 1, 10, 11, 20, 21, 30, 31, 40, 41])
# the same 3 x 2 stream with the filter byte of an empty pass 2 slipped in: one byte too many
case("3x2 with a filter byte for the empty pass 2", png(3, 2, 8, 0, zstored(rows([0, 1]) + b"\x00" + rows([0, 3]) + rows([0, 2]) +
                                                                             rows([0, 4, 5, 6]))), INVALID)

# ---- 5 x 5 at sub-byte depths: rows packed by the pass's width, spare bits ignored ---------------------------------------------------
# gray 1, frame bits          pass 1 (0,0)  2 (4,0)  3 (0,4) (4,4)  4 (2,0) / (2,4)  5 (0,2) (2,2) (4,2)
#   1 0 1 1 0                 6 (1,y) (3,y) of rows 0 2 4           7 rows 1 3
#   0 1 1 0 1
#   1 1 0 0 1
#   0 0 1 1 1
#   1 0 0 1 0
raw = (rows([0, b("1 1111111")]) + rows([0, b("0 1111111")]) + rows([0, b("10 111111")]) + rows([0, b("1 0000000")], [0, b("0 1010101")]) +
       rows([0, b("101 11111")]) + rows([0, b("01 000000")], [0, b("10 111111")], [0, b("01 111111")]) +
       rows([0, b("01101 111")], [0, b("00111 000")]))
F = 255
case("5x5 gray1 packed by pass width", png(5, 5, 1, 0, zstored(raw)), OK, GRAY, 5, 5,
     [F, 0, F, F, 0, 0, F, F, 0, F, F, F, 0, 0, F, 0, 0, F, F, F, F, 0, 0, F, 0])
# palette 2, index (x, y) = (x + 3y) mod 4; 3 PLTE entries, so index 3 shows the opaque black behind them
#   0 1 2 3 0
#   3 0 1 2 3
#   2 3 0 1 2
#   1 2 3 0 1
#   0 1 2 3 0
E = [(200, 0, 0), (0, 200, 0), (0, 0, 200)]
raw = (rows([0, b("00 111111")]) + rows([0, b("00 010101")]) + rows([0, b("00 00 1111")]) + rows([0, b("10 000000")], [0, b("10 111111")]) +
       rows([0, b("10 00 10 11")]) + rows([0, b("01 11 0000")], [0, b("11 01 1111")], [0, b("01 11 1010")]) +
       rows([0, b("11 00 01 10"), b("11 000000")], [0, b("01 10 11 00"), b("01 111111")]))
case("5x5 pal2 packed by pass width", png(5, 5, 2, 3, zstored(raw), pre=chunk(b"PLTE", bytes(sum(E, ())))), OK, PALETTED, 5, 5,
     [0, 1, 2, 3, 0, 3, 0, 1, 2, 3, 2, 3, 0, 1, 2, 1, 2, 3, 0, 1, 0, 1, 2, 3, 0], pal_bytes(E))

# ---- the row above a pass's first row is zero, not the pass before's last row -----------------------------------------------------
# 8 x 8 gray 8, every row of passes 2 .. 7 filtered Up (type 2).  Pass 1 [10]; 2 [5] -> 5 (15 if pass 1's row were above); 3 [7 8] ->
# 7 8; 4 [1 2] -> 1 2, [1 1] -> 2 3; 5 [3 3 3 3] -> 3s, [1 1 1 1] -> 4s; 6 [9 9 9 9] -> 9s, then [1 1 1 1] three times -> 10s 11s 12s;
# 7 [20 x 8] -> 20s, then [1 x 8] three times -> 21s 22s 23s
raw = (rows([0, 10]) + rows([2, 5]) + rows([2, 7, 8]) + rows([2, 1, 2], [2, 1, 1]) + rows([2, 3, 3, 3, 3], [2, 1, 1, 1, 1]) +
       rows([2, 9, 9, 9, 9], [2, 1, 1, 1, 1], [2, 1, 1, 1, 1], [2, 1, 1, 1, 1]) +
       rows([2] + [20] * 8, [2] + [1] * 8, [2] + [1] * 8, [2] + [1] * 8))
case("8x8 passes open with an Up row", png(8, 8, 8, 0, zstored(raw)), OK, GRAY, 8, 8,
     [10, 9, 1, 9, 5, 9, 2, 9] + [20] * 8 + [3, 10, 3, 10, 3, 10, 3, 10] + [21] * 8 + [7, 11, 2, 11, 8, 11, 3, 11] + [22] * 8 +
     [4, 12, 4, 12, 4, 12, 4, 12] + [23] * 8)
# the first row of passes 2 .. 7 filtered Paeth (type 4), their other rows None: over a zero row Paeth adds the pixel to the left
# (a, 0, 0 -> a), over the pass before's last row it would add that row's pixel.  Pass 1 [10]; 2 [5] -> 5; 3 [7 1] -> 7 8;
# 4 [1 1] -> 1 2, then 50 60; 5 [3 1 1 1] -> 3 4 5 6, then 70 .. 73; 6 [9 1 1 1] -> 9 10 11 12, then 80 .. 83, 84 .. 87, 88 .. 91;
# 7 [20 1 1 1 1 1 1 1] -> 20 .. 27, then 100 .. 107, 110 .. 117, 120 .. 127
raw = (rows([0, 10]) + rows([4, 5]) + rows([4, 7, 1]) + rows([4, 1, 1], [0, 50, 60]) + rows([4, 3, 1, 1, 1], [0, 70, 71, 72, 73]) +
       rows([4, 9, 1, 1, 1], [0, 80, 81, 82, 83], [0, 84, 85, 86, 87], [0, 88, 89, 90, 91]) +
       rows([4, 20, 1, 1, 1, 1, 1, 1, 1], [0] + list(range(100, 108)), [0] + list(range(110, 118)), [0] + list(range(120, 128))))
case("8x8 passes open with a Paeth row", png(8, 8, 8, 0, zstored(raw)), OK, GRAY, 8, 8,
     [10, 9, 1, 10, 5, 11, 2, 12] + list(range(20, 28)) + [3, 80, 4, 81, 5, 82, 6, 83] + list(range(100, 108)) +
     [7, 84, 50, 85, 8, 86, 60, 87] + list(range(110, 118)) + [70, 88, 71, 89, 72, 90, 73, 91] + list(range(120, 128)))
# RGBA 8, 2 x 2 (bpp 4): pass 1 (0,0) None; 6 (1,0) Sub over nothing to the left -> itself; 7 row 1: Average [10 10 10 10, 1 1 1 1]
# over a zero row -> 10s, then 1 + (10 + 0) / 2 = 6s
raw = rows([0, 1, 2, 3, 4]) + rows([1, 5, 6, 7, 8]) + rows([3, 10, 10, 10, 10, 1, 1, 1, 1])
case("2x2 rgba8", png(2, 2, 8, 6, zstored(raw)), OK, NRGBA, 2, 2, [1, 2, 3, 4, 5, 6, 7, 8, 10, 10, 10, 10, 6, 6, 6, 6])

# ---- the raw length and the filter types ----------------------------------------------------------------------------------------------
case("8x8 one byte short", png(8, 8, 8, 0, zstored(RAW8[:-1])), INVALID)
case("8x8 one byte long", png(8, 8, 8, 0, zstored(RAW8 + b"\x00")), INVALID)
case("filter type 5 in the first row of pass 3", png(8, 8, 8, 0, zstored(P1 + P2 + rows([5, 32, 36]) + P4 + P5 + P6 + P7)), INVALID)
case("filter type 5 in the last row of pass 7", png(8, 8, 8, 0, zstored(P1 + P2 + P3 + P4 + P5 + P6 + P7[:27] + b"\x05" + P7[28:])), INVALID)
case("a byte after the Adler-32", png(8, 8, 8, 0, zstored(RAW8) + b"\x00"), UNSUPPORTED)
case("an empty IDAT after the stream", png(8, 8, 8, 0, zstored(RAW8), post=chunk(b"IDAT", b"")), UNSUPPORTED)

# ---- the container rules hold for interlaced files too (with the switch off, the IHDR has answered before them) --------------------------
case("palette without PLTE", png(1, 1, 8, 3, zstored(rows([0, 0]))), INVALID)
case("tRNS on sub-byte gray", png(1, 1, 1, 0, zstored(rows([0, 0])), pre=chunk(b"tRNS", b"\x00\x01")), UNSUPPORTED)
case("tRNS on RGBA", png(1, 1, 8, 6, zstored(rows([0, 1, 2, 3, 4])), pre=chunk(b"tRNS", b"\x00\x01\x00\x02\x00\x03")), INVALID)
bad = bytearray(png(1, 1, 8, 0, zstored(rows([0, 77]))))
bad[8 + 8 + 13] ^= 1
case("bad IHDR CRC", bytes(bad), INVALID)

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "png_adam7_kats.json"), "w") as f:
    json.dump(CASES, f, separators=(",", ":"))
print("%d cases" % len(CASES))
