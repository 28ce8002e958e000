"""Writes tests/golden/gif_dec_kats.json: known answers of gif.Decode (image/gif's reader with compress/lzw's, the first image) derived
WITHOUT tests/gif_decode_model.py.

Every case is a small stream assembled here: code sequences with their widths written out by hand (comments below), packed LSB-first,
framed in sub-blocks and wrapped in a container.  Each case carries its expected outcome -- "ok" (gif.Decode returns an image) and, when
ok, the first image's rectangle, its indices in row order and its palette (len(m.Palette) and the entries as (R, G, B, A)).  The width
rule the literal-only streams use: a code is read at the width bit_length(hi), hi being eof + (codes read since the last clear) and
capped at 4095 (width 12), since hi grows by one per code and the width grows when hi reaches 1 << width.

python tests/golden/make_gif_dec_kats.py   (rewrites the file; no seed involved)"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def pack(codes_widths):
    bits = nbits = 0
    out = bytearray()
    for c, w in codes_widths:
        assert 0 <= c < 1 << w
        bits |= c << nbits
        nbits += w
        while nbits >= 8:
            out.append(bits & 0xFF)
            bits >>= 8
            nbits -= 8
    if nbits:
        out.append(bits & 0xFF)
    return bytes(out)


def colour(i):
    return ((i * 7) & 255, (i * 13 + 1) & 255, (i * 29 + 2) & 255)


def table(n):
    return b"".join(bytes(colour(i)) for i in range(n))


def u16(v):
    return bytes((v & 255, v >> 8))


def blocks(data, sizes=None):
    """sub-blocks of the given sizes (default: 255 at a time), then the block terminator"""
    out, p = bytearray(), 0
    sizes = list(sizes) if sizes is not None else []
    while p < len(data) or sizes:
        n = sizes.pop(0) if sizes else min(255, len(data) - p)
        out.append(n)
        out += data[p:p + n]
        p += n
    return bytes(out) + b"\x00"


def gif(lzw, lit, w, h, sw=None, sh=None, gtab=4, ltab=None, pre=b"", left=0, top=0, interlace=False, version=b"GIF89a",
        framing=None, tail=b"\x3b"):
    """a file: header, logical screen (sw x sh, default w x h), a global table of `gtab` entries (0 / None: none), the blocks `pre`,
    the image descriptor, a local table of `ltab` entries, the LZW minimum code size, the data (framing: the whole image-data part
    as given, else blocks(lzw)), then `tail`"""
    sw = w if sw is None else sw
    sh = h if sh is None else sh
    out = bytearray(version + u16(sw) + u16(sh))
    if gtab:
        out += bytes((0x80 | (gtab.bit_length() - 2), 0, 0)) + table(gtab)
    else:
        out += b"\x00\x00\x00"
    out += pre
    flags = (0x40 if interlace else 0) | ((0x80 | (ltab.bit_length() - 2)) if ltab else 0)
    out += b"\x2c" + u16(left) + u16(top) + u16(w) + u16(h) + bytes((flags,))
    if ltab:
        out += b"".join(bytes(colour(100 + i)) for i in range(ltab))
    out += bytes((lit,)) + (framing if framing is not None else blocks(lzw))
    return bytes(out + tail)


def pal(n, trans=None, base=0):
    p = [list(colour(base + i)) + [255] for i in range(n)]
    if trans is not None:
        p += [[0, 0, 0, 0]] * max(0, trans + 1 - n)
        p[trans] = [0, 0, 0, 0]
    return p


def gce(trans=None, size=4, term=0):
    return bytes((0x21, 0xF9, size, 1 if trans is not None else 0, 0, 0, trans or 0, term))


def literal_widths(lits, lit):
    """clear, then the literal codes at the bit_length(hi) widths, then EOF (see the module docstring)"""
    clear, eof = 1 << lit, (1 << lit) + 1
    out = [(clear, lit + 1)]
    hi = eof
    for v in lits:
        out.append((v, min(12, hi.bit_length())))
        hi = min(hi + 1, 4095)
    out.append((eof, min(12, hi.bit_length())))
    return out


CASES = []


def case(name, data, ok, rect=None, index=None, palette=None):
    CASES.append({"name": name, "data": data.hex(), "ok": ok, "rect": rect, "index": index, "palette": palette})


# ---- lit 2: clear 4, eof 5; width 3 until hi reaches 8 -----------------------------------------------------------------------
# 4@3 clear; 0@3 -> [0] (hi 6); 1@3 -> [1], entry 6 = [0,1] (hi 7); 7@3 = hi: KwKwK -> [1,1], entry 7 = [1,1] (hi 8: width 4);
# 5@4 eof.  2 x 2 frame [[0,1],[1,1]].
BASIC = pack([(4, 3), (0, 3), (1, 3), (7, 3), (5, 4)])       # 16 bits: 2 bytes, ends on a byte
case("lit2 kwkwk", gif(BASIC, 2, 2, 2), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(4))
case("GIF87a", gif(BASIC, 2, 2, 2, version=b"GIF87a"), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(4))
case("bad version", gif(BASIC, 2, 2, 2, version=b"GIF88a"), False)
case("truncated header", gif(BASIC, 2, 2, 2)[:10], False)
case("truncated global table", gif(BASIC, 2, 2, 2)[:13 + 5], False)
case("no table at all", gif(BASIC, 2, 2, 2, gtab=None), False)
case("local table replaces global", gif(BASIC, 2, 2, 2, gtab=4, ltab=8), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(8, base=100))
case("local table only", gif(BASIC, 2, 2, 2, gtab=None, ltab=4), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(4, base=100))
case("truncated local table", gif(BASIC, 2, 2, 2, gtab=None, ltab=4)[:13 + 10 + 6], False)
case("second frame after the first", gif(BASIC, 2, 2, 2, tail=b"\x2c" + b"\x00" * 8 + b"\x00\x09garbage"), True, [0, 0, 2, 2],
     [0, 1, 1, 1], pal(4))
case("no trailer", gif(BASIC, 2, 2, 2, tail=b""), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(4))
case("frame at an origin", gif(BASIC, 2, 2, 2, sw=5, sh=4, left=3, top=2), True, [3, 2, 2, 2], [0, 1, 1, 1], pal(4))
case("frame bounds larger than image bounds", gif(BASIC, 2, 2, 2, sw=3, sh=4, left=2, top=0), False)
case("frame taller than the screen", gif(BASIC, 2, 2, 2, sw=2, sh=1), False)
case("lzw width 1", gif(BASIC, 1, 2, 2), False)
case("lzw width 9", gif(BASIC, 9, 2, 2), False)
case("missing lzw width", gif(BASIC, 2, 2, 2)[:13 + 12 + 10], False)

# ---- blocks before the image ------------------------------------------------------------------------------------------------
COMMENT = b"\x21\xfe\x05hello\x03abc\x00"
APP = b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"
TEXT = b"\x21\x01" + bytes((12,)) + bytes(12) + b"\x02hi\x00"
case("extensions before the image", gif(BASIC, 2, 2, 2, pre=COMMENT + APP + TEXT + gce()), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(4))
case("application block of 10 bytes", gif(BASIC, 2, 2, 2, pre=b"\x21\xff\x0aADOBE2.0ab\x00"), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(4))
case("unknown extension label", gif(BASIC, 2, 2, 2, pre=b"\x21\x02\x01x\x00"), False)
case("graphic control of size 5", gif(BASIC, 2, 2, 2, pre=gce(size=5)), False)
case("graphic control without terminator", gif(BASIC, 2, 2, 2, pre=gce(term=7)), False)
case("truncated comment", gif(BASIC, 2, 2, 2, pre=b"\x21\xfe\x05hel")[:13 + 12 + 6], False)
case("trailer before the image", gif(BASIC, 2, 2, 2, pre=b"\x3b"), False)
case("unknown block", gif(BASIC, 2, 2, 2, pre=b"\x00"), False)

# ---- transparency ------------------------------------------------------------------------------------------------------------
case("transparent index in the table", gif(BASIC, 2, 2, 2, pre=gce(1)), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(4, trans=1))
case("transparent flag cleared later keeps the index", gif(BASIC, 2, 2, 2, pre=gce(1) + gce()), True, [0, 0, 2, 2], [0, 1, 1, 1],
     pal(4, trans=1))
case("transparent index in a local table", gif(BASIC, 2, 2, 2, ltab=4, pre=gce(0)), True, [0, 0, 2, 2], [0, 1, 1, 1],
     pal(4, trans=0, base=100))
# lit 4 over a 4-entry table: literals 0..15 are codes, the palette check decides.  clear 16, eof 17; three literals at width 5.
L4 = lambda lits: pack(literal_widths(lits, 4))
case("transparent index past the table lengthens it", gif(L4([9, 0, 3]), 4, 3, 1, pre=gce(9)), True, [0, 0, 3, 1], [9, 0, 3],
     pal(4, trans=9))
case("index past the lengthened palette", gif(L4([9, 10, 3]), 4, 3, 1, pre=gce(9)), False)
case("index past the table", gif(L4([1, 5, 3]), 4, 3, 1), False)
case("256 entries: no pixel check", gif(L4([1, 5, 3]), 4, 3, 1, gtab=256), True, [0, 0, 3, 1], [1, 5, 3], pal(256))

# ---- lit 2 .. 8: clear, three literals, eof --------------------------------------------------------------------------------
for lit in range(2, 9):
    lits = [(1 << lit) - 1, 0, 1 % (1 << lit)] if lit > 2 else [3, 0, 1]
    case("lit %d literals" % lit, gif(pack(literal_widths(lits, lit)), lit, 3, 1, gtab=1 << lit), True, [0, 0, 3, 1], lits,
         pal(1 << lit))

# ---- clear codes ----------------------------------------------------------------------------------------------------------
# 4@3; 0@3 (hi 6); 1@3 -> entry 6 = [0,1] (hi 7); 6@3 -> [0,1], entry 7 = [1,0] (hi 8, width 4); 4@4 clear (width 3, hi 5);
# 2@3 (hi 6); 3@3 -> entry 6 = [2,3] (hi 7); 6@3 -> [2,3], entry 7 = [3,2] (hi 8, width 4); 5@4 eof.  4 x 2: [0,1,0,1],[2,3,2,3].
CLEARS = pack([(4, 3), (0, 3), (1, 3), (6, 3), (4, 4), (2, 3), (3, 3), (6, 3), (5, 4)])
case("clear in mid-stream", gif(CLEARS, 2, 4, 2), True, [0, 0, 4, 2], [0, 1, 0, 1, 2, 3, 2, 3], pal(4))
# after the clear, entry 7 is gone: 4@3; 0@3 (hi 6); 1@3 (hi 7); 4@3 clear; 2@3 (hi 6); 7@3 > hi = invalid
case("code of a cleared entry", gif(pack([(4, 3), (0, 3), (1, 3), (4, 3), (2, 3), (7, 3), (5, 3)]), 2, 2, 2), False)
case("code above hi", gif(pack([(4, 3), (0, 3), (7, 3), (5, 3)]), 2, 2, 1), False)
case("entry code first after clear", gif(pack([(4, 3), (6, 3), (5, 3)]), 2, 2, 1), False)
case("no clear code first", gif(pack([(1, 3), (2, 3), (6, 3), (5, 4)]), 2, 4, 1), True, [0, 0, 4, 1], [1, 2, 1, 2], pal(4))

# ---- amount of data -------------------------------------------------------------------------------------------------------------
# 4@3 1@3: 6 bits, the last 2 bits are too few for a code: the data end without EOF
case("missing EOF", gif(pack([(4, 3), (1, 3)]), 2, 1, 1), True, [0, 0, 1, 1], [1], pal(4))
case("missing EOF, not enough", gif(pack([(4, 3), (1, 3)]), 2, 2, 1), False)
case("not enough image data", gif(pack([(4, 3), (0, 3), (1, 3), (5, 3)]), 2, 3, 1), False)
case("a code after the last pixel", gif(pack([(4, 3), (1, 3), (0, 3), (5, 3)]), 2, 1, 1), False)
case("clear codes after the last pixel", gif(pack([(4, 3), (1, 3), (4, 3), (4, 3), (5, 3)]), 2, 1, 1), True, [0, 0, 1, 1], [1], pal(4))
# 4@3 0@3 1@3 6@3 = [0,1,0,1]: one byte past a 3 x 1 frame
case("last string runs past the frame", gif(pack([(4, 3), (0, 3), (1, 3), (6, 3), (5, 4)]), 2, 3, 1), False)
case("empty frame", gif(pack([(4, 3), (5, 3)]), 2, 0, 0, sw=1, sh=1), True, [0, 0, 0, 0], [], pal(4))
case("empty frame with a pixel", gif(pack([(4, 3), (1, 3), (5, 3)]), 2, 0, 0, sw=1, sh=1), False)

# ---- sub-blocks after the EOF code (BASIC: 2 bytes, the EOF code ends on the second) -------------------------------------------
case("EOF at a sub-block boundary, one 1-byte sub-block", gif(BASIC, 2, 2, 2, framing=b"\x02" + BASIC + b"\x01\xaa\x00"), True,
     [0, 0, 2, 2], [0, 1, 1, 1], pal(4))
case("EOF at a sub-block boundary, a 2-byte sub-block", gif(BASIC, 2, 2, 2, framing=b"\x02" + BASIC + b"\x02\xaa\xbb\x00"), False)
case("EOF at a sub-block boundary, two 1-byte sub-blocks", gif(BASIC, 2, 2, 2, framing=b"\x02" + BASIC + b"\x01\xaa\x01\xbb\x00"),
     False)
case("rest of the sub-block after EOF", gif(BASIC, 2, 2, 2, framing=b"\x04" + BASIC + b"\xaa\xbb\x00"), True, [0, 0, 2, 2],
     [0, 1, 1, 1], pal(4))
case("rest of the sub-block, then a 1-byte sub-block", gif(BASIC, 2, 2, 2, framing=b"\x03" + BASIC + b"\xaa\x01\xbb\x00"), False)
case("data split over sub-blocks", gif(BASIC, 2, 2, 2, framing=b"\x01" + BASIC[:1] + b"\x01" + BASIC[1:] + b"\x00"), True,
     [0, 0, 2, 2], [0, 1, 1, 1], pal(4))
case("split, EOF at the boundary, one 1-byte sub-block",
     gif(BASIC, 2, 2, 2, framing=b"\x01" + BASIC[:1] + b"\x01" + BASIC[1:] + b"\x01\x00\x00"), True, [0, 0, 2, 2], [0, 1, 1, 1], pal(4))
case("no block terminator", gif(BASIC, 2, 2, 2, framing=b"\x02" + BASIC, tail=b""), False)
case("sub-block cut short", gif(BASIC, 2, 2, 2, framing=b"\x05" + BASIC, tail=b""), False)
case("terminator only", gif(b"", 2, 1, 1, framing=b"\x00"), False)

# ---- interlace: 2 x h, stream row r holds the pixels (r, r); where it lands, by hand for h = 1 .. 9 --------------------------------
ORDER = {1: [0], 2: [0, 1], 3: [0, 2, 1], 4: [0, 2, 1, 3], 5: [0, 4, 2, 1, 3], 6: [0, 4, 2, 1, 3, 5], 7: [0, 4, 2, 6, 1, 3, 5],
         8: [0, 4, 2, 6, 1, 3, 5, 7], 9: [0, 8, 4, 2, 6, 1, 3, 5, 7]}
for h, order in ORDER.items():
    lits = [r for r in range(h) for _ in range(2)]
    rows = [None] * h
    for r, y in enumerate(order):
        rows[y] = [r, r]
    case("interlaced h=%d" % h, gif(pack(literal_widths(lits, 4)), 4, 2, h, gtab=16, interlace=True), True, [0, 0, 2, h],
         [v for row in rows for v in row], pal(16))

# ---- a full dictionary without a clear (lit 2: clear 4, eof 5) -------------------------------------------------------------------
# 4091 literals after the clear: literal i is read with hi = 5 + i (width bit_length(hi)); the one read at hi = 4095 (i = 4090)
# defines entry 4095 and hi stays there (width 12).  lits: 0 ... 0, then 1, 2, 3 at i = 4088, 4089, 4090, so entry 4094 = [1, 2]
# (defined at i = 4089) and entry 4095 = [2, 3].  Then, at width 12 with no previous code: 4095 -> [2,3] (the entry, not KwKwK),
# 4094 -> [1,2], 1 -> [1] (no entry is added), 4095 -> [2,3] again, clear (at 12), 2@3, eof@3.
lits = [0] * 4088 + [1, 2, 3]
codes = literal_widths(lits, 2)[:-1] + [(4095, 12), (4094, 12), (1, 12), (4095, 12), (4, 12), (2, 3), (5, 3)]
out = lits + [2, 3, 1, 2, 1, 2, 3, 2]
case("full dictionary, then 4095", gif(pack(codes), 2, len(out), 1), True, [0, 0, len(out), 1], out, pal(4))
# the same with 4095 twice, then EOF at width 12
codes = literal_widths(lits, 2)[:-1] + [(4095, 12), (4095, 12), (5, 12)]
out = lits + [2, 3, 2, 3]
case("full dictionary, 4095 twice", gif(pack(codes), 2, len(out), 1), True, [0, 0, len(out), 1], out, pal(4))

if __name__ == "__main__":
    with open(os.path.join(HERE, "gif_dec_kats.json"), "w") as f:
        json.dump(CASES, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases" % len(CASES))
