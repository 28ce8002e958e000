"""Writes jpeg_411_kats.json: 4:1:1 and 4:1:0 JPEGs of DC-only blocks and the planes Go's image/jpeg gives for them, derived by hand
for tests/test_jpeg_411_model.py -- not with tests/jpeg_411_model.py or tests/jpeg_decode_model.py.

Every quantiser entry is 8 and a block's only coefficient is DC = s - 128.  idct.go on such a block: the first row takes the row
shortcut and becomes 8 * D with D = 8 * (s - 128), the other rows are zero; the column pass leaves y0 = (8 * D << 8) + 8192 in every
column and every pixel is (y0 >> 14) + 128 = ((64 * (s - 128) * 256 + 8192) >> 14) + 128 = s.  So a block's 64 samples are all s, and a
plane is its grid of block values, each spread over 8 x 8 pixels (spread() below) -- the layout is what these cases pin:

  4:1:1   MCU 32 x 8: Y blocks 0..3 left to right, then Cb, Cr.  Y plane 8 * myy rows of 32 * mxx; Cb / Cr 8 * myy rows of 8 * mxx
  4:1:0   MCU 32 x 16: Y blocks 0..3 the upper row, 4..7 the lower row, then Cb, Cr.  Y plane 16 * myy rows of 32 * mxx
  `scan_order` lists the block values in the order the interleaved scan codes them, written out by hand below per case, and the
  generator checks that the file it stores codes exactly that sequence of DC differences per component
  `at` holds [x, y, Y, Cb, Cr] triples of YCbCrAt(x, y): Y[y * YStride + x], C[(y or y / 2) * CStride + x / 4]

The streams come from tests/jpeg_writer.py (one DC table, one AC table that holds EOB only).

  python tests/golden/make_jpeg_411_kats.py      # rewrites tests/golden/jpeg_411_kats.json"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_writer as jw  # noqa: E402


def spread(grid):
    """a grid of block values -> the plane: every value over 8 x 8 pixels"""
    return [[v for v in row for _ in range(8)] for row in grid for _ in range(8)]


def stream(w, h, v0, y, cb, cr):
    comps = [(1, 4, v0, 0), (2, 1, 1, 0), (3, 1, 1, 0)]
    fr = jw.Frame(w, h, comps)
    blocks = []
    for g in (y, cb, cr):
        b = np.zeros((len(g), len(g[0]), 64), np.int64)
        b[..., 0] = np.asarray(g, np.int64) - 128
        blocks.append(b)
    dct = jw.huff(jw.spread(9, 2, 9), range(9))
    act = jw.huff([1] + [0] * 15, [0x00])
    sel = [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    return (jw.soi() + jw.app0_jfif() + jw.dqt([(0, [8] * 64, 0)]) + jw.sof(w, h, comps) + jw.dht([(0, 0, dct), (1, 0, act)]) +
            jw.sos(comps, sel) + jw.scan(fr, sel, blocks, ({0: dct}, {0: act})) + jw.eoi())


def dc_sequence(data):
    """the scan's bits (unstuffed) and the DC table's codes as bit strings, for a reader of this file's own (check_scan_order): the DC
    table holds the sizes 0..8, the AC table the single one-bit code 0 for EOB"""
    sos = data.index(b"\xff\xda")
    p = sos + 2 + (data[sos + 2] << 8 | data[sos + 3])
    raw = data[p:-2].replace(b"\xff\x00", b"\xff")
    bits = "".join("{:08b}".format(c) for c in raw)
    dct = jw.huff(jw.spread(9, 2, 9), range(9))
    codes = {"{:0{}b}".format(c, ln): s for s, (c, ln) in dct.code.items()}
    return bits, codes


def check_scan_order(case):
    """decodes the stored file's DC differences and compares with the hand-written scan order"""
    data = bytes.fromhex(case["file"])
    bits, codes = dc_sequence(data)
    pos = 0
    pred = [0, 0, 0]
    nluma = 4 * case["v0"]
    seq = []
    for k, _ in enumerate(case["scan_order"]):
        comp = 0 if k % (nluma + 2) < nluma else k % (nluma + 2) - nluma + 1
        code = ""
        while code not in codes:
            code += bits[pos]
            pos += 1
        s = codes[code]
        v = int(bits[pos:pos + s], 2) if s else 0
        pos += s
        if s and v < 1 << (s - 1):
            v += (-1 << s) + 1
        assert bits[pos] == "0"                      # EOB
        pos += 1
        pred[comp] += v
        seq.append(pred[comp] + 128)
    assert seq == case["scan_order"], (case["name"], seq)
    assert set(bits[pos:]) <= {"1"} and len(bits) - pos < 8


def case(name, w, h, v0, y, cb, cr, scan_order, at):
    mxx, myy = (w + 31) // 32, (h + 8 * v0 - 1) // (8 * v0)
    assert len(y) == v0 * myy and all(len(r) == 4 * mxx for r in y) and len(cb) == myy == len(cr) and all(len(r) == mxx for r in cb + cr)
    c = dict(name=name, w=w, h=h, v0=v0, ratio=5 if v0 == 1 else 6, ystride=32 * mxx, cstride=8 * mxx, yrows=8 * v0 * myy, crows=8 * myy,
             cw=(w + 3) // 4, ch=h if v0 == 1 else (h + 1) // 2,
             y_blocks=y, cb_blocks=cb, cr_blocks=cr, scan_order=scan_order,
             y=spread(y), cb=spread(cb), cr=spread(cr), at=at, file=stream(w, h, v0, y, cb, cr).hex())
    check_scan_order(c)
    return c


def main():
    cases = [
        # one MCU each: the four (eight) Y blocks differ, so their order within the MCU shows
        case("4:1:1 one MCU 32x8", 32, 8, 1, [[10, 20, 30, 40]], [[100]], [[200]], [10, 20, 30, 40, 100, 200],
             [[0, 0, 10, 100, 200], [7, 7, 10, 100, 200], [8, 0, 20, 100, 200], [31, 7, 40, 100, 200]]),
        case("4:1:0 one MCU 32x16", 32, 16, 2, [[10, 20, 30, 40], [50, 60, 70, 80]], [[100]], [[200]], [10, 20, 30, 40, 50, 60, 70, 80, 100, 200],
             [[0, 0, 10, 100, 200], [8, 7, 20, 100, 200], [0, 8, 50, 100, 200], [31, 15, 80, 100, 200]]),
        # 1 x 1: one MCU, of which one pixel is the image
        case("4:1:1 1x1", 1, 1, 1, [[90, 1, 2, 3]], [[60]], [[70]], [90, 1, 2, 3, 60, 70], [[0, 0, 90, 60, 70]]),
        case("4:1:0 1x1", 1, 1, 2, [[90, 1, 2, 3], [4, 5, 6, 7]], [[60]], [[70]], [90, 1, 2, 3, 4, 5, 6, 7, 60, 70], [[0, 0, 90, 60, 70]]),
        # 33 x 9: 2 x 2 MCUs.  A chroma BLOCK covers 32 x 8 (32 x 16) pixels, so the sample at x / 4 changes with the MCU: x = 31 reads
        # chroma column 7 (MCU 0), x = 32 column 8 (MCU 1); for 4:1:1 y = 8 reads chroma row 8 (MCU row 1), for 4:1:0 y = 8 reads chroma
        # row 4 -- still MCU row 0, whose 16 luma rows cover the whole 9-row image
        case("4:1:1 33x9", 33, 9, 1, [[11, 12, 13, 14, 15, 16, 17, 18], [21, 22, 23, 24, 25, 26, 27, 28]], [[101, 102], [103, 104]],
             [[201, 202], [203, 204]],
             [11, 12, 13, 14, 101, 201, 15, 16, 17, 18, 102, 202, 21, 22, 23, 24, 103, 203, 25, 26, 27, 28, 104, 204],
             [[0, 0, 11, 101, 201], [31, 0, 14, 101, 201], [32, 0, 15, 102, 202], [32, 8, 25, 104, 204], [0, 8, 21, 103, 203], [31, 7, 14, 101, 201]]),
        case("4:1:0 33x9", 33, 9, 2, [[11, 12, 13, 14, 15, 16, 17, 18], [21, 22, 23, 24, 25, 26, 27, 28]], [[101, 102]], [[201, 202]],
             [11, 12, 13, 14, 21, 22, 23, 24, 101, 201, 15, 16, 17, 18, 25, 26, 27, 28, 102, 202],
             [[0, 0, 11, 101, 201], [31, 0, 14, 101, 201], [32, 0, 15, 102, 202], [32, 8, 25, 102, 202], [0, 8, 21, 101, 201]]),
    ]
    about = ("Hand known answers for 4:1:1 / 4:1:0 JPEGs (tests/golden/make_jpeg_411_kats.py).  DC-only blocks, every quantiser entry 8, DC = s - 128: "
             "a block's 64 samples are all s.  *_blocks: the block values per component (rows of blocks); y / cb / cr: the MCU-padded planes "
             "spelled out; scan_order: the block values as the interleaved scan codes them; at: [x, y, Y, Cb, Cr] as YCbCrAt reads them; "
             "file: the stream, hex.  ratio 5 / 6 as include/ipx.h numbers 411 / 410.")
    with open(os.path.join(HERE, "jpeg_411_kats.json"), "w") as fh:
        json.dump(dict(about=about, cases=cases), fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
