"""Writes jpeg_dec_kats.json: one-block 8 x 8 Gray JPEGs and the pixels Go's image/jpeg gives for them, derived by hand for
tests/test_jpeg_edge_streams.py -- not with tests/jpeg_decode_model.py.  The streams come from tests/jpeg_writer.py (one DC and one
AC table, a 16-bit DQT where the entry needs it); the answers from closed forms of idct.go for the two block shapes whose rows all
take its shortcut (every row has at most its first term):

  DC only, dequantised value D:         every row but the first is zero, the first is 8D; the column pass leaves
                                         y0 = (8D << 8) + 8192 and every pixel is clip((y0 >> 14) + 128)
  D at natural 0 and A at natural 8:     rows 0 and 1 become 8D and 8A; every column is the same; with a = 8A the column pass gives
                                         Y4 = (W1 a + 4) >> 3, Y5 = (W7 a + 4) >> 3, y2 = (181 (Y4 + Y5) + 128) >> 8,
                                         y4 = (181 (Y4 - Y5) + 128) >> 8, c = (8D << 8) + 8192 and rows
                                         c + Y4, c + y2, c + y4, c + Y5, c - Y5, c - y4, c - y2, c - Y4, each >> 14
All of it in int32 that wraps, as Go computes (wrap() below).  The cases include values where the full row path would wrap and the
shortcut does not (|D| or |A| >= 2^20 after dequantisation: the issue's 16-bit 20000 entry, and DC 3 / -5254 at natural 8 with q 255).

  python tests/golden/make_jpeg_dec_kats.py      # rewrites tests/golden/jpeg_dec_kats.json"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_writer as jw  # noqa: E402

W1, W7, R2 = 2841, 565, 181


def wrap(x):
    return ((int(x) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def pix(v):
    return max(0, min(255, v + 128))


def answer(D, A):
    c = wrap(wrap(wrap(8 * D) << 8) + 8192)
    a = wrap(8 * A)
    Y4 = wrap(W1 * a + 4) >> 3
    Y5 = wrap(W7 * a + 4) >> 3
    y2 = wrap(R2 * wrap(Y4 + Y5) + 128) >> 8
    y4 = wrap(R2 * wrap(Y4 - Y5) + 128) >> 8
    rows = [c + Y4, c + y2, c + y4, c + Y5, c - Y5, c - y4, c - y2, c - Y4]
    return [[pix(wrap(r) >> 14)] * 8 for r in rows]


def stream(dc, ac, q0, q2):
    """one 8 x 8 Gray block: DC value dc, the coefficient ac at zig 2 (natural 8); q0 / q2 the table's entries there"""
    sizes = list(range(17))
    runs = [0x00] + [0x10 | s for s in range(1, 16)] + [s for s in range(1, 16)]
    dct = jw.huff(jw.spread(len(sizes), 2, 16), sizes)
    act = jw.huff(jw.spread(len(runs), 2, 16), runs)
    q = [1] * 64
    q[0], q[2] = q0, q2
    comps = [(1, 1, 1, 0)]
    fr = jw.Frame(8, 8, comps)
    b = np.zeros((1, 1, 64), np.int64)
    b[0, 0, 0], b[0, 0, 2] = dc, ac
    return (jw.soi() + jw.dqt([(0, q, 1 if max(q) > 255 else 0)]) + jw.sof(8, 8, comps) + jw.dht([(0, 0, dct), (1, 0, act)]) +
            jw.sos(comps, [(0, 0, 0)]) + jw.scan(fr, [(0, 0, 0)], [b], ({0: dct}, {0: act})) + jw.eoi())


CASES = [  # name, dc, ac at natural 8, q[0], q[2]
    ("dc_zero", 0, 0, 1, 1), ("dc_one", 1, 0, 1, 1), ("dc_minus_one", -1, 0, 1, 1), ("dc_4", 4, 0, 1, 1), ("dc_minus_4", -4, 0, 1, 1),
    ("dc_minus_5", -5, 0, 1, 1), ("dc_1023_q1", 1023, 0, 1, 1), ("dc_2047_q255", 2047, 0, 255, 1), ("dc_minus_1024_q255", -1024, 0, 255, 1),
    ("dc_16bit_q_wraps", 20, 0, 65535, 1), ("dc_32767_q65535", 32767, 0, 65535, 1), ("dc_minus_32768_q65535", -32768, 0, 65535, 1),
    ("ac8_small", 0, 3, 1, 16), ("ac8_negative", 10, -7, 16, 16), ("ac8_q20000", 3, 1, 1, 20000), ("ac8_q20000_neg", -3, -1, 1, 20000),
    ("ac8_issue_q255", 3, -5254, 255, 255), ("ac8_issue_q255_pos", 3, 5254, 255, 255), ("ac8_32767_q65535", 0, 32767, 1, 65535),
]


def main():
    out = []
    for name, dc, ac, q0, q2 in CASES:
        out.append({"name": name, "jpeg": stream(dc, ac, q0, q2).hex(), "y": answer(dc * q0, ac * q2)})
    with open(os.path.join(HERE, "jpeg_dec_kats.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
