"""The 4:1:1 / 4:1:0 JPEG files of the IPX_JPEG_411 tests, written at the coefficient level with tests/jpeg_writer.py (sequential files)
and tests/jpeg_prog_writer.py (progressive files).  One quantiser for every table id (jpeg_prog_writer's default), so that a file of
any kind built from the same blocks decodes to jpeg_411_model.from_blocks(frame, blocks, Q).  A helper of the tests only."""
import numpy as np

import jpeg_edge_corpus as ec
import jpeg_prog_writer as pw
import jpeg_writer as jw

QV = pw._quant(None)
Q = {0: QV, 1: QV}
# the sizes the issue names, and the edges of jpeg_idct_kernel's workgroup: 8 MCUs of 32 columns for 4:1:1 (6 blocks per MCU), 4 for
# 4:1:0 (10 blocks per MCU); heights either side of an MCU row (8 / 16 rows)
SIZES = {1: [(1, 1), (31, 7), (32, 8), (33, 9), (65, 17), (7 * 32, 7), (8 * 32, 8), (9 * 32, 9), (8 * 32 + 1, 16)],
         2: [(1, 1), (31, 7), (32, 8), (33, 9), (65, 17), (3 * 32, 15), (4 * 32, 16), (5 * 32, 17), (4 * 32 + 1, 33)]}


def frame(w, h, v0=1, h0=4, chroma=(1, 1)):
    """v0 = 1: 4:1:1, v0 = 2: 4:1:0; other h0 / chroma for the vectors Go refuses"""
    return jw.Frame(w, h, [(1, h0, v0, 0), (2, chroma[0], chroma[1], 1), (3, chroma[0], chroma[1], 1)])


def blocks(fr, seed, amp=200, ac=40, density=0.2):
    return jw.all_blocks(fr, np.random.default_rng(seed), amp=amp, ac=ac, density=density)


def _tables():
    dc, ac, _ = ec.tables_short()
    return {(0, 0): dc, (1, 0): ac, (0, 1): dc, (1, 1): ac}


def baseline(fr, b, ri=0, scans=None):
    """one interleaved baseline scan (restart markers every ri MCUs), or the scans given: [[(component, td, ta)]]"""
    return ec.file(fr.w, fr.h, fr.comps, b, _tables(), {0: (QV, 0), 1: (QV, 0)}, ri=ri, scans=scans)


def multiscan(fr, b):
    """a sequential frame in three non-interleaved scans (Y walks its own 4-wide block grid)"""
    return baseline(fr, b, scans=[[(0, 0, 0)], [(2, 1, 1)], [(1, 1, 1)]])


def progressive(fr, b):
    """SOF2 with libjpeg's scan script: interleaved DC scans, non-interleaved AC bands, refinements"""
    return pw.progressive(fr, b, pw.libjpeg_script(fr))


def cut_in_scan(data, keep=0.6):
    """the file cut inside its entropy-coded data (no EOI): malformed"""
    sos = data.index(b"\xff\xda")
    return data[:sos + int((len(data) - sos) * keep)]


def scan_len(data):
    """bytes of entropy-coded data of a single-scan file"""
    sos = data.index(b"\xff\xda")
    start = sos + 2 + (data[sos + 2] << 8 | data[sos + 3])
    return len(data) - 2 - start


# frames Go refuses, whatever the switch says: (name, frame arguments)
REFUSED = [("Y 4x4", dict(v0=4)), ("Y 4x1 over 2x1 chroma", dict(v0=1, chroma=(2, 1))), ("Y 3x1", dict(h0=3, v0=1))]


def refused_file(w, h, **kw):
    """the frame header is what counts: the parsers refuse these before any scan is read, so the scan is a 4:1:1 file's"""
    fr = frame(w, h, 1)
    data = baseline(fr, blocks(fr, 9))
    bad = jw.sof(w, h, frame(w, h, **kw).comps)
    good = jw.sof(w, h, fr.comps)
    assert data.count(good) == 1
    return data.replace(good, bad)
