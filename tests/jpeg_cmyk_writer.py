"""Four-component JPEG files (Adobe CMYK / YCCK) at the coefficient level, for the tests of the IPX_JPEG_CMYK=1 decoder.

Built on tests/jpeg_prog_writer.py (and through it tests/jpeg_writer.py).  Pillow writes only transform-0 files of the sampling vector
11 11 11 11 (or 22 11 11 11 with subsampling=2, which Go refuses); Go's reader takes 11 11 11 11 and 22 11 11 22 with any transform.

  frame4(w, h, v=1, hv=None)          the frame: components 1..4, (h, v) = (v, v) (1, 1) (1, 1) (v, v), or the four pairs of hv (illegal
                                      vectors); quantiser ids 0, 1, 1, 2 -- K has a table of its own
  quants(flat=None)                   {tq: 64 zig-zag values}: three different tables, or `flat` everywhere
  blocks4(frame, seed)                random zig-zag coefficient blocks per component, (rows, cols, 64)
  cmyk_file(frame, blocks, ...)       the file: transform 0 (CMYK) / 1 / 2 (YCCK); baseline (one interleaved scan, restart markers every
                                      `dri` MCUs) or progressive (a libjpeg-like script over four components); app14 "ok" | "absent" |
                                      "short" (an 11-byte Adobe segment: no transform byte)
  split_files(frame, blocks, q, progressive)
                                      the same coefficients as a three-component file (components 0..2) and a Gray file (component 3,
                                      at the size of K's MCU-padded plane) for a three-component decoder

A helper of the tests only."""
import numpy as np

import jpeg_prog_writer as jpw
import jpeg_writer as jw

ILLEGAL_VECTORS = {"22 11 11 11": [(2, 2), (1, 1), (1, 1), (1, 1)], "21 11 11 21": [(2, 1), (1, 1), (1, 1), (2, 1)],
                   "11 11 11 22": [(1, 1), (1, 1), (1, 1), (2, 2)]}


def frame4(w, h, v=1, hv=None):
    hv = hv or [(v, v), (1, 1), (1, 1), (v, v)]
    return jw.Frame(w, h, [(c + 1, hv[c][0], hv[c][1], (0, 1, 1, 2)[c]) for c in range(4)])


def quants(flat=None):
    if flat is not None:
        return {tq: [int(flat)] * 64 for tq in range(3)}
    return {tq: [1 + tq + ((k + tq) >> 2) for k in range(64)] for tq in range(3)}


def blocks4(frame, seed, amp=200, ac=40, density=0.2):
    return jw.all_blocks(frame, np.random.default_rng(seed), amp=amp, ac=ac, density=density)


def script4():
    """spectral selection and successive approximation over four components, in libjpeg's order of ideas"""
    every = [0, 1, 2, 3]
    return ([(every, 0, 0, 0, 1)] + [([c], 1, 5, 0, 2) for c in every] + [([c], 6, 63, 0, 2) for c in (3, 2, 1, 0)] +
            [([c], 1, 63, 2, 1) for c in every] + [(every, 0, 0, 1, 0)] + [([c], 1, 63, 1, 0) for c in (2, 0, 3, 1)])


def _app14(kind, transform):
    if kind == "absent":
        return b""
    if kind == "short":
        return jw.seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0]))          # 11 bytes: Go wants 12
    return jw.app14_adobe(transform)


def _dqt(frame, q):
    return jw.dqt([(tq, q[tq], 0) for tq in sorted({c[3] for c in frame.comps})])


def _baseline(frame, blocks, q, head, dri=0):
    dct = jw.Huff(jw.spread(16, 2, 9), list(range(16)))
    act = jw.Huff(jw.spread(256, 3, 12), sorted(range(256), key=lambda s: (s & 15, s >> 4)))
    sel = [(c, 0, 0) for c in range(len(frame.comps))]
    return (jw.soi() + head + _dqt(frame, q) + jw.sof(frame.w, frame.h, frame.comps, 0xC0) + (jw.dri(dri) if dri else b"") +
            jw.dht([(0, 0, dct), (1, 0, act)]) + jw.sos(frame.comps, sel) + jw.scan(frame, sel, blocks, ({0: dct}, {0: act}), ri=dri) + jw.eoi())


def _progressive(frame, blocks, q, head, script):
    out = jw.soi() + head + _dqt(frame, q) + jw.sof(frame.w, frame.h, frame.comps, 0xC2)
    carry = 0
    for n, (sel, ss, se, ah, al) in enumerate(script):
        S, carry = jpw._scan_tokens(frame, blocks, list(sel), ss, se, ah, al, {}, carry)
        syms = [it[1] for it in S.items if it[0] == "sym"]
        tids, table = (0, 0), None
        if syms:
            table = jpw._table(syms)
            tc, tid = (0 if ss == 0 else 1), n % 4
            out += jw.dht([(tc, tid, table)])
            tids = (tid, 0) if tc == 0 else (0, tid)
        out += jpw._sos(frame, list(sel), tids, ss, se, ah, al) + S.write(table)
    return out + jw.eoi()


def cmyk_file(frame, blocks, transform=0, progressive=False, dri=0, app14="ok", q=None):
    q = q or quants()
    head = _app14(app14, transform)
    if progressive:
        assert not dri
        return _progressive(frame, blocks, q, head, script4())
    return _baseline(frame, blocks, q, head, dri)


def split_files(frame, blocks, q=None, progressive=False):
    """-> (three-component file, Gray file): what a three-component decoder can say about the four planes"""
    q = q or quants()
    f3 = jw.Frame(frame.w, frame.h, frame.comps[:3])
    rows, cols = frame.grid(3)
    fk = jw.Frame(8 * cols, 8 * rows, [(1, 1, 1, frame.comps[3][3])])
    head = jw.app0_jfif()
    if progressive:
        s3 = [([0, 1, 2], 0, 0, 0, 1)] + [([c], 1, 63, 0, 1) for c in range(3)] + [([0, 1, 2], 0, 0, 1, 0)] + [([c], 1, 63, 1, 0) for c in range(3)]
        sk = [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 1), ([0], 1, 63, 1, 0)]
        return _progressive(f3, blocks[:3], q, head, s3), _progressive(fk, [blocks[3]], q, head, sk)
    return _baseline(f3, blocks[:3], q, head), _baseline(fk, [blocks[3]], q, head)
