"""Go's image.Decode of a 4:1:1 or 4:1:0 JPEG, restated in numpy: the frame rules of processSOF for these two sampling vectors and the
plane layout of makeImg.  Everything else -- the marker loop, Huffman reader, scans, restart intervals, reconstructBlock, idct.go -- is
tests/jpeg_decode_model.py's, imported and not copied: decode() runs that module's reader with this module's frame-header rule in
place of its own (which refuses h = 4 by design).

The rules are restated from image/jpeg reader.go AS RECALLED: parity with Go is not pinned by this model;
tests/test_jpeg_411_model.py pins the model on hand known answers, on the Gray oracle and (sizes only) on libjpeg.

  processSOF   three components with Y (h, v) in {(4,1), (4,2)} and Cb = Cr = (1,1) are taken; v = 4, a factor of 3, chroma other than
               1 x 1: Unsupported, as before
  makeImg      hRatio << 4 | vRatio = 0x41 -> YCbCrSubsampleRatio411, 0x42 -> ...410 (numbered RATIO_411 = 5, RATIO_410 = 6 here, as
               ipx.h does: Go's own values differ).  MCU 32 x 8 (4 Y blocks in one row, Cb, Cr) and 32 x 16 (8 Y blocks as 2 rows of 4,
               Cb, Cr).  Planes MCU-padded: YStride = 32 * mxx, CStride = 8 * mxx
  chroma       cw = (w + 3) / 4; ch = h (4:1:1) or (h + 1) / 2 (4:1:0); COffset = (y or y / 2) * CStride + x / 4

  decode(data, enabled=True)         a SEQUENTIAL file through the entropy decoder -> dict(w, h, ratio, y, cb, cr, dc_wide); enabled=False:
                                     the switch unset, these files are Unsupported like every sampling outside (1|2) x (1|2)
  from_blocks(frame, blocks, q, progressive=False)
                                     the same planes straight from coefficient blocks (tests/jpeg_writer.py's inputs): what any file of
                                     these coefficients decodes to; progressive=True leaves the blocks that hold no image pixel at zero
                                     (reconstructProgressiveImage)
  status_of(data, enabled=True)      0 / -1 (malformed) / -4 (unsupported): IPX_OK, IPX_ERR_INVALID, IPX_ERR_UNSUPPORTED
  chroma_size, upsample              the operators' view: the 4:4:4 planes whose samples At(x, y) reads"""
import contextlib

import numpy as np

import jpeg_decode_model as jm
from jpeg_decode_model import Malformed, Unsupported, reconstruct

RATIO_411, RATIO_410 = 5, 6
RATIO_OF = {(1, 1): 0, (2, 1): 1, (2, 2): 2, (1, 2): 3, (4, 1): RATIO_411, (4, 2): RATIO_410}
OK, INVALID, UNSUPPORTED = 0, -1, -4


def _sof411(st, b, baseline):
    """processSOF with the two new vectors admitted; the other rules in jpeg_decode_model._sof's order"""
    if st["ncomp"]:
        raise Malformed("multiple SOF markers")
    if len(b) not in (9, 15, 18):
        raise Unsupported("number of components")
    if len(b) == 18:
        raise Unsupported("CMYK")
    nc = 1 if len(b) == 9 else 3
    if b[0] != 8:
        raise Unsupported("precision")
    h, w = b[1] << 8 | b[2], b[3] << 8 | b[4]
    if b[5] != nc:
        raise Malformed("SOF has wrong length")
    ids, hv, tq = [], [], []
    for i in range(nc):
        cid, f, q = b[6 + 3 * i], b[7 + 3 * i], b[8 + 3 * i]
        if cid in ids:
            raise Malformed("repeated component identifier")
        if q > 3:
            raise Malformed("bad Tq value")
        ch, cv = f >> 4, f & 15
        if not (1 <= ch <= 4 and 1 <= cv <= 4):
            raise Malformed("sampling factor")
        if ch == 3 or cv == 3:
            raise Unsupported("sampling factor of 3")
        ids.append(cid)
        hv.append((1, 1) if nc == 1 else (ch, cv))
        tq.append(q)
    if nc == 3 and (hv[1] != (1, 1) or hv[2] != (1, 1) or hv[0] not in RATIO_OF):
        raise Unsupported("subsampling ratio")
    if w <= 0 or h <= 0:
        raise Malformed("empty frame")
    h0, v0 = hv[0]
    st.update(ncomp=nc, w=w, h=h, ids=ids, hv=hv, tq=tq, baseline=baseline,
              mxx=(w + 8 * h0 - 1) // (8 * h0), myy=(h + 8 * v0 - 1) // (8 * v0), ratio=4 if nc == 1 else RATIO_OF[hv[0]])


@contextlib.contextmanager
def _frame_rule(rule):
    old = jm._sof
    jm._sof = rule
    try:
        yield
    finally:
        jm._sof = old


def decode(data, enabled=True, **kw):
    """jpeg_decode_model.decode under this module's frame rule; the planes come out of its _sos, which sizes them from (h0, v0) already:
    y (8 * v0 * myy) x (32 * mxx), cb / cr (8 * myy) x (8 * mxx)"""
    if not enabled:
        return jm.decode(data, **kw)
    with _frame_rule(_sof411):
        return jm.decode(data, **kw)


def status_of(data, enabled=True):
    try:
        out = decode(data, enabled)
    except Malformed:
        return INVALID
    except Unsupported:
        return UNSUPPORTED
    return UNSUPPORTED if out["dc_wide"] else OK


def from_blocks(frame, blocks, q, progressive=False):
    """frame: jpeg_writer.Frame; blocks[c]: (rows, cols, 64) zig-zag; q: {tq: 64 values, zig-zag order}"""
    hv = frame.hv
    if len(frame.comps) != 3 or hv[0] not in RATIO_OF or hv[1] != (1, 1) or hv[2] != (1, 1):
        raise Unsupported("subsampling ratio")
    planes = []
    for c in range(3):
        rows, cols = frame.grid(c)
        assert blocks[c].shape == (rows, cols, 64)
        px = reconstruct(blocks[c].reshape(-1, 64), np.asarray(q[frame.comps[c][3]], np.int64)).reshape(rows, cols, 8, 8)
        if progressive:                                    # only the blocks (bx, by) with bx * 8 * h0 / hc < w and by * 8 * v0 / vc < h
            sx, sy = 8 * hv[0][0] // hv[c][0], 8 * hv[0][1] // hv[c][1]
            keep = (np.arange(rows)[:, None] * sy < frame.h) & (np.arange(cols)[None, :] * sx < frame.w)
            px = px * keep[:, :, None, None].astype(np.uint8)
        planes.append(px.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8))
    return dict(w=frame.w, h=frame.h, ratio=RATIO_OF[hv[0]], y=planes[0], cb=planes[1], cr=planes[2], dc_wide=False)


def chroma_size(ratio, w, h):
    """(cw, ch) of image.NewYCbCr(Rect(0, 0, w, h), ratio)"""
    assert ratio in (RATIO_411, RATIO_410)
    return (w + 3) // 4, h if ratio == RATIO_411 else (h + 1) // 2


def upsample(c, ratio, w, h):
    """the (h, w) plane of the samples YCbCrAt(x, y) reads from a chroma plane: c[y or y / 2, x / 4] -- each sample replicated 4 x across
    and, for 4:1:0, 2 x down"""
    ys = np.arange(h) // (2 if ratio == RATIO_410 else 1)
    return np.ascontiguousarray(c[ys[:, None], (np.arange(w) // 4)[None, :]])
