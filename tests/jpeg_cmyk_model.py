"""Go's image.Decode of a four-component JPEG, restated in numpy: the four-component rules of processSOF, the planes, and applyBlack.

Built on tests/jpeg_decode_model.py's Table, Bits, idct and reconstruct (imported, not copied).  The rules are restated from image/jpeg
reader.go AS RECALLED: parity with Go is not pinned by this model; tests/test_jpeg_cmyk_model.py pins the model
on the three-component oracle, on hand known answers and on libjpeg.

  processSOF    four components are legal only with (h, v) = 11 11 11 11 or 22 11 11 22: anything else is Unsupported
  APP14         at least 12 bytes starting with "Adobe": the transform is byte 11; a four-component file without one is Unsupported
                ("unknown color model")
  planes        components 0..2 into an *image.YCbCr (4:4:4 or 4:2:0), component 3 into blackPix (stride 8 * h3 * mxx, component 0's
                resolution); a progressive file leaves the blocks that hold no image pixel at zero
  applyBlack    transform != 0: DrawYCbCr of the three planes, then Pix[4i+3] = 255 - K; transform == 0: Pix[4i+t] = 255 - plane_t at
                the pixel's coordinates, halved for a component whose (h, v) differs from component 0's

  decode(data)                              a SEQUENTIAL file (interleaved or not, restart intervals) through the entropy decoder
  from_blocks(frame, blocks, q, transform, progressive)
                                            the same from coefficient blocks (tests/jpeg_cmyk_writer.py's inputs): what a progressive
                                            file of these coefficients decodes to
Both return dict(w, h, v, transform, y, cb, cr, k, pix) -- the MCU-padded planes and the (h, w, 4) *image.CMYK pixels."""
import numpy as np

from jpeg_decode_model import Bits, Malformed, Table, Unsupported, i32, reconstruct

LEGAL = ([(1, 1)] * 4, [(2, 2), (1, 1), (1, 1), (2, 2)])


def ycbcr_to_rgb(y, cb, cr):
    """color.YCbCrToRGB on uint8 arrays"""
    yy1 = y.astype(np.int64) * 0x10101
    cb1, cr1 = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    out = []
    for v in (yy1 + 91881 * cr1, yy1 - 22554 * cb1 - 46802 * cr1, yy1 + 116130 * cb1):
        v = i32(v)
        out.append(np.where((v & 0xFF000000) == 0, v >> 16, ~(v >> 31)).astype(np.uint8))
    return out


def apply_black(w, h, v, transform, y, cb, cr, k):
    yy, kk = y[:h, :w], k[:h, :w]
    if v == 2:                                                 # the pixel's coordinates halved
        ys, xs = np.arange(h)[:, None] // 2, np.arange(w)[None, :] // 2
        bb, rr = cb[ys, xs], cr[ys, xs]
    else:
        bb, rr = cb[:h, :w], cr[:h, :w]
    pix = np.zeros((h, w, 4), np.uint8)
    if transform != 0:
        pix[..., 0], pix[..., 1], pix[..., 2] = ycbcr_to_rgb(yy, bb, rr)
    else:
        pix[..., 0], pix[..., 1], pix[..., 2] = 255 - yy, 255 - bb, 255 - rr
    pix[..., 3] = 255 - kk
    return pix


def _planes(w, h, hv, grids, coefs, qs, progressive):
    """coefs[c]: (rows, cols, 64) zig-zag; qs[c]: the component's table -> the four MCU-padded planes"""
    out = []
    for c in range(4):
        rows, cols = grids[c]
        px = reconstruct(coefs[c].reshape(-1, 64), qs[c]).reshape(rows, cols, 8, 8)
        if progressive:                                        # reconstructProgressiveImage: only blocks that hold an image pixel
            sx, sy = 8 * hv[0][0] // hv[c][0], 8 * hv[0][1] // hv[c][1]
            keep = (np.arange(rows)[:, None] * sy < h) & (np.arange(cols)[None, :] * sx < w)
            px = px * keep[:, :, None, None].astype(np.uint8)
        out.append(px.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8))
    return out


def _result(w, h, hv, transform, planes):
    y, cb, cr, k = planes
    return dict(w=w, h=h, v=hv[0][1], transform=transform, y=y, cb=cb, cr=cr, k=k, pix=apply_black(w, h, hv[0][1], transform, y, cb, cr, k))


def from_blocks(frame, blocks, q, transform, progressive=False):
    if list(frame.hv) not in LEGAL:
        raise Unsupported("subsampling ratio")
    grids = [frame.grid(c) for c in range(4)]
    qs = [np.asarray(q[frame.comps[c][3]], np.int64) for c in range(4)]
    return _result(frame.w, frame.h, frame.hv, transform, _planes(frame.w, frame.h, frame.hv, grids, blocks, qs, progressive))


def decode(data):
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise Malformed("missing SOI marker")
    quant = np.zeros((4, 64), np.int64)
    huff, sof, ri, adobe, coefs, pos, n = {}, None, 0, None, None, 2, len(data)
    while True:
        if pos + 2 > n:
            raise Malformed("unexpected EOF")
        if data[pos] != 0xFF:
            pos += 1
            continue
        marker = data[pos + 1]
        pos += 2
        if marker in (0, 0xFF) or 0xD0 <= marker <= 0xD7:
            pos -= 1 if marker == 0xFF else 0
            continue
        if marker == 0xD9:
            break
        if pos + 2 > n:
            raise Malformed("unexpected EOF")
        ln = (data[pos] << 8 | data[pos + 1]) - 2
        if ln < 0 or pos + 2 + ln > n:
            raise Malformed("segment length")
        body = data[pos + 2:pos + 2 + ln]
        pos += 2 + ln
        if marker in (0xC0, 0xC1):
            if sof:
                raise Malformed("multiple SOF markers")
            if ln != 18 or body[5] != 4:
                raise Unsupported("not a four-component frame (outside this model)")
            if body[0] != 8:
                raise Unsupported("precision")
            h, w = body[1] << 8 | body[2], body[3] << 8 | body[4]
            ids = [body[6 + 3 * c] for c in range(4)]
            hv = [(body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15) for c in range(4)]
            tq = [body[8 + 3 * c] for c in range(4)]
            if len(set(ids)) != 4 or max(tq) > 3 or not all(1 <= f <= 4 for p in hv for f in p):
                raise Malformed("frame header")
            if hv not in LEGAL:
                raise Unsupported("subsampling ratio")
            if w <= 0 or h <= 0:
                raise Malformed("empty frame")
            v = hv[0][0]
            sof = dict(w=w, h=h, ids=ids, hv=hv, tq=tq, mxx=(w + 8 * v - 1) // (8 * v), myy=(h + 8 * v - 1) // (8 * v))
        elif marker == 0xC2:
            raise Unsupported("progressive (outside this model: from_blocks)")
        elif marker == 0xC4:
            k = 0
            while k < ln:
                counts = list(body[k + 1:k + 17])
                if ln - k < 17 or body[k] >> 4 > 1 or body[k] & 15 > 3 or not 0 < sum(counts) <= 256 or k + 17 + sum(counts) > ln:
                    raise Malformed("DHT")
                huff[body[k] >> 4, body[k] & 15] = Table(counts, body[k + 17:k + 17 + sum(counts)])
                k += 17 + sum(counts)
        elif marker == 0xDB:
            k = 0
            while k < ln:
                pq, t = body[k] >> 4, body[k] & 15
                need = 128 if pq else 64
                if t > 3 or pq > 1 or k + 1 + need > ln:
                    raise Malformed("DQT")
                quant[t] = np.frombuffer(body[k + 1:k + 1 + need], ">u2" if pq else np.uint8).astype(np.int64)
                k += 1 + need
        elif marker == 0xDD:
            if ln != 2:
                raise Malformed("DRI has wrong length")
            ri = body[0] << 8 | body[1]
        elif marker == 0xEE:
            if ln >= 12 and body[:5] == b"Adobe":
                adobe = body[11]
        elif marker == 0xDA:
            if not sof:
                raise Malformed("missing SOF marker")
            if coefs is None:
                coefs = [np.zeros((sof["myy"] * sof["hv"][c][1], sof["mxx"] * sof["hv"][c][0], 64), np.int64) for c in range(4)]
            pos = _scan(data, body, pos, sof, huff, ri, coefs)
        elif 0xE0 <= marker <= 0xEF or marker == 0xFE:
            pass
        else:
            raise Malformed("unknown marker") if marker < 0xC0 else Unsupported("unknown marker")
    if coefs is None:
        raise Malformed("missing SOS marker")
    if adobe is None:
        raise Unsupported("unknown color model")
    grids = [c.shape[:2] for c in coefs]
    qs = [quant[sof["tq"][c]] for c in range(4)]
    return _result(sof["w"], sof["h"], sof["hv"], adobe, _planes(sof["w"], sof["h"], sof["hv"], grids, coefs, qs, False))


def _scan(data, b, pos, sof, huff, ri, coefs):
    """one sequential scan into coefs; -> the position behind the bytes the entropy decoder used"""
    if len(b) < 6 or len(b) > 12 or len(b) % 2 or len(b) != 4 + 2 * b[0]:
        raise Malformed("SOS has wrong length")
    sel = []
    for i in range(b[0]):
        if b[1 + 2 * i] not in sof["ids"]:
            raise Malformed("unknown component selector")
        c = sof["ids"].index(b[1 + 2 * i])
        if c in [s[0] for s in sel]:
            raise Malformed("repeated component selector")
        sel.append((c, b[2 + 2 * i] >> 4, b[2 + 2 * i] & 15))
    hv, mxx, myy = sof["hv"], sof["mxx"], sof["myy"]
    if sum(hv[c][0] * hv[c][1] for c, _, _ in sel) > 10:
        raise Malformed("total sampling factors too large")
    for c, td, ta in sel:
        if (0, td) not in huff or (1, ta) not in huff:
            raise Malformed("uninitialized Huffman table")
    br = Bits(data, pos)
    dc, rst, eobrun = [0] * 4, 0xD0, 0
    nbx = nby = 0
    for m in range(mxx * myy):
        my, mx = divmod(m, mxx)
        for c, td, ta in sel:
            hi, vi = hv[c]
            for j in range(hi * vi):
                if len(sel) != 1:
                    bx, by = hi * mx + j % hi, vi * my + j // hi
                else:
                    bx, by = nbx, nby
                    nbx += 1
                    if nbx == mxx * hi:
                        nbx, nby = 0, nby + 1
                    if bx * 8 >= sof["w"] or by * 8 >= sof["h"]:
                        continue
                zz = np.zeros(64, np.int64)
                t = br.huffman(huff[0, td])
                if t > 16:
                    raise Unsupported("excessive DC component")
                dc[c] = int(i32(np.int64(dc[c] + br.receive_extend(t))))
                zz[0] = dc[c]
                if eobrun > 0:
                    eobrun -= 1
                else:
                    zig = 1
                    while zig <= 63:
                        val = br.huffman(huff[1, ta])
                        r, s = val >> 4, val & 15
                        if s:
                            zig += r
                            if zig > 63:
                                break
                            zz[zig] = br.receive_extend(s)
                        elif r == 15:
                            zig += 15
                        else:
                            eobrun = ((1 << r) | (br.bits(r) if r else 0)) - 1
                            break
                        zig += 1
                coefs[c][by, bx] = zz
        if ri and (m + 1) % ri == 0 and m + 1 < mxx * myy:
            br.reset()
            if br.pos + 2 > len(data):
                raise Malformed("unexpected EOF")
            if data[br.pos] != 0xFF or data[br.pos + 1] != rst:
                raise Unsupported("restart marker not where it belongs")
            br.pos += 2
            rst = 0xD0 if rst == 0xD7 else rst + 1
            dc, eobrun = [0] * 4, 0
    br.reset()
    return br.pos
