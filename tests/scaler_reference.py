"""An independent float64 reference for the scaler and the colour conversions, with a margin per byte.

Every other pixel test compares a HIP kernel with the project's C restatement of Go's integer and float64 code, written by the
same hands as the kernels.  This module restates nothing of that code: it builds each source type's colour from the colour
model's definition in real numbers, and interpolates with torch's antialiased bilinear filter (the same tent kernel as x/image's
BiLinear, support widened by the downscale ratio, weights renormalised at the edges -- written by other people).  Then it applies
the rest of kernelScaler.Scale in real arithmetic: colour clamped to alpha, Over, ftou, >> 8.

Two float64 evaluations of one real number agree to about 1e-12, but Go's taps are integers that may sit up to `e` away from the
real colour (a truncating division, a fixed-point coefficient).  So a byte is only decided when the exact value lies further than
the error bound from a rounding boundary.  Every result here is a Ref(byte, margin, tol): the byte of the real value, the distance
of that value from the nearest boundary (16-bit units, boundaries 256 k for k = 1..255; 0 and 65535 saturate and are not
boundaries) and the bound the integer code can be off by.  assert_matches() then asks for exact equality wherever margin > tol
and for +-1 elsewhere.  Over is the one step whose integer form is its definition (x/image stores (d * (0xffff - a) * 0x101 /
0xffff + c) >> 8): there the store is evaluated over the whole range of integers c and a the bounds allow, and tol is -inf where
that range gives one byte, inf where it does not.

Plain numpy and torch on CPU tensors; nothing here reads the project's C restatement or its kernels.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

OP_OVER, OP_SRC = 0, 1

# Two float64 evaluations of the same sums in a different order differ by far less than this (16-bit units).
FLOAT_SLACK = 1e-6

# YCbCr -> RGB (JFIF): R = Y + 1.402 Cr', G = Y - 0.344136 Cb' - 0.714136 Cr', B = Y + 1.772 Cb', with Cb' = Cb - 128, Cr' = Cr - 128.
KR, KGB, KGR, KB = 1.402, 0.344136, 0.714136, 1.772

# Error bounds, in 16-bit units, of Go's integer taps against the real colour.
#  The 16-bit YCbCr tap (color.YCbCr.RGBA) is (Y * 0x10101 + c1 * Cr' ...) >> 8 against the real 257 Y + 256 * 1.402 Cr':
#  Y * 0x10101 / 256 = 257 Y + Y / 256 (at most 0.997 over), the fixed-point coefficients are at most 0.47 / 65536 off the
#  real ones (91881 vs 1.402 * 65536 = 91881.47; 22554 + 46802 vs 22553.6 + 46802.4 for green: 0.38 * 128 / 256 = 0.19 each),
#  and the >> 8 truncates (up to 1): 0.997 + 0.38 + 1 < 2.4.
E_YCBCR_TAP = 2.4
#  color.YCbCrToRGB (draw.Draw's 8-bit conversion) keeps the >> 16 to the very end: the same coefficient terms in 16-bit units,
#  without the truncation in between: 0.997 + 0.38 < 1.4 (0.0055 of a byte).
E_YCBCR_DRAW = 1.4
#  one truncating division (c * a / 0xff, c * a / 0xffff, CMYK's product / 0xffff): at most 1 below the real value.
E_TRUNC = 1.0

Ref = collections.namedtuple("Ref", "byte margin tol")


class Taps:
    """A source image as the scaler sees it: premultiplied 16-bit colour per pixel in real numbers, (h, w, 4) float64.

    e:         how far Go's integer tap may be from this value (any channel);
    draw_e:    the same for draw.Draw's 8-bit conversion, where the integer code keeps floor(floor(x) / 256) = floor(x / 256)
               and so is exact for truncating divisions (0), but not for YCbCrToRGB's fixed-point coefficients;
    alpha_one: the type's scaleX writes a literal alpha 1 (Gray, YCbCr) -- in real numbers the same as interpolating 0xffff's;
    opaque:    the image's Opaque(): kernelScaler.Scale turns Over into Src."""

    def __init__(self, taps, e, draw_e=0.0, alpha_one=False, kind=""):
        self.taps = np.asarray(taps, np.float64)
        assert self.taps.ndim == 3 and self.taps.shape[2] == 4
        self.e, self.draw_e, self.alpha_one, self.kind = float(e), float(draw_e), alpha_one, kind
        self.opaque = alpha_one or bool((self.taps[..., 3] == 65535.0).all())

    @property
    def shape(self):
        return self.taps.shape[:2]


def _premul(c, a):
    """color.NRGBA-style: 8-bit colour c and alpha a in real 16-bit units: c * 257 * a * 257 / 65535, alpha a * 257."""
    c = np.asarray(c, np.float64) * 257.0
    a = np.asarray(a, np.float64) * 257.0
    return np.concatenate([c * a[..., None] / 65535.0, a[..., None]], -1)


def rgba(px):
    """*image.RGBA: already premultiplied, c * 257."""
    return Taps(np.asarray(px, np.float64) * 257.0, 0.0, kind="rgba")


def nrgba(px):
    """*image.NRGBA: straight alpha, premultiplied per tap."""
    px = np.asarray(px)
    return Taps(_premul(px[..., :3], px[..., 3]), E_TRUNC, kind="nrgba")


def gray(g):
    """*image.Gray: y * 257 in every colour channel, alpha a literal 1."""
    g = np.asarray(g, np.float64) * 257.0
    return Taps(np.stack([g, g, g, np.full_like(g, 65535.0)], -1), 0.0, alpha_one=True, kind="gray")


RATIO_444, RATIO_422, RATIO_420, RATIO_440 = 0, 1, 2, 3
RATIO_411, RATIO_410 = 5, 6                    # include/ipx.h's numbers (4 is Gray there; Go's own values differ)


def ycbcr_real(y, cb, cr, ratio, x0=0, y0=0):
    """Real 16-bit RGB of an *image.YCbCr (Rect.Min = (0, 0)) over its whole plane, or of the pixels from (x0, y0) on: chroma is
    the sample at (x >> hs, y >> vs) of the ABSOLUTE coordinate.  Unclamped, (h, w, 3)."""
    y = np.asarray(y, np.float64)
    h, w = y.shape
    hs = 2 if ratio in (RATIO_411, RATIO_410) else 1 if ratio in (RATIO_422, RATIO_420) else 0
    vs = 1 if ratio in (RATIO_420, RATIO_440, RATIO_410) else 0
    ys, xs = np.arange(y0, h)[:, None], np.arange(x0, w)[None, :]
    cbp = np.asarray(cb, np.float64)[ys >> vs, xs >> hs] - 128.0
    crp = np.asarray(cr, np.float64)[ys >> vs, xs >> hs] - 128.0
    yy = 257.0 * y[y0:, x0:]
    return np.stack([yy + 256.0 * KR * crp, yy - 256.0 * (KGB * cbp + KGR * crp), yy + 256.0 * KB * cbp], -1)


def ycbcr(y, cb, cr, ratio):
    """*image.YCbCr: the JFIF conversion in real numbers, clamped to [0, 65535] (clamping keeps the bound), alpha a literal 1."""
    rgb = np.clip(ycbcr_real(y, cb, cr, ratio), 0.0, 65535.0)
    return Taps(np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 65535.0)], -1), E_YCBCR_TAP, E_YCBCR_DRAW, alpha_one=True,
                kind="ycbcr")


def paletted(idx, pal, entry="nrgba"):
    """*image.Paletted: the entry's premultiplied colour.  entry "rgba": color.RGBA entries (GIF; PNG without tRNS), taken as
    they are (c * 257, exact); "nrgba": color.NRGBA entries (PNG with tRNS), premultiplied."""
    pal = np.zeros((256, 4), np.uint8) if pal is None else np.asarray(pal, np.uint8)
    if entry == "rgba":
        p16, e = pal.astype(np.float64) * 257.0, 0.0
    else:
        p16, e = _premul(pal[:, :3], pal[:, 3]), E_TRUNC
    return Taps(p16[np.asarray(idx, np.intp)], e, kind="paletted-" + entry)


def nrgba64(v):
    """*image.NRGBA64: c * a / 65535, alpha a."""
    v = np.asarray(v, np.float64)
    return Taps(np.concatenate([v[..., :3] * v[..., 3:4] / 65535.0, v[..., 3:4]], -1), E_TRUNC, kind="nrgba64")


def rgba64(v):
    """*image.RGBA64: as stored."""
    return Taps(np.asarray(v, np.float64), 0.0, kind="rgba64")


def gray16(v):
    """*image.Gray16: y in every colour channel, alpha 65535."""
    v = np.asarray(v, np.float64)
    return Taps(np.stack([v, v, v, np.full_like(v, 65535.0)], -1), 0.0, kind="gray16")


def cmyk(v):
    """*image.CMYK: (65535 - 257 c) (65535 - 257 k) / 65535, alpha 65535."""
    v = np.asarray(v, np.float64)
    w = 65535.0 - 257.0 * v[..., 3:4]
    rgb = (65535.0 - 257.0 * v[..., :3]) * w / 65535.0
    return Taps(np.concatenate([rgb, np.full_like(w, 65535.0)], -1), E_TRUNC, kind="cmyk")


# ---- bytes and margins -----------------------------------------------------------------------------------------------------

def _byte(v):
    return np.clip(np.floor(v / 256.0), 0, 255).astype(np.uint8)


def _margin(v):
    """distance of v from the nearest boundary 256 k, k = 1..255"""
    k = np.clip(np.rint(v / 256.0), 1, 255)
    return np.abs(v - 256.0 * k)


def _interp(t, dw, dh):
    """(h, w, c) float64 -> (dh, dw, c): torch's antialiased bilinear, float64 on the CPU."""
    x = torch.from_numpy(np.ascontiguousarray(np.moveaxis(t, -1, 0)))[None]
    y = F.interpolate(x, size=(dh, dw), mode="bilinear", antialias=True, align_corners=False)
    return np.moveaxis(y[0].numpy(), 0, -1)


def _over(d, c_lo, c_hi, a_lo, a_hi, c):
    """Over onto destination bytes d.  The integer code stores (d * (65535 - a) * 0x101 / 0xffff + p) >> 8, a truncating division,
    where p and a are the 16-bit colour and alpha it reached.  Given the ranges [c_lo, c_hi], [a_lo, a_hi] those integers can lie in
    (from the real values and their bounds), the stored byte lies between two bytes; it is decided where they are one.  The real
    value d * 257 * (65535 - a) / 65535 + c gives the margin that is reported.  -> Ref parts (byte, margin, tol)."""
    d = np.asarray(d, np.int64)
    lo = (d * (65535 - a_hi) * 257) // 65535 + c_lo
    hi = (d * (65535 - a_lo) * 257) // 65535 + c_hi
    b_lo, b_hi = np.minimum(lo >> 8, 255), np.minimum(hi >> 8, 255)
    a = (a_lo + a_hi) / 2.0
    v = d * 257.0 * (65535.0 - a) / 65535.0 + c
    decided = b_lo == b_hi
    return np.where(decided, b_lo, _byte(v)).astype(np.uint8), _margin(v), np.where(decided, -np.inf, np.inf)


def _ftou_range(x, e):
    """ftou(x') = floor(x' + 0.5) for every x' within e of x"""
    return (np.clip(np.floor(x + 0.5 - e - FLOAT_SLACK), 0, 65535).astype(np.int64),
            np.clip(np.floor(x + 0.5 + e + FLOAT_SLACK), 0, 65535).astype(np.int64))


def _floor_range(x, e):
    """floor(x') for every x' within e of x, where x is exact integer arithmetic's value (a float64 within FLOAT_SLACK of an
    integer IS that integer)"""
    r = np.rint(x)
    x = np.where(np.abs(x - r) < FLOAT_SLACK, r, x)
    return np.floor(x - e).astype(np.int64), np.floor(x + e).astype(np.int64)


def scale(src, dw, dh, sr=None, op=OP_OVER, dst=None):
    """BiLinear.Scale(dst, dst.Bounds(), src, sr, op, nil) onto a dh x dw RGBA frame (zeros by default) -> Ref."""
    t = src.taps
    if sr is not None:
        x0, y0, x1, y1 = sr
        t = t[y0:y1, x0:x1]
    f = _interp(t, dw, dh)                           # weighted averages of taps, 16-bit units
    a = np.full(f.shape[:2], 65535.0) if src.alpha_one else f[..., 3]
    c = np.concatenate([np.minimum(f[..., :3], a[..., None]), a[..., None]], -1)   # colour clamped to alpha
    if op == OP_SRC or src.opaque:
        # ftou(x) = floor(x + 0.5) when x is in range, then >> 8: floor((x + 0.5) / 256) exactly; only the taps' own error remains
        v = c + 0.5
        return Ref(_byte(v), _margin(v), src.e + FLOAT_SLACK)
    if dst is None:
        dst = np.zeros((dh, dw, 4), np.uint8)
    c_lo, c_hi = _ftou_range(c, np.array([src.e] * 3 + [0.0]))        # alpha taps are exact in every type
    a_lo, a_hi = c_lo[..., 3:4], c_hi[..., 3:4]
    return Ref(*_over(dst, c_lo, c_hi, a_lo, a_hi, c))


def _clip(dshape, r, sshape, sp):
    """draw.clip: r within the destination and within the source placed at r.Min - sp -> (r, sp) or None"""
    x0, y0, x1, y1 = r
    ox, oy = x0, y0
    dh, dw = dshape
    sh, sw = sshape
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, dw), min(y1, dh)
    x0, y0 = max(x0, ox - sp[0]), max(y0, oy - sp[1])
    x1, y1 = min(x1, ox - sp[0] + sw), min(y1, oy - sp[1] + sh)
    if x0 >= x1 or y0 >= y1:
        return None
    return (x0, y0, x1, y1), (sp[0] + x0 - ox, sp[1] + y0 - oy)


def draw(dst, r, src, sp=(0, 0), op=OP_SRC):
    """draw.Draw(dst, r, src, sp, op) onto an RGBA frame -> Ref over the whole destination (untouched pixels: margin inf).
    Src stores floor(x / 256) of the source's 16-bit colour x; Over stores floor((d * 257 * (65535 - a) / 65535 + x) / 256)
    with up to two truncations on the way.  CMYK and YCbCr are opaque: either op stores the conversion."""
    dst = np.asarray(dst, np.uint8)
    byte = dst.copy()
    margin = np.full(dst.shape, np.inf)
    tol = np.zeros(dst.shape)
    cl = _clip(dst.shape[:2], r, src.shape, sp)
    if cl is None:
        return Ref(byte, margin, tol)
    (x0, y0, x1, y1), (sx, sy) = cl
    s = src.taps[sy:sy + y1 - y0, sx:sx + x1 - x0]
    if op == OP_SRC or src.kind in ("cmyk", "ycbcr"):
        v, t = s, src.draw_e + FLOAT_SLACK
    else:
        # the source's colour is truncated once before it is added (drawNRGBAOver, drawRGBA: floor of the exact value)
        s_lo, s_hi = _floor_range(s, src.draw_e)
        (byte[y0:y1, x0:x1], margin[y0:y1, x0:x1], tol[y0:y1, x0:x1]) = _over(dst[y0:y1, x0:x1], s_lo, s_hi, s_lo[..., 3:4],
                                                                              s_hi[..., 3:4], s)
        return Ref(byte, margin, tol)
    byte[y0:y1, x0:x1] = _byte(v)
    margin[y0:y1, x0:x1] = _margin(v)
    tol[y0:y1, x0:x1] = t
    return Ref(byte, margin, tol)


def crop_thumbnail(src, crop, tw, th, stage1):
    """cropAndResize (thumbnail.go:128-131): an equal-size Scale of the crop rectangle onto a zeroed frame, then resizeImage of that
    RGBA frame.  Stage 1 is checked here against `stage1`, the bytes the code under test made of it: exact where the
    reference is clear of a boundary, +-1 elsewhere.  Stage 2 then reads those bytes -- where stage 1 was clear they ARE the
    reference's -- so the second stage's reference is exact in its input.  Returns (Ref of stage 2, Ref of stage 1)."""
    cs = crop[2] - crop[0]
    r1 = scale(src, cs, cs, sr=crop)
    assert_matches(stage1, *r1, max_ambiguous=1.0, what="thumbnail crop (stage 1)")
    return scale(rgba(stage1), tw, th), r1


# ---- the comparison --------------------------------------------------------------------------------------------------------

def ambiguous(margin, tol):
    return ~(np.asarray(margin) > np.asarray(tol))


def assert_matches(got, ref, margin, tol, max_ambiguous, what=""):
    """Every byte clear of a boundary (margin > tol) equals the reference; every byte is within 1 of it; and at most a share
    max_ambiguous of the bytes (plus one pixel's four, for the tiniest outputs) is ambiguous, so the check cannot quietly become
    empty.  Returns the ambiguous share."""
    got = np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape, "%s: shape %r, reference %r" % (what, got.shape, ref.shape)
    amb = ambiguous(margin, tol)
    amb = np.broadcast_to(amb, ref.shape)
    diff = got.astype(np.int32) - ref.astype(np.int32)
    bad = (diff != 0) & ~amb
    if bad.any():
        where = np.argwhere(bad)[:8]
        m = np.broadcast_to(margin, ref.shape)
        raise AssertionError("%s: %d of %d bytes clear of a rounding boundary differ from the float64 reference; first at %s "
                             "(got %s, reference %s, margins %s)"
                             % (what, int(bad.sum()), int((~amb).sum()), [tuple(int(i) for i in w) for w in where],
                                [int(got[tuple(w)]) for w in where], [int(ref[tuple(w)]) for w in where],
                                [round(float(m[tuple(w)]), 3) for w in where]))
    far = np.abs(diff) > 1
    if far.any():
        w = tuple(int(i) for i in np.argwhere(far)[0])
        raise AssertionError("%s: %d bytes differ from the float64 reference by more than 1; first at %s (got %d, reference %d)"
                             % (what, int(far.sum()), w, int(got[w]), int(ref[w])))
    share = float(amb.mean()) if amb.size else 0.0
    assert amb.sum() <= max_ambiguous * amb.size + 4, "%s: %.4f of the bytes are ambiguous, above the cap %.4f" % (what, share, max_ambiguous)
    return share
