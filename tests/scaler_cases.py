"""Source images of every type the scaler takes, each with the oracle's routines for it and its float64 reference
(tests/scaler_reference.py), for tests/test_scaler_reference.py and tests/test_scaler_reference_gpu.py."""
import numpy as np

import jpeg_411_model as M411
import oracle
import scaler_reference as R
from oracle import DEEP_CMYK, DEEP_GRAY16, DEEP_NRGBA64, DEEP_RGBA64

KINDS = ["rgba", "nrgba", "gray", "ycbcr444", "ycbcr422", "ycbcr420", "ycbcr440", "ycbcr411", "ycbcr410", "paletted-gif",
         "paletted-trns", "nrgba64", "rgba64", "gray16", "cmyk"]
ALPHA_KINDS = ["rgba", "nrgba", "paletted-trns", "nrgba64", "rgba64"]
DEEP = {"nrgba64": DEEP_NRGBA64, "rgba64": DEEP_RGBA64, "gray16": DEEP_GRAY16, "cmyk": DEEP_CMYK}
RATIO = {"ycbcr444": 0, "ycbcr422": 1, "ycbcr420": 2, "ycbcr440": 3, "ycbcr411": M411.RATIO_411, "ycbcr410": M411.RATIO_410}
# 4:1:1 and 4:1:0 have no routine of their own in the oracle: x/image/draw takes them through At(x, y).RGBA(), the same integer
# conversion with the chroma sample at (x / 4, y or y / 2), so the oracle runs at 4:4:4 on planes whose samples
# are replicated (jpeg_411_model.upsample).  The float64 reference reads the subsampled planes themselves.
RATIOS_41X = (M411.RATIO_411, M411.RATIO_410)

# The largest share of ambiguous bytes (exact value within the integer code's error bound of a rounding boundary) a case may
# have, per source type: about twice the most seen over this suite's cases (outputs of 1000 bytes and more; assert_matches allows
# one pixel more, for the tiniest).
MAX_AMBIGUOUS = {"rgba": 0.005, "nrgba": 0.025, "gray": 0.002, "ycbcr": 0.05, "paletted-gif": 0.008, "paletted-trns": 0.03,
                 "nrgba64": 0.025, "rgba64": 0.01, "gray16": 0.008, "cmyk": 0.02}


# Alpha only from {0, 1, 254, 255}: a = 254 puts every premultiplied colour c * 254 * 257 / 255 = 255.996 c within 0.004 c of the
# boundary 256 c, where a type whose taps truncate (NRGBA, NRGBA64, a tRNS palette) is honestly undecided.
MAX_AMBIGUOUS_MIXED_ALPHA = 0.25


def cap(kind, alpha="random"):
    if alpha == "mixed":
        return MAX_AMBIGUOUS_MIXED_ALPHA
    return MAX_AMBIGUOUS["ycbcr" if kind.startswith("ycbcr") else kind]


def _alpha(rng, shape, alpha, top=255):
    if alpha == "opaque":
        return np.full(shape, top)
    if alpha == "zero":
        return np.zeros(shape, np.int64)
    if alpha == "mixed":                       # the extremes the premultiplication and the clamp turn on
        return np.choose(rng.integers(0, 4, shape), [0, 1, top - 1, top])
    return rng.integers(0, top + 1, shape)


class Source:
    """One source image: `ref` (scaler_reference.Taps), the oracle's scale / draw for its type, and the arguments the product's
    entries take (`data`)."""

    def __init__(self, kind, w, h, seed=1, alpha="random"):
        rng = np.random.default_rng(seed)
        self.kind, self.w, self.h = kind, w, h
        if kind in ("rgba", "nrgba"):
            px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            px[..., 3] = _alpha(rng, (h, w), alpha)
            if kind == "rgba":                # premultiplied, as an *image.RGBA holds it
                px[..., :3] = np.minimum(px[..., :3], px[..., 3:4])
                self.ref = R.rgba(px)
            else:
                self.ref = R.nrgba(px)
            self.data = px
        elif kind == "gray":
            self.data = rng.integers(0, 256, (h, w), dtype=np.uint8)
            self.ref = R.gray(self.data)
            self.rgba = np.dstack([self.data] * 3 + [np.full_like(self.data, 255)])    # the oracle's only route for Gray
        elif kind.startswith("ycbcr"):
            ratio = RATIO[kind]
            chh, cw = M411.chroma_size(ratio, w, h)[::-1] if ratio in RATIOS_41X else oracle.chroma_shape(w, h, ratio)
            self.data = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (chh, cw), dtype=np.uint8),
                         rng.integers(0, 256, (chh, cw), dtype=np.uint8), ratio)
            self.ref = R.ycbcr(*self.data)
            self.oracle_data = self.data     # what the oracle's 4:4:4 routine reads in place of a 4:1:x image
            if ratio in RATIOS_41X:
                y, cb, cr, _ = self.data
                self.oracle_data = (y, M411.upsample(cb, ratio, w, h), M411.upsample(cr, ratio, w, h), 0)
        elif kind.startswith("paletted"):
            pal = rng.integers(0, 256, (256, 4), dtype=np.uint8)
            if kind == "paletted-gif":        # opaque color.RGBA entries and a transparent index (the zero colour)
                pal[:, 3] = 255
                pal[7] = 0
                entry = "rgba"
            else:                             # a PNG palette with tRNS: color.NRGBA entries
                pal[:, 3] = _alpha(rng, 256, alpha)
                entry = "nrgba"
            idx = rng.integers(0, 256, (h, w), dtype=np.uint8)
            idx[h // 3: h // 2, w // 4: w // 2] = 7   # a flat area, as palette images have
            self.data = (idx, pal)
            self.pal16 = oracle.palette16(pal, entry)
            self.ref = R.paletted(idx, pal, entry)
        else:
            dk = DEEP[kind]
            if kind == "gray16":
                v = rng.integers(0, 65536, (h, w), dtype=np.uint16)
                self.ref = R.gray16(v)
            elif kind == "cmyk":
                v = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
                self.ref = R.cmyk(v)
            else:
                v = rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
                v[..., 3] = _alpha(rng, (h, w), alpha, 0xffff)
                if kind == "rgba64":
                    v[..., :3] = np.minimum(v[..., :3], v[..., 3:4])
                    self.ref = R.rgba64(v)
                else:
                    self.ref = R.nrgba64(v)
            self.data = oracle.deep_pix(v, dk)

    # ---- the oracle --------------------------------------------------------------------------------------------------------
    def oracle_scale(self, dw, dh, sr=None, op=oracle.OP_OVER, dst=None):
        k = self.kind
        dst = None if dst is None else dst.copy()
        if k == "rgba":
            return oracle.scale_bilinear(self.data, dw, dh, sr=sr, op=op, dst=dst)
        if k == "nrgba":
            return oracle.scale_bilinear_nrgba(self.data, dw, dh, sr=sr, op=op, dst=dst)
        if k == "gray":
            return oracle.scale_bilinear(self.rgba, dw, dh, sr=sr, op=op, dst=dst)
        if k.startswith("ycbcr"):
            return oracle.scale_bilinear_ycbcr(*self.oracle_data, dw, dh, sr=sr, dst=dst)
        if k.startswith("paletted"):
            return oracle.scale_bilinear_paletted(self.data[0], self.pal16, dw, dh, sr=sr, op=op, dst=dst)
        return oracle.scale_bilinear_deep(self.data, DEEP[k], dw, dh, sr=sr, op=op, dst=dst)

    def oracle_draw(self, dst, r, sp=(0, 0), op=oracle.OP_SRC):
        k = self.kind
        dst = dst.copy()
        if k == "rgba":
            return oracle.draw(dst, r, self.data, sp, op)
        if k == "nrgba":
            return oracle.draw_nrgba(dst, r, self.data, sp, op)
        if k == "gray":
            return oracle.draw(dst, r, self.rgba, sp, op)
        if k.startswith("ycbcr"):
            return oracle.draw_ycbcr(dst, r, *self.oracle_data, sp)
        if k.startswith("paletted"):
            return oracle.draw_paletted(dst, r, self.data[0], self.pal16, sp, op)
        return oracle.draw_deep(dst, r, self.data, DEEP[k], sp, op)

    # ---- the three operators of one frame, as the reference's helpers apply them -----------------------------------------
    def oracle_ops(self, resize, thumb):
        """resize -> resizeImage; thumbnail -> cropAndResize (equal-size Scale of the crop, then resizeImage) or resizeImage;
        watermark without text -> draw.Draw(Src) onto a zeroed RGBA frame.  Also returns the crop's stage-1 bytes."""
        nw, nh = oracle.resize_dims(self.w, self.h, *resize)
        out = {"resize": self.oracle_scale(nw, nh)}
        crop, tw, th = oracle.thumb_geometry(self.w, self.h, *thumb)
        stage1 = None
        if thumb[1]:
            cs = crop[2] - crop[0]
            stage1 = self.oracle_scale(cs, cs, sr=crop)
            out["thumbnail"] = oracle.scale_bilinear(stage1, tw, th)
        else:
            out["thumbnail"] = self.oracle_scale(tw, th)
        out["watermark"] = self.oracle_draw(np.zeros((self.h, self.w, 4), np.uint8), (0, 0, self.w, self.h))
        return out, stage1

    def ref_ops(self, resize, thumb, stage1):
        nw, nh = oracle.resize_dims(self.w, self.h, *resize)
        out = {"resize": R.scale(self.ref, nw, nh)}
        crop, tw, th = oracle.thumb_geometry(self.w, self.h, *thumb)
        if thumb[1]:
            out["thumbnail"] = R.crop_thumbnail(self.ref, crop, tw, th, stage1)[0]
        else:
            out["thumbnail"] = R.scale(self.ref, tw, th)
        out["watermark"] = R.draw(np.zeros((self.h, self.w, 4), np.uint8), (0, 0, self.w, self.h), self.ref)
        return out


# Geometries (sw, sh, dw, dh, sr): the edges where a scaler goes wrong.
GEOMETRIES = [
    (1, 1, 1, 1, None),            # 1x1 source and output
    (1, 1, 5, 3, None),            # a single tap spread
    (1, 9, 5, 3, None),            # 1 x N
    (9, 1, 1, 1, None),            # N x 1 to 1 x 1
    (40, 1, 17, 3, None),
    (333, 251, 1, 1, None),        # every source pixel into one
    (61, 47, 61, 47, None),        # equal size: one tap of weight 1
    (40, 25, 64, 40, None),        # x1.6: dyadic weights, exact ties
    (25, 25, 128, 128, None),      # x5.12
    (3, 2, 300, 200, None),        # x100
    (8000, 40, 16, 40, None),      # 1000 horizontal taps
    (495, 37, 10, 37, None),       # nx + ny = 99 + 1 = 100: the float pass's last tap count
    (500, 37, 10, 37, None),       # nx + ny = 100 + 1 = 101: float64 throughout
    (333, 251, 100, 90, None),     # odd sizes
    (333, 251, 50, 50, (13, 7, 320, 240)),    # a sub-rectangle at odd x and y
    (97, 61, 31, 200, (1, 3, 96, 60)),
]
