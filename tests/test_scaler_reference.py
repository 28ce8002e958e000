"""CPU: the oracle's scaler and colour conversions against an independent float64 reference (tests/scaler_reference.py).

The oracle restates x/image's Kernel.Scale and Go's colour conversions in integer and float64 C; the reference builds every tap from
the colour model's definition in real numbers and interpolates with torch's antialiased bilinear.  Every byte whose exact value is
clear of a rounding boundary (by more than the integer code's error bound) must be equal; the rest may differ by 1.  The
sensitivity tests at the end feed deliberately wrong outputs through the same check and require it to reject each one."""
import numpy as np
import pytest

import oracle
import scaler_reference as R
from scaler_cases import ALPHA_KINDS, GEOMETRIES, KINDS, Source, cap

SEEN = {}


def _check(got, ref, kind, what, alpha="random"):
    share = R.assert_matches(got, *ref, max_ambiguous=cap(kind, alpha), what="%s %s" % (kind, what))
    key = kind if alpha != "mixed" else kind + "/mixed"
    if np.asarray(got).size >= 1000:                   # (the cap allows one pixel more: the tiniest outputs are not counted here)
        SEEN[key] = max(SEEN.get(key, 0.0), share)
    return share


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "%dx%d-%dx%d%s" % (g[0], g[1], g[2], g[3], "-sr" if g[4] else ""))
def test_scale_against_reference(kind, geom):
    sw, sh, dw, dh, sr = geom
    src = Source(kind, sw, sh, seed=sw * 7 + sh)
    _check(src.oracle_scale(dw, dh, sr=sr), R.scale(src.ref, dw, dh, sr=sr), kind, "scale %r" % (geom,))
    # Src, and Over onto a destination that already holds pixels
    under = np.random.default_rng(dw).integers(0, 256, (dh, dw, 4), dtype=np.uint8)
    under[..., :3] = np.minimum(under[..., :3], under[..., 3:4])
    for op in (oracle.OP_SRC, oracle.OP_OVER):
        if kind.startswith("ycbcr") and op == oracle.OP_SRC:
            continue                                    # the oracle's YCbCr entry has no op: a YCbCr image is opaque
        _check(src.oracle_scale(dw, dh, sr=sr, op=op, dst=under), R.scale(src.ref, dw, dh, sr=sr, op=op, dst=under), kind,
               "scale op %d onto pixels %r" % (op, geom))


@pytest.mark.parametrize("kind", ALPHA_KINDS)
@pytest.mark.parametrize("alpha", ["zero", "opaque", "mixed", "random"])
def test_alpha_extremes(kind, alpha):
    """alpha all 0, all 255, only {0, 1, 254, 255}, and any: premultiplication, the clamp of colour to alpha, Opaque()."""
    src = Source(kind, 83, 61, seed=5, alpha=alpha)
    under = np.random.default_rng(2).integers(0, 256, (40, 50, 4), dtype=np.uint8)
    for dw, dh, sr in ((50, 40, None), (83, 61, None), (131, 97, (3, 1, 80, 60)), (1, 1, None)):
        d = np.ascontiguousarray(np.resize(under, (dh, dw, 4)))
        for op in (oracle.OP_SRC, oracle.OP_OVER):
            _check(src.oracle_scale(dw, dh, sr=sr, op=op, dst=d), R.scale(src.ref, dw, dh, sr=sr, op=op, dst=d), kind,
                   "alpha %s %dx%d op %d" % (alpha, dw, dh, op), alpha)
        for op in (oracle.OP_SRC, oracle.OP_OVER):
            _check(src.oracle_draw(under, (3, 5, 49, 40), (7, 9), op), R.draw(under, (3, 5, 49, 40), src.ref, (7, 9), op), kind,
                   "draw alpha %s op %d" % (alpha, op), alpha)


@pytest.mark.parametrize("kind", KINDS)
def test_draw_against_reference(kind):
    """draw.Draw's 8-bit conversions (the watermark's copy): the whole frame, a clipped rectangle at an odd source point, Over."""
    src = Source(kind, 157, 93, seed=11)
    zeros = np.zeros((93, 157, 4), np.uint8)
    _check(src.oracle_draw(zeros, (0, 0, 157, 93)), R.draw(zeros, (0, 0, 157, 93), src.ref), kind, "draw")
    under = np.random.default_rng(4).integers(0, 256, (64, 80, 4), dtype=np.uint8)
    under[..., :3] = np.minimum(under[..., :3], under[..., 3:4])
    for op in (oracle.OP_SRC, oracle.OP_OVER):
        for r, sp in (((5, 7, 75, 60), (3, 1)), ((-4, -3, 200, 200), (9, 13)), ((70, 50, 90, 90), (150, 90))):
            _check(src.oracle_draw(under, r, sp, op), R.draw(under, r, src.ref, sp, op), kind, "draw %r %r op %d" % (r, sp, op))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(333, 251, (200, 100, False), (64, True)),       # crop origin (41, 0)
                                  (251, 333, (1024, 768, True), (64, True)),       # crop origin (0, 41), an upscale
                                  (97, 61, (155, 97, False), (40, False)),         # x1.6 and a non-crop thumbnail
                                  (4000, 41, (8, 41, False), (20, True))],         # 500 taps, and a crop of 41 from 4000
                         ids=lambda c: "%dx%d" % (c[0], c[1]))
def test_three_operators(kind, case):
    """resizeImage, cropAndResize in two stages (the crop's equal-size Scale, then resizeImage of its RGBA bytes) and the
    watermark's draw.Draw(Src), each from the original frame."""
    w, h, resize, thumb = case
    src = Source(kind, w, h, seed=w + h)
    want, stage1 = src.oracle_ops(resize, thumb)
    ref = src.ref_ops(resize, thumb, stage1)
    for k in ("resize", "thumbnail", "watermark"):
        _check(want[k], ref[k], kind, "%s %r" % (k, case))


def test_oracle_process_matches_reference():
    """oracle.process, the pipeline entry bench.py and smoke() check against, for an RGBA frame (opaque and translucent)."""
    for opaque in (True, False):
        src = Source("rgba", 640, 480, seed=3, alpha="opaque" if opaque else "random")
        for resize, thumb in (((1024, 768, True), (200, True)), ((300, 300, False), (100, False))):
            got = oracle.process(src.data, resize=resize, thumb=thumb)
            _, stage1 = src.oracle_ops(resize, thumb)
            ref = src.ref_ops(resize, thumb, stage1)
            for k in ("resize", "thumbnail", "watermark"):
                _check(got[k], ref[k], "rgba", "process %s" % k)


def test_headline_geometry():
    """1920x1080 -> 1024x768, the bench frame: no ambiguous byte at all is expected on an opaque frame."""
    src = Source("rgba", 1920, 1080, seed=9, alpha="opaque")
    assert _check(src.oracle_scale(1024, 768), R.scale(src.ref, 1024, 768), "rgba", "1080p") < 1e-4


# ---- the check is not empty: deliberately wrong outputs are rejected ------------------------------------------------------------

def _rejects(got, ref, kind="rgba"):
    with pytest.raises(AssertionError, match="clear of a rounding boundary differ"):
        R.assert_matches(got, *ref, max_ambiguous=cap(kind))


def test_rejects_two_tap_approx_bilinear():
    """x/image's ApproxBiLinear: 2 x 2 taps around the scaled centre, what rounds 1-2 of this project computed."""
    src = Source("rgba", 270, 270, seed=1, alpha="opaque")
    f = src.data.astype(np.float64)
    s = (np.arange(50) + 0.5) * 5.4 - 0.5
    i0 = np.clip(np.floor(s).astype(int), 0, 268)
    fr = (s - i0)
    wy, wx = fr[:, None, None], fr[None, :, None]
    two = ((f[i0][:, i0] * (1 - wx) + f[i0][:, i0 + 1] * wx) * (1 - wy) + (f[i0 + 1][:, i0] * (1 - wx) + f[i0 + 1][:, i0 + 1] * wx) * wy)
    _rejects(np.clip(np.floor(two + 0.5), 0, 255).astype(np.uint8), R.scale(src.ref, 50, 50))


@pytest.mark.parametrize("ratio", [1, 2, 3], ids=["422", "420", "440"])
def test_rejects_chroma_shifted_by_one(ratio):
    """A kernel that reads the chroma sample one to the right (or below, for 4:4:0) of (x >> hs, y >> vs)."""
    src = Source("ycbcr" + ["444", "422", "420", "440"][ratio], 333, 251, seed=2)
    y, cb, cr, _ = src.data
    ax = 0 if ratio == 3 else 1
    shifted = (y, np.roll(cb, -1, axis=ax), np.roll(cr, -1, axis=ax), ratio)
    _rejects(oracle.scale_bilinear_ycbcr(*shifted, 100, 90), R.scale(src.ref, 100, 90), "ycbcr")
    z = np.zeros((251, 333, 4), np.uint8)
    _rejects(oracle.draw_ycbcr(z.copy(), (0, 0, 333, 251), *shifted), R.draw(z, (0, 0, 333, 251), src.ref), "ycbcr")


def test_rejects_0x100_widening():
    """Taps widened by << 8 instead of * 0x101 (an RGBA64 frame of c << 8 goes through the oracle's generic routine)."""
    src = Source("rgba", 320, 200, seed=4, alpha="opaque")
    wrong = oracle.scale_bilinear_deep(oracle.deep_pix(src.data.astype(np.uint16) << 8, oracle.DEEP_RGBA64), oracle.DEEP_RGBA64, 200, 120)
    _rejects(wrong, R.scale(src.ref, 200, 120))


def test_rejects_nrgba_taps_not_premultiplied():
    """Straight-alpha pixels weighted as they are (the RGBA routine on NRGBA data), for a frame whose alpha is mostly high:
    the colour clamp hides the error at alpha 0, not at 254."""
    src = Source("nrgba", 320, 200, seed=6, alpha="random")
    src.data[..., 3] = np.maximum(src.data[..., 3], 200)
    src.ref = R.nrgba(src.data)
    _rejects(oracle.scale_bilinear(src.data, 200, 120), R.scale(src.ref, 200, 120), "nrgba")


def test_rejects_one_flipped_byte():
    src = Source("nrgba", 97, 61, seed=7)
    ref = R.scale(src.ref, 31, 20)
    got = src.oracle_scale(31, 20)
    R.assert_matches(got, *ref, max_ambiguous=cap("nrgba"))
    clear = np.argwhere(~R.ambiguous(ref.margin, ref.tol) & (ref.byte < 255))
    y, x, c = clear[len(clear) // 2]
    got[y, x, c] += 1
    with pytest.raises(AssertionError, match=r"1 of \d+ bytes clear"):
        R.assert_matches(got, *ref, max_ambiguous=cap("nrgba"))


def test_rejects_far_bytes_and_empty_checks():
    """A byte off by 2 where the value is ambiguous is rejected too, and so is a check whose bytes are mostly ambiguous."""
    ref = R.Ref(np.array([10, 20], np.uint8), np.array([0.1, 0.1]), 0.5)
    with pytest.raises(AssertionError, match="by more than 1"):
        R.assert_matches(np.array([12, 20], np.uint8), *ref, max_ambiguous=1.0)
    many = R.Ref(np.full(100, 10, np.uint8), np.full(100, 0.1), 0.5)
    with pytest.raises(AssertionError, match="above the cap"):
        R.assert_matches(np.full(100, 10, np.uint8), *many, max_ambiguous=0.5)


def test_zz_report_ambiguous_shares():
    """(runs last in this file) the largest ambiguous share seen per source type, beside its cap -- printed with -s"""
    for k in sorted(SEEN):
        print("ambiguous %-22s %.4f (cap %.3f)" % (k, SEEN[k], cap(k.split("/")[0], "mixed" if "/" in k else "random")))
