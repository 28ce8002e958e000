"""The *image.YCbCr operators on planes of ratio 4:1:1 and 4:1:0 (IPX_YCBCR_411 / _410; caller-supplied planes, so no switch):
ipx_scale_bilinear_ycbcr, ipx_draw_ycbcr and ipx_plan_run_dev_ycbcr (resize + crop thumbnail + watermark copy).

x/image/draw has specialised loops only for 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0; every other ratio goes through src.At(x, y).RGBA(), that is
color.YCbCr.RGBA() -- the same integer conversion -- with the chroma sample at (x / 4, y or y / 2).  So the
existing oracle run at 4:4:4 on chroma planes whose samples are replicated 4 x across (and 2 x down for 4:1:0) gives the expected
bytes, and every comparison here is byte for byte.

Widths 37 .. 40 (every x mod 4 at the right edge; 40 is the one the one-pass kernel takes, a row of whole four-pixel chunks), odd and
even heights; 47 x 20, whose crop thumbnail starts at x = 13; 4036 x 40, which the planner cuts into two strips.  Which kernel ran is
asserted from the library's IPX_KS_DEBUG line.  On a library without the feature every call is refused (IPX_ERR_INVALID)."""
import numpy as np
import pytest

import jpeg_411_model as model
import oracle
from helpers import DEFAULT_COL, text_glyphs
from test_sources_gpu import _expect_ycbcr_ops

pytestmark = pytest.mark.gpu

RATIOS = [model.RATIO_411, model.RATIO_410]
SMALL = [(37, 21), (38, 22), (39, 21), (40, 22), (40, 21)]
KEYS = ("resize", "thumbnail", "watermark")
KS_KNOBS = ("IPX_FUSED", "IPX_KS_FAST", "IPX_KS_STRIPS", "IPX_KS_SPLIT", "IPX_KS_SPLIT_ROWS", "IPX_KS_FIX_CAP", "IPX_NO_FUSE")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


def planes(w, h, ratio, seed):
    """random planes of image.NewYCbCr(Rect(0, 0, w, h), ratio), and the 4:4:4 planes At(x, y) reads from them"""
    rng = np.random.default_rng(seed)
    cw, ch = model.chroma_size(ratio, w, h)
    y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))
    return (y, cb, cr), (y, model.upsample(cb, ratio, w, h), model.upsample(cr, ratio, w, h))


def one_pass_lines(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith("[ipx ks] src")]


@pytest.mark.parametrize("ratio", RATIOS, ids=["411", "410"])
@pytest.mark.parametrize("w,h", SMALL + [(47, 20)])
def test_scale_and_draw(ctx, ratio, w, h):
    src, full = planes(w, h, ratio, 10 * w + h + ratio)
    for dw, dh, sr in ((23, 13, None), (w, h, None), (61, 40, None), (16, 11, (5, 3, w - 2, h - 1)), (9, 9, (13, 2, 31, 20))):
        np.testing.assert_array_equal(ctx.scale_bilinear_ycbcr(*src, ratio, dw, dh, sr=sr), oracle.scale_bilinear_ycbcr(*full, 0, dw, dh, sr=sr),
                                      err_msg="scale to %dx%d from %r" % (dw, dh, sr))
    # the thumbnail's crop copy: a Scale of equal size is DrawYCbCr from an origin that is no multiple of 4
    side = min(w, h)
    crop = ((w - side) // 2, (h - side) // 2, (w - side) // 2 + side, (h - side) // 2 + side)
    np.testing.assert_array_equal(ctx.scale_bilinear_ycbcr(*src, ratio, side, side, sr=crop), oracle.scale_bilinear_ycbcr(*full, 0, side, side, sr=crop))
    for r, sp in (((0, 0, w, h), (0, 0)), ((3, 2, w, h), (1, 1)), ((0, 0, 20, 10), (13, 7)), ((5, 5, 200, 200), (2, 3))):
        d0 = np.full((h + 3, w + 5, 4), 17, np.uint8)
        np.testing.assert_array_equal(ctx.draw_ycbcr(d0.copy(), r, *src, ratio, sp), oracle.draw_ycbcr(d0.copy(), r, *full, 0, sp), err_msg="draw %r from %r" % (r, sp))


def run_dev(ctx, plan, batch, ratio, w, h):
    """tight planes of n frames up, ipx_plan_run_dev_ycbcr, the three outputs down"""
    n = len(batch)
    y, cb, cr = (np.stack([b[k] for b in batch]) for k in range(3))
    cw, ch = model.chroma_size(ratio, w, h)
    i_ = plan.info
    bufs = [ctx.alloc(a.nbytes).upload(a) for a in (y, cb, cr)]
    outs = [ctx.alloc(n * i_.resize_bytes), ctx.alloc(n * i_.thumb_bytes), ctx.alloc(n * i_.wm_bytes)]
    plan.run_dev_ycbcr(n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, ratio, w, cw, w * h, cw * ch, outs[0].ptr, outs[1].ptr, outs[2].ptr)
    ctx.sync()
    got = {"resize": outs[0].download((n, i_.resize_h, i_.resize_w, 4)), "thumbnail": outs[1].download((n, i_.thumb_h, i_.thumb_w, 4)),
           "watermark": outs[2].download((n, h, w, 4))}
    for b in bufs + outs:
        b.free()
    return got


def plan_case(ctx, monkeypatch, capfd, ratio, w, h, resize, thumb, n, env=None):
    for k in KS_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("IPX_KS_DEBUG", "1")
    pairs = [planes(w, h, ratio, 100 * w + h + 7 * i + ratio) for i in range(n)]
    glyphs = text_glyphs(w, h, n=4, width_px=min(30, w), height_px=min(12, h))
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(w, h, resize=resize, thumbnail=thumb, watermark=gs)
    try:
        capfd.readouterr()
        got = run_dev(ctx, plan, [p[0] for p in pairs], ratio, w, h)
        lines = one_pass_lines(capfd)
    finally:
        plan.close()
        gs.close()
    for i, (_, full) in enumerate(pairs):
        want = _expect_ycbcr_ops(*full, 0, resize, thumb, glyphs, DEFAULT_COL)
        for k in KEYS:
            np.testing.assert_array_equal(got[k][i], want[k], err_msg="%s of frame %d (%dx%d ratio %d %r)" % (k, i, w, h, ratio, env))
    return lines


@pytest.mark.parametrize("ratio", RATIOS, ids=["411", "410"])
@pytest.mark.parametrize("w,h", SMALL + [(47, 20)])
def test_plan_on_device_planes(ctx, monkeypatch, capfd, ratio, w, h):
    """resize + crop thumbnail (47 x 20: the crop starts at x = 13) + watermark copy.  Rows of whole four-pixel chunks (w % 4 == 0) run on
    the one-pass kernel -- with the float pass, without it, and with lists every frame overflows --, ragged rows on the per-output kernels
    (launch_ks_fused's gate for planar sources)"""
    resize, thumb = (23, 13, False), (10, True)
    if w == 47:
        from oracle import thumb_geometry
        assert thumb_geometry(w, h, *thumb)[0][0] == 13
    for env in ({}, {"IPX_KS_FAST": "0"}, {"IPX_KS_FIX_CAP": "9"}):
        lines = plan_case(ctx, monkeypatch, capfd, ratio, w, h, resize, thumb, 3, env)
        assert bool(lines) == (w % 4 == 0), "%dx%d: the one-pass kernel %s" % (w, h, "should have run" if w % 4 == 0 else "should not have run")
    assert not plan_case(ctx, monkeypatch, capfd, ratio, w, h, resize, thumb, 2, {"IPX_FUSED": "0"})


@pytest.mark.parametrize("ratio", RATIOS, ids=["411", "410"])
@pytest.mark.parametrize("env", [{}, {"IPX_KS_STRIPS": "3", "IPX_KS_SPLIT": "1", "IPX_KS_SPLIT_ROWS": "23"}], ids=["natural", "three-strips-split"])
def test_a_frame_of_several_strips(ctx, monkeypatch, capfd, ratio, env):
    """4036 x 40: the planner cuts it into two strips by itself (tests/tiling_cases.py JPEG_CASE); the second strip's tile starts below
    its own columns, at a multiple of 4 -- the chroma column of a chunk is x / 4 of the chunk's first pixel.  The crop thumbnail starts
    at x = 1998."""
    lines = plan_case(ctx, monkeypatch, capfd, ratio, 4036, 40, (1024, 40, False), (16, True), 2, env)
    assert lines, "the one-pass kernel did not take the batch"
    strips = [int(l.split(" strips ")[1].split()[0]) for l in lines]
    assert all(s >= (3 if env else 2) for s in strips), lines


def test_other_ratios_are_still_refused(ctx):
    """IPX_GRAY (4) has entries of its own, and nothing above IPX_YCBCR_410 names a ratio"""
    (y, cb, cr), _ = planes(40, 22, model.RATIO_411, 1)
    for ratio in (4, 7, -1):
        with pytest.raises(Exception):
            ctx.scale_bilinear_ycbcr(y, cb, cr, ratio, 20, 11)
