"""The tail launch behind the one-pass kernel's float pass (ipx_ks_tail.hip): the exact pass over both outputs' lists and the text
of the watermark frames in ONE launch, after the float64 redo pass.  Every case runs twice, with IPX_KS_TAIL unset (the tail) and
IPX_KS_TAIL=0 (the sequence it replaces: two exact launches, the redo pass, the text launch), byte for byte against the oracle."""
import numpy as np
import pytest

import oracle
from helpers import DEFAULT_COL, rgba_frames, text_glyphs

pytestmark = pytest.mark.gpu

TAIL = pytest.mark.parametrize("tail", [None, "0"], ids=["tail", "IPX_KS_TAIL=0"])
KEYS = ("resize", "thumbnail", "watermark")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _env(monkeypatch, tail, **more):
    monkeypatch.delenv("IPX_KS_TAIL", raising=False)
    monkeypatch.delenv("IPX_KS_FIX_CAP", raising=False)
    if tail is not None:
        monkeypatch.setenv("IPX_KS_TAIL", tail)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def _same(got, want, keys, what):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


# ---- (a), (b): values on rounding boundaries, overlapping glyph boxes, lists that overflow --------------------------------------

_BOUNDARY = {}


def _boundary_pool():
    """The three 1080p frames of test_values_exactly_on_a_rounding_boundary (test_parity_gpu.py): two random ones -- an exact 2:1
    downscale puts hundreds of their values EXACTLY on a multiple of 256 -- and one whose every interior value sits there (period-2
    tiles that sum to 510), so that all its lists overflow and every item is redone in float64.  With the oracle's outputs."""
    if not _BOUNDARY:
        frames = rgba_frames(3, 1920, 1080, seed=0xB0DA)
        rng = np.random.default_rng(0xA11)
        for ch in range(3):
            a = rng.integers(100, 156, (540, 960)); b = rng.integers(100, 156, (540, 960)); c = rng.integers(100, 156, (540, 960))
            d = 510 - a - b - c
            tile = np.empty((1080, 1920), np.int64)
            tile[0::2, 0::2] = a[0, 0]; tile[0::2, 1::2] = b[0, 0]; tile[1::2, 0::2] = c[0, 0]; tile[1::2, 1::2] = d[0, 0]
            frames[2, :, :, ch] = tile.astype(np.uint8)
        glyphs = text_glyphs(1920, 1080)                       # 16 glyphs, neighbouring boxes overlap
        boxes = [g["dr"] for g in glyphs]
        assert len(glyphs) == 16 and any(boxes[i][2] > boxes[i + 1][0] for i in range(15))
        want = [oracle.process(frames[i], resize=(960, 540, False), thumb=(270, True), glyphs=glyphs, col=DEFAULT_COL) for i in range(3)]
        _BOUNDARY.update(frames=frames, glyphs=glyphs, want=want)
    return _BOUNDARY


@TAIL
@pytest.mark.parametrize("cap", [None, "64", "7"], ids=["full-lists", "cap64", "cap7"])
@pytest.mark.parametrize("n", [1, 3, 300])
def test_boundary_values_with_overlapping_text(ctx, monkeypatch, n, cap, tail):
    """cap64 / cap7 (IPX_KS_FIX_CAP): lists overflow, so the redo pass rewrites frames -- watermark rows included -- before the
    exact pixels and the text land."""
    pool = _boundary_pool()
    _env(monkeypatch, tail, **({"IPX_KS_FIX_CAP": cap} if cap else {}))
    gs = ctx.glyphset(pool["glyphs"], DEFAULT_COL)
    plan = ctx.plan(1920, 1080, resize=(960, 540, False), thumbnail=(270, True), watermark=gs)
    frames = pool["frames"][np.arange(n) % 3]
    got = plan.run_host(frames)
    for i in range(n):
        _same({k: got[k][i] for k in KEYS}, pool["want"][i % 3], KEYS, "frame %d of %d cap %s tail %s" % (i, n, cap, tail))
    plan.close()
    gs.close()


# ---- (c): one frame that is not opaque among opaque ones -------------------------------------------------------------------------

@TAIL
def test_one_translucent_frame_among_opaque_ones(ctx, monkeypatch, tail):
    _env(monkeypatch, tail)
    w, h, n = 1280, 720, 5
    frames = rgba_frames(n, w, h, seed=77)
    frames[2] = rgba_frames(1, w, h, seed=78, opaque=False)[0]
    glyphs = text_glyphs(w, h)
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(w, h, resize=(640, 360, False), thumbnail=(200, True), watermark=gs)
    got = plan.run_host(frames)
    for i in range(n):
        want = oracle.process(frames[i], resize=(640, 360, False), thumb=(200, True), glyphs=glyphs, col=DEFAULT_COL)
        _same({k: got[k][i] for k in KEYS}, want, KEYS, "frame %d" % i)
    plan.close()
    gs.close()


# ---- (d): where the text box lies ---------------------------------------------------------------------------------------------------

def _box_glyphs(x0, y0, n=5, mw=23, mh=31, seed=3):
    """n overlapping glyph boxes walking right from (x0, y0); they may leave the frame (DrawMask clips them)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = rng.integers(0, 256, (mh + i, mw), dtype=np.uint8)
        m[rng.random(m.shape) < 0.3] = 0
        m[rng.random(m.shape) > 0.8] = 255
        x = x0 + i * (mw - 2)
        out.append({"mask": m, "dr": (x, y0 + i, x + mw, y0 + i + mh + i), "mp": (0, 0)})
    return out


W, H = 640, 360
TEXT_BOXES = {
    "left-edge": (-9, 100), "top-edge": (200, -12), "right-edge": (W - 60, 150), "bottom-edge": (300, H - 20),
    "corner": (W - 30, H - 15), "x=1mod4": (101, 50), "x=2mod4": (102, 50), "x=3mod4": (103, 50), "x=0mod4": (104, 50),
}


@TAIL
@pytest.mark.parametrize("where", list(TEXT_BOXES))
def test_text_box_positions(ctx, monkeypatch, where, tail):
    _env(monkeypatch, tail)
    x0, y0 = TEXT_BOXES[where]
    glyphs = _box_glyphs(x0, y0)
    frames = rgba_frames(3, W, H, seed=len(where) + x0)
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(W, H, resize=(320, 180, False), thumbnail=(90, True), watermark=gs)
    got = plan.run_host(frames)
    for i in range(3):
        want = oracle.process(frames[i], resize=(320, 180, False), thumb=(90, True), glyphs=glyphs, col=DEFAULT_COL)
        _same({k: got[k][i] for k in KEYS}, want, KEYS, "%s frame %d" % (where, i))
        assert not np.array_equal(want["watermark"], frames[i]), "the case draws no text"
    plan.close()
    gs.close()


@TAIL
@pytest.mark.parametrize("wm", ["no-glyphs", "no-watermark"])
def test_tail_without_text(ctx, monkeypatch, wm, tail):
    """An empty glyph list (the watermark output is draw.Draw's copy) and a plan without the watermark output: exact part only."""
    _env(monkeypatch, tail)
    frames = rgba_frames(3, W, H, seed=11)
    plan = ctx.plan(W, H, resize=(320, 180, False), thumbnail=(90, True), watermark=True if wm == "no-glyphs" else None)
    keys = KEYS if wm == "no-glyphs" else KEYS[:2]
    got = plan.run_host(frames, want=keys)
    for i in range(3):
        want = oracle.process(frames[i], resize=(320, 180, False), thumb=(90, True), glyphs=(), col=DEFAULT_COL, want=keys)
        _same({k: got[k][i] for k in keys}, want, keys, "%s frame %d" % (wm, i))
    plan.close()


# ---- (e): the ends of the row and of the frame -----------------------------------------------------------------------------------

@TAIL
@pytest.mark.parametrize("nrgba", [False, True], ids=["rgba", "nrgba"])
def test_listed_pixels_in_the_last_column_and_row(ctx, monkeypatch, nrgba, tail):
    """854 x 480 (a width that is no multiple of 4) to 427 x 240, exactly 2:1.  Frame 0 ends in three columns, frame 1 (the last of
    the batch) in three rows, whose values alternate between 127 and 128 along the other axis.  Along that axis an interior
    destination index weighs its four taps (1, 3, 3, 1) / 8, so every such tap sum is 127.5; across it the last index has three
    taps whose weights sum to 1 whatever they are.  The value is 257 * 127.5 = 32767.5: + 0.5 is 128 * 256 exactly, which no float
    sum can decide -- the pixels of the last column (frame 0) and the last row (frame 1) are on their frame's lists, and the exact
    pass reads the taps at the very end of a source row and of the last frame."""
    _env(monkeypatch, tail)
    sw, sh, dw, dh = 854, 480, 427, 240
    frames = rgba_frames(2, sw, sh, seed=0xE0F)
    period = np.array([127, 128], np.uint8)
    frames[0, :, sw - 3:, :3] = period[np.arange(sh) % 2][:, None, None]
    frames[1, sh - 3:, :, :3] = period[np.arange(sw) % 2][None, :, None]
    # (integer arithmetic: the last column's taps weigh (1, 3, 3) x (1, 3, 3, 1), total 56)
    col = frames[0, :, sw - 3:, 0].astype(np.int64)
    for dy in (1, 100, dh - 2):
        s = int((np.array([1, 3, 3, 1])[:, None] * np.array([1, 3, 3])[None, :] * col[2 * dy - 1:2 * dy + 3]).sum())
        assert (514 * s + 56) % (112 * 256) == 0, (dy, s)
    glyphs = text_glyphs(sw, sh, n=6, width_px=150, height_px=30)
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(sw, sh, resize=(dw, dh, False), thumbnail=(120, True), watermark=gs)
    if nrgba:   # alpha 255: the same values through scaleX_NRGBA
        got = plan.run_host_nrgba(frames)
    else:
        got = plan.run_host(frames)
    crop, tw, th = oracle.thumb_geometry(sw, sh, 120, True)
    for i in range(2):
        if nrgba:
            cs = crop[2] - crop[0]
            want = {"resize": oracle.scale_bilinear_nrgba(frames[i], dw, dh),
                    "thumbnail": oracle.scale_bilinear(oracle.scale_bilinear_nrgba(frames[i], cs, cs, sr=crop), tw, th),
                    "watermark": oracle.composite_glyphs(oracle.draw_nrgba(np.zeros((sh, sw, 4), np.uint8), (0, 0, sw, sh), frames[i]), glyphs, DEFAULT_COL)}
        else:
            want = oracle.process(frames[i], resize=(dw, dh, False), thumb=(120, True), glyphs=glyphs, col=DEFAULT_COL)
        _same({k: got[k][i] for k in KEYS}, want, KEYS, "frame %d" % i)
    plan.close()
    gs.close()


# ---- (f): the other source types ----------------------------------------------------------------------------------------------------

SW, SH, RESIZE, THUMB = 640, 480, (320, 240, False), (120, True)


def _text(ctx):
    glyphs = text_glyphs(SW, SH, n=16, width_px=280, height_px=40)
    return glyphs, ctx.glyphset(glyphs, DEFAULT_COL)


@TAIL
def test_ycbcr_420_batch_with_text(ctx, monkeypatch, tail):
    _env(monkeypatch, tail)
    n, ratio = 3, oracle.RATIO_420
    rng = np.random.default_rng(420)
    ch, cw = oracle.chroma_shape(SW, SH, ratio)
    y = rng.integers(0, 256, (n, SH, SW), dtype=np.uint8)
    cb = rng.integers(0, 256, (n, ch, cw), dtype=np.uint8)
    cr = rng.integers(0, 256, (n, ch, cw), dtype=np.uint8)
    glyphs, gs = _text(ctx)
    plan = ctx.plan(SW, SH, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    got = plan.run_host_ycbcr(y, cb, cr, ratio)
    crop, tw, th = oracle.thumb_geometry(SW, SH, *THUMB)
    cs = crop[2] - crop[0]
    for i in range(n):
        want = {"resize": oracle.scale_bilinear_ycbcr(y[i], cb[i], cr[i], ratio, RESIZE[0], RESIZE[1]),
                "thumbnail": oracle.scale_bilinear(oracle.scale_bilinear_ycbcr(y[i], cb[i], cr[i], ratio, cs, cs, sr=crop), tw, th),
                "watermark": oracle.composite_glyphs(oracle.draw_ycbcr(np.zeros((SH, SW, 4), np.uint8), (0, 0, SW, SH), y[i], cb[i], cr[i], ratio),
                                                     glyphs, DEFAULT_COL)}
        _same({k: got[k][i] for k in KEYS}, want, KEYS, "frame %d" % i)
    plan.close()
    gs.close()


@TAIL
def test_gray_batch_with_text(ctx, monkeypatch, tail):
    _env(monkeypatch, tail)
    n = 3
    gray = np.random.default_rng(8).integers(0, 256, (n, SH, SW), dtype=np.uint8)
    glyphs, gs = _text(ctx)
    plan = ctx.plan(SW, SH, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    got = plan.run_host_gray(gray)
    for i in range(n):
        rgba = np.dstack([gray[i]] * 3 + [np.full_like(gray[i], 255)])
        want = oracle.process(rgba, resize=RESIZE, thumb=THUMB, glyphs=glyphs, col=DEFAULT_COL)
        _same({k: got[k][i] for k in KEYS}, want, KEYS, "frame %d" % i)
    plan.close()
    gs.close()


@TAIL
def test_nrgba_batch_with_text(ctx, monkeypatch, tail):
    _env(monkeypatch, tail)
    n = 3
    nrgba = np.random.default_rng(9).integers(0, 256, (n, SH, SW, 4), dtype=np.uint8)
    nrgba[1, ..., 3] = 255
    glyphs, gs = _text(ctx)
    plan = ctx.plan(SW, SH, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    got = plan.run_host_nrgba(nrgba)
    crop, tw, th = oracle.thumb_geometry(SW, SH, *THUMB)
    cs = crop[2] - crop[0]
    for i in range(n):
        want = {"resize": oracle.scale_bilinear_nrgba(nrgba[i], RESIZE[0], RESIZE[1]),
                "thumbnail": oracle.scale_bilinear(oracle.scale_bilinear_nrgba(nrgba[i], cs, cs, sr=crop), tw, th),
                "watermark": oracle.composite_glyphs(oracle.draw_nrgba(np.zeros((SH, SW, 4), np.uint8), (0, 0, SW, SH), nrgba[i]), glyphs, DEFAULT_COL)}
        _same({k: got[k][i] for k in KEYS}, want, KEYS, "frame %d" % i)
    plan.close()
    gs.close()


# ---- the tail is what runs by default -----------------------------------------------------------------------------------------------

@TAIL
def test_stats_report_under_either_sequence(ctx, monkeypatch, capfd, tail):
    """IPX_KS_STATS=1 keeps reporting the float pass's lists whichever sequence follows it."""
    _env(monkeypatch, tail, IPX_KS_STATS="1")
    frames = rgba_frames(2, 1280, 720, seed=5)
    plan = ctx.plan(1280, 720, resize=(1024, 768, True), thumbnail=(200, True), watermark=None)
    plan.run_host(frames)
    assert "frames: undecided pixels per frame resize mean" in capfd.readouterr().err   # (one report per lane's share of the batch)
    plan.close()
