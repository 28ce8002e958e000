"""gif.Encode on the GPU (csrc/ipx_gif.hip): the Plan 9 / Floyd-Steinberg dither, LZW and the four entries, byte for byte against
tests/gif_model.py (the restatement of Go's image/gif writer), and every stream decoded by Pillow.  PARITY UNPINNED against Go itself."""
import io

import numpy as np
import pytest

import gif_model as gm
from helpers import DEFAULT_COL, rgba_frames, text_glyphs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _frame(w, h, seed, alpha=False):
    """premultiplied RGBA: noise over gradients and flat patches (LZW finds runs), alpha < 255 in places when asked"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 4), np.int64)
    f[..., 0] = xx * 255 // max(w - 1, 1)
    f[..., 1] = yy * 255 // max(h - 1, 1)
    f[..., 2] = (xx + yy) * 3 % 256
    f[..., :3] += rng.integers(-40, 41, (h, w, 3))
    f[h // 3:h // 2, w // 4:w // 2, :3] = 90
    f[..., 3] = 255
    if alpha:
        f[..., 3] = np.where(rng.random((h, w)) < 0.4, rng.integers(0, 256, (h, w)), 255)
        f[: h // 4, : w // 4, 3] = 0
    f = f.clip(0, 255)
    f[..., :3] = f[..., :3] * f[..., 3:4] // 255
    return f.astype(np.uint8)


def _decode(stream):
    from PIL import Image
    im = Image.open(io.BytesIO(stream))
    assert im.format == "GIF" and im.mode == "P"
    pal = np.array(im.getpalette()[:768], np.uint8).reshape(256, 3)
    np.testing.assert_array_equal(pal, gm.PLAN9)
    return np.array(im)


SHAPES = [(1, 1), (1, 300), (300, 1), (127, 5), (200, 200), (97, 131), (1024, 768)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_dither_dev_is_the_model(ctx, w, h):
    frames = np.stack([_frame(w, h, 1, alpha=False), _frame(w, h, 2, alpha=True)])
    n = frames.shape[0]
    src = ctx.alloc(frames.nbytes).upload(frames)
    idx = ctx.alloc(n * w * h)
    ctx.gif_dither_dev(src.ptr, w, h, n, idx.ptr)
    ctx.sync()
    got = idx.download((n, h, w))
    for k in range(n):
        np.testing.assert_array_equal(got[k], gm.dither_wavefront(frames[k]), err_msg="%dx%d frame %d" % (w, h, k))


@pytest.mark.parametrize("waves", ["1", "2", "3", "16"])
def test_dither_rows_in_flight(ctx, monkeypatch, waves):
    """one wave per frame hands error rows from band to band through global scratch, more waves through LDS at wave boundaries:
    every choice gives the same indices (strided source rows, padded frames)"""
    monkeypatch.setenv("IPX_GIF_WAVES", waves)
    w, h, n = 150, 333, 2
    stride, fs = w * 4 + 12, (w * 4 + 12) * h + 64
    frames = np.stack([_frame(w, h, 5), _frame(w, h, 6, alpha=True)])
    buf = np.zeros(n * fs, np.uint8)
    for k in range(n):
        v = buf[k * fs:k * fs + stride * h].reshape(h, stride)
        v[:, :w * 4] = frames[k].reshape(h, w * 4)
    src = ctx.alloc(buf.nbytes).upload(buf)
    idx = ctx.alloc(n * w * h)
    ctx.gif_dither_dev(src.ptr, w, h, n, idx.ptr, stride=stride, frame_stride=fs)
    ctx.sync()
    got = idx.download((n, h, w))
    for k in range(n):
        np.testing.assert_array_equal(got[k], gm.dither_wavefront(frames[k]), err_msg="waves %s frame %d" % (waves, k))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (127, 5), (200, 200), (97, 131)])
def test_single_frame_stream_is_the_model(ctx, w, h):
    f = _frame(w, h, 9, alpha=True)
    s = ctx.gif_encode(f)
    want_idx = gm.dither_wavefront(f)
    assert s == gm.encode_index(want_idx)
    np.testing.assert_array_equal(_decode(s), want_idx)


def test_large_frame_stream(ctx):
    """1024 x 768 through both host-facing entries: several LZW clear codes, thousands of sub-blocks"""
    f = _frame(1024, 768, 11)
    want = gm.encode(f)
    assert ctx.gif_encode(f) == want
    src = ctx.alloc(f.nbytes).upload(f)
    assert ctx.gif_encode_batch_dev(src.ptr, 1024, 768, 1) == [want]
    np.testing.assert_array_equal(_decode(want), gm.dither_wavefront(f))


def test_batch_of_mixed_frames(ctx):
    """a batch of 80 frames: noise (long streams), flat (few codes, exact sub-block sizes vary), gradients, alpha < 255"""
    w, h, n = 40, 30, 80
    rng = np.random.default_rng(4)
    frames = rgba_frames(n, w, h, seed=3)
    for k in range(0, n, 4):
        frames[k] = _frame(w, h, 100 + k, alpha=True)
    for k in range(1, n, 4):
        frames[k] = rng.integers(0, 256, 4, dtype=np.uint8) * np.ones((h, w, 1), np.uint8)
        frames[k, ..., 3] = 255
    frames[2] = 0
    src = ctx.alloc(frames.nbytes).upload(frames)
    got = ctx.gif_encode_batch_dev(src.ptr, w, h, n)
    views, release = ctx.gif_encode_batch_dev(src.ptr, w, h, n, copy=False)
    try:
        assert [bytes(v) for v in views] == got
    finally:
        release()
    for k in range(n):
        want_idx = gm.dither_wavefront(frames[k])
        assert got[k] == gm.encode_index(want_idx), "frame %d" % k
        np.testing.assert_array_equal(_decode(got[k]), want_idx)


def test_plan_run_host_paletted_gif(ctx):
    """the GIF task's leg: resize and thumbnail as GIF streams of run_host_paletted's pixels, the watermark as the JPEG stream of its
    pixels; opaque palettes plus a transparent index (the zero colour), so the resized frames carry alpha < 255"""
    w, h, n, q = 160, 120, 3, 85
    rng = np.random.default_rng(21)
    idx = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    idx[:, 20:60, 30:90] = 7
    pal = rng.integers(0, 256, (n, 256, 4), dtype=np.uint8)
    pal[..., 3] = 255
    pal[:, 7] = 0
    gs = ctx.glyphset(text_glyphs(w, h, n=5, width_px=100, height_px=24), DEFAULT_COL)
    for th in ((48, True), (48, False)):
        plan = ctx.plan(w, h, resize=(100, 70, False), thumbnail=th, watermark=gs)
        pix = plan.run_host_paletted(idx, pal)
        got = plan.run_host_paletted_gif(idx, pal, quality=q)
        for k in range(n):
            for op in ("resize", "thumbnail"):
                want_idx = gm.dither_wavefront(pix[op][k])
                assert got[op][k] == gm.encode_index(want_idx), "%s %d" % (op, k)
                np.testing.assert_array_equal(_decode(got[op][k]), want_idx)
            assert got["watermark"][k] == ctx.jpeg_encode(pix["watermark"][k], q), "watermark %d" % k
        only = plan.run_host_paletted_gif(idx, pal, quality=q, want=("thumbnail",))
        assert list(only) == ["thumbnail"] and only["thumbnail"] == got["thumbnail"]
        plan.close()
    gs.close()


def test_plan_run_host_paletted_gif_chunks(ctx, monkeypatch):
    """chunks of 2 frames: the GIF and JPEG streams do not depend on where the chunks fall"""
    w, h, n = 96, 64, 7
    rng = np.random.default_rng(22)
    idx = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    pal = rng.integers(0, 256, (n, 256, 4), dtype=np.uint8)
    pal[..., 3] = 255
    pal[:, 7] = 0
    gs = ctx.glyphset(text_glyphs(w, h, n=4, width_px=60, height_px=20), DEFAULT_COL)
    plan = ctx.plan(w, h, resize=(50, 30, False), thumbnail=(32, True), watermark=gs)
    try:
        whole = plan.run_host_paletted_gif(idx, pal, quality=80)
        monkeypatch.setenv("IPX_HOST_CHUNK_GIF", "2")
        parts = plan.run_host_paletted_gif(idx, pal, quality=80)
        assert set(whole) == {"resize", "thumbnail", "watermark"} and whole == parts
    finally:
        plan.close()
        gs.close()


def test_plan_watermark_matches_run_host_jpeg(ctx):
    """with an opaque palette the expanded frames are plain RGBA: the watermark stream is run_host_jpeg's"""
    w, h, n = 96, 64, 2
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    pal = rng.integers(0, 256, (n, 256, 4), dtype=np.uint8)
    pal[..., 3] = 255
    rgba = np.stack([pal[k][idx[k]] for k in range(n)])
    gs = ctx.glyphset(text_glyphs(w, h, n=4, width_px=60, height_px=20), DEFAULT_COL)
    plan = ctx.plan(w, h, resize=(50, 30, True), thumbnail=(32, True), watermark=gs)
    got = plan.run_host_paletted_gif(idx, pal, quality=70)
    assert got["watermark"] == plan.run_host_jpeg(rgba, quality=70)["watermark"]
    plan.close()
    gs.close()


def test_bad_arguments_touch_nothing(ctx):
    import imageprocessor_amd as m
    L = m.lib()
    w, h = 8, 8
    f = _frame(w, h, 1)
    src = ctx.alloc(f.nbytes).upload(f)
    idx = ctx.alloc(w * h).upload(np.full(w * h, 0xA5, np.uint8))
    for args in ((w, h, -1, None), (0, h, 1, None), (w, 0, 1, None), (65536, 1, 1, None), (1, 65536, 1, None),
                 (w, h, 1, w * 4 - 1)):
        ww, hh, n, stride = args
        with pytest.raises(m.IpxError) as e:
            ctx.gif_dither_dev(src.ptr, ww, hh, n, idx.ptr, stride=stride if stride is not None else ww * 4)
        assert e.value.status == -1
    with pytest.raises(m.IpxError):
        ctx.gif_dither_dev(None, w, h, 1, idx.ptr)
    ctx.sync()
    assert (idx.download(w * h) == 0xA5).all()
    # too large for gif.Encode, as Go refuses it: no stream, an error status
    wide = np.zeros((1, 65536, 4), np.uint8)
    with pytest.raises(m.IpxError) as e:
        ctx.gif_encode(wide)
    assert e.value.status == -1
    with pytest.raises(m.IpxError):
        ctx.gif_encode_batch_dev(src.ptr, 65536, 1, 1)
    import ctypes as C
    out, n = C.c_void_p(), C.c_size_t(7)
    assert L.ipx_gif_encode_rgba8(ctx.handle, None, w, h, w * 4, C.byref(out), C.byref(n)) == -1
    assert not out.value and n.value == 0
    assert L.ipx_gif_encode_batch_dev(ctx.handle, src.ptr, w, h, w * 4, w * h * 4, 1, None, None, None) == -1
    assert L.ipx_plan_run_host_paletted_gif(ctx.handle, None, 1, None, w, w * h, None, 85, None, None, None, None) == -1
    assert ctx.gif_encode_batch_dev(src.ptr, w, h, 0) == []
