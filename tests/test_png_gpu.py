"""png.Encode on the GPU (csrc/ipx_png.hip): the filter pass, the segment deflate and the three entries, byte for byte against
tests/png_model.py, and every stream decoded by Pillow to the pixels png.Encode writes.  PARITY UNPINNED against Go's compressed bytes."""
import io

import numpy as np
import pytest

import png_model as pm
from helpers import DEFAULT_COL, rgba_frames, text_glyphs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _frame(w, h, seed, kind="mixed"):
    """premultiplied RGBA: 'noise' (stored fallback), 'flat' (long matches), 'mixed' (gradients, noise, a flat patch), 'alpha'
    (mixed with alpha 0 and 1..254 in places)"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        f[..., 3] = 255
        return f
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 4), np.int64)
    if kind == "flat":
        f[..., 0] = np.where((xx // 16 + yy // 16) % 2 == 0, 200, 30)
        f[..., 1] = 90
        f[..., 2] = (yy // 64) * 40 % 256
    else:
        f[..., 0] = xx * 255 // max(w - 1, 1)
        f[..., 1] = yy * 255 // max(h - 1, 1)
        f[..., 2] = (xx + yy) * 3 % 256
        f[..., :3] += rng.integers(-20, 21, (h, w, 3))
        f[h // 3:h // 2, w // 4:w // 2, :3] = 90
    f[..., 3] = 255
    if kind == "alpha":
        f[..., 3] = np.where(rng.random((h, w)) < 0.4, rng.integers(0, 256, (h, w)), 255)
        f[: h // 4 + 1, : w // 4 + 1, 3] = 0
    f = f.clip(0, 255)
    f[..., :3] = f[..., :3] * f[..., 3:4] // 255
    return f.astype(np.uint8)


def _check_pixels(stream, frame):
    from PIL import Image
    im = Image.open(io.BytesIO(stream))
    bpp, raw = pm.raw_rows(frame)
    assert im.mode == ("RGB" if bpp == 3 else "RGBA")
    np.testing.assert_array_equal(np.array(im), raw.reshape(frame.shape[0], frame.shape[1], bpp))
    assert [k for k, _ in pm.read_chunks(stream)][:2] == [b"IHDR", b"IDAT"]


def _dev(ctx, frames):
    frames = np.ascontiguousarray(frames)
    return ctx.alloc(frames.nbytes).upload(frames)


@pytest.mark.parametrize("w,h,kind", [(1, 1, "mixed"), (2, 3, "alpha"), (17, 5, "noise"), (64, 48, "flat"), (200, 200, "mixed"),
                                      (333, 257, "alpha"), (640, 480, "noise"), (1024, 768, "flat"), (1920, 1080, "mixed")])
def test_png_encode_matches_model(ctx, w, h, kind):
    f = _frame(w, h, w * 7 + h, kind)
    got = ctx.png_encode(f)
    assert got == pm.png_encode(f)
    _check_pixels(got, f)


def test_png_encode_wide_rows(ctx):
    """rowbytes beyond the window: the row distances drop out of the fixed set, every row is a segment of its own"""
    for kind in ("alpha", "flat"):
        f = _frame(8200, 3, 5, kind)
        got = ctx.png_encode(f)
        assert got == pm.png_encode(f)
        _check_pixels(got, f)


def test_png_encode_alpha_values(ctx):
    """every alpha from 0 to 255 over a few colour values (the un-premultiply), in one RGBA frame"""
    a = np.arange(256, dtype=np.int64)
    f = np.zeros((8, 256, 4), np.int64)
    for r, c in enumerate((0, 1, 17, 100, 128, 200, 254, 255)):
        f[r, :, 0] = np.minimum(c, a)
        f[r, :, 1] = a // 2
        f[r, :, 2] = a * c // 255
        f[r, :, 3] = a
    f = f.astype(np.uint8)
    got = ctx.png_encode(f)
    assert got == pm.png_encode(f)
    _check_pixels(got, f)


def test_png_stored_fallback(ctx):
    """noise: every segment goes out stored, and the stream sits at the bound exactly"""
    f = _frame(300, 400, 9, "noise")
    got = ctx.png_encode(f)
    assert got == pm.png_encode(f)
    assert len(got) == pm.stream_bound(300, 400, 3)


@pytest.mark.parametrize("w,h", [(1, 1), (97, 61), (200, 200)])
def test_png_encode_batch_dev_80(ctx, w, h):
    kinds = ["mixed", "alpha", "noise", "flat"]
    frames = np.stack([_frame(w, h, 100 + i, kinds[i % 4]) for i in range(80)])
    d = _dev(ctx, frames)
    got = ctx.png_encode_batch_dev(d.ptr, w, h, 80)
    for i in range(80):
        assert got[i] == pm.png_encode(frames[i]), "frame %d" % i
    _check_pixels(got[1], frames[1])


def test_png_encode_batch_dev_strided(ctx):
    """rows and frames further apart than the pixels need"""
    w, h, n = 50, 30, 3
    big = np.zeros((n, h + 5, w + 7, 4), np.uint8)
    frames = np.stack([_frame(w, h, 7 + i, "alpha" if i else "mixed") for i in range(n)])
    big[:, :h, :w] = frames
    d = _dev(ctx, big)
    got = ctx.png_encode_batch_dev(d.ptr, w, h, n, stride=(w + 7) * 4, frame_stride=(h + 5) * (w + 7) * 4)
    assert got == [pm.png_encode(f) for f in frames]
    views, release = ctx.png_encode_batch_dev(d.ptr, w, h, n, stride=(w + 7) * 4, frame_stride=(h + 5) * (w + 7) * 4, copy=False)
    assert [bytes(v) for v in views] == got
    release()
    assert ctx.png_encode_batch_dev(d.ptr, w, h, 0) == []


def test_png_bad_arguments(ctx):
    import ctypes as C

    import imageprocessor_amd as m
    from imageprocessor_amd import _lib
    f = np.zeros((4, 4, 4), np.uint8)
    out, n = C.c_void_p(), C.c_size_t()
    L = m.lib()
    for w, h, stride in ((0, 4, 16), (4, 0, 16), (-1, 4, 16), (4, 4, 15)):
        assert L.ipx_png_encode_rgba8(ctx.handle, f.ctypes.data, w, h, stride, C.byref(out), C.byref(n)) == -1
    assert L.ipx_png_encode_rgba8(ctx.handle, None, 4, 4, 16, C.byref(out), C.byref(n)) == -1
    assert L.ipx_png_encode_rgba8(ctx.handle, f.ctypes.data, 4, 4, 16, None, C.byref(n)) == -1
    assert L.ipx_png_encode_rgba8(ctx.handle, f.ctypes.data, 70000, 1, 280000, C.byref(out), C.byref(n)) == -4
    blob, offs, lens = C.c_void_p(), (C.c_size_t * 1)(), (C.c_size_t * 1)()
    assert L.ipx_png_encode_batch_dev(ctx.handle, f.ctypes.data, 4, 4, 16, 64, -1, C.byref(blob), offs, lens) == -1
    assert L.ipx_png_encode_batch_dev(ctx.handle, f.ctypes.data, 0, 4, 16, 64, 1, C.byref(blob), offs, lens) == -1
    assert L.ipx_png_encode_batch_dev(ctx.handle, f.ctypes.data, 4, 4, 16, 64, 1, None, offs, lens) == -1
    plan = ctx.plan(8, 8, resize=(4, 4, False), thumbnail=None)
    res = C.c_void_p()
    outs = (_lib.Bytes * 1)()
    assert L.ipx_plan_run_host_png(ctx.handle, plan.handle, 1, None, 32, 256, outs, None, None, C.byref(res)) == -1
    assert L.ipx_plan_run_host_png(ctx.handle, plan.handle, 1, f.ctypes.data, 31, 256, outs, None, None, C.byref(res)) == -1
    assert L.ipx_plan_run_host_png(ctx.handle, plan.handle, -1, f.ctypes.data, 32, 256, outs, None, None, C.byref(res)) == -1
    plan.close()
    with pytest.raises(m.IpxError):
        ctx.png_encode(np.zeros((0, 4, 4), np.uint8))


def test_run_host_png_matches_model_of_run_host(ctx):
    sw, sh, n = 320, 180, 5
    frames = rgba_frames(n, sw, sh, seed=11)
    frames[1, ..., 3] = np.where(np.arange(sw)[None, :] % 7 == 0, 128, 255)   # a frame with alpha: colour type 6 on every output
    frames[1, ..., :3] = frames[1, ..., :3] // 2
    glyphs = text_glyphs(sw, sh)
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(sw, sh, resize=(256, 144, True), thumbnail=(64, True), watermark=gs)
    pix = plan.run_host(frames)
    got = plan.run_host_png(frames)
    assert set(got) == {"resize", "thumbnail", "watermark"}
    for k in got:
        for i in range(n):
            assert got[k][i] == pm.png_encode(pix[k][i]), "%s of frame %d" % (k, i)
        _check_pixels(got[k][1], pix[k][1])
    lens = plan.run_host_png(frames, want=("thumbnail",), copy=False)
    assert lens == {"thumbnail": [len(s) for s in got["thumbnail"]]}
    plan.close()
    gs.close()


def test_run_host_png_chunks(ctx, monkeypatch):
    """chunks of 3 frames: the streams do not depend on where the chunks fall"""
    sw, sh, n = 96, 64, 7
    frames = rgba_frames(n, sw, sh, seed=12)
    frames[4, ..., 3] = 128
    frames[4, ..., :3] //= 2
    gs = ctx.glyphset(text_glyphs(sw, sh), DEFAULT_COL)
    plan = ctx.plan(sw, sh, resize=(50, 30, False), thumbnail=(32, True), watermark=gs)
    try:
        whole = plan.run_host_png(frames)
        monkeypatch.setenv("IPX_HOST_CHUNK_PNG", "3")
        parts = plan.run_host_png(frames)
        assert set(whole) == {"resize", "thumbnail", "watermark"} and whole == parts
    finally:
        plan.close()
        gs.close()
