"""gif.Encode on the GPU (csrc/ipx_gif.hip) at the edges of its LZW coder and of its dither: every case of tests/gif_encode_corpus.py
through the public entries, byte for byte against tests/gif_model.py, and independently decoded by the reader of compress/lzw
(tests/gif_decode_model.py) and by Pillow to the indices.  The LZW inputs go in as opaque frames of Plan 9 colours, which dither to
exactly the chosen indices.  What each case reaches (final hi, the width of EOF, where the 4095 clear falls, the last sub-block, the
clamps) is asserted on the CPU by tests/test_encode_edge_corpus.py."""
import numpy as np
import pytest

import gif_encode_corpus as gc
import gif_model as gm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _check(got, idx, what):
    assert got == gm.encode_index(idx), what
    gc.check_stream(got, idx)


def _dither(ctx, frames, stride=None, frame_stride=None, buf=None):
    n, h, w = frames.shape[:3]
    src = ctx.alloc((buf if buf is not None else frames).nbytes).upload(buf if buf is not None else frames)
    idx = ctx.alloc(n * w * h)
    ctx.gif_dither_dev(src.ptr, w, h, n, idx.ptr, stride=stride, frame_stride=frame_stride)
    ctx.sync()
    return idx.download((n, h, w))


@pytest.mark.parametrize("k", range(len(gc.lzw_cases())), ids=[c[0] for c in gc.lzw_cases()])
def test_lzw_case(ctx, k):
    name, idx, _ = gc.lzw_cases()[k]
    got = ctx.gif_encode(gc.index_frame(idx))
    _check(got, idx, name)
    for c in gc.kats():
        if name == "kat: " + c["name"]:                  # the hand-derived data, not only the model's
            assert gc.lzw_payload(got, idx.shape[1], idx.shape[0])[0].hex() == c["lzw_hex"]


@pytest.mark.parametrize("k", range(len(gc.lzw_batches())), ids=["%dx%d" % b[:2] for b in gc.lzw_batches()])
def test_lzw_batch_dev(ctx, k):
    """frames of one shape through the batch entry, tightly packed and with padded rows and frames: clears on both sides of the staging
    chunk's edge, a frame that clears at Close and one that does not, side by side"""
    w, h, frames = gc.lzw_batches()[k]
    rgba = [gc.index_frame(i) for i in frames]
    src = ctx.alloc(len(rgba) * w * h * 4).upload(np.stack(rgba))
    got = ctx.gif_encode_batch_dev(src.ptr, w, h, len(rgba))
    buf, stride, fs = gc.lay_out(rgba, 12, 40)
    pad = ctx.alloc(buf.nbytes).upload(buf)
    assert ctx.gif_encode_batch_dev(pad.ptr, w, h, len(rgba), stride=stride, frame_stride=fs) == got
    for i, idx in enumerate(frames):
        _check(got[i], idx, "frame %d of batch %d" % (i, k))


@pytest.mark.parametrize("k", range(len(gc.dither_cases())), ids=[c[0] for c in gc.dither_cases()])
def test_dither_case(ctx, monkeypatch, k):
    """the dither entry and the stream entry against drawPaletted line by line (gif_model.dither_scalar), with the number of waves
    the case asks for"""
    name, f, waves = gc.dither_cases()[k]
    if waves:
        monkeypatch.setenv("IPX_GIF_WAVES", waves)
    want = gc.dither_reference(k)
    np.testing.assert_array_equal(_dither(ctx, f[None])[0], want, err_msg=name)
    h, w = f.shape[:2]
    buf, stride, fs = gc.lay_out([f, f], 8, 24)
    got = _dither(ctx, np.stack([f, f]), stride=stride, frame_stride=fs, buf=buf)
    np.testing.assert_array_equal(got[0], want, err_msg=name + ", padded rows")
    np.testing.assert_array_equal(got[1], want, err_msg=name + ", second frame")
    _check(ctx.gif_encode(f), want, name)


def test_tie_colours(ctx):
    """colours at the same distance from two palette entries, one 1 x 1 frame each: the first minimum decides"""
    frames, first = gc.tie_frames()
    np.testing.assert_array_equal(_dither(ctx, frames).reshape(-1), first)
    src = ctx.alloc(frames.nbytes).upload(frames)
    got = ctx.gif_encode_batch_dev(src.ptr, 1, 1, len(frames))
    for i in range(len(frames)):
        _check(got[i], first[i].reshape(1, 1), "tie colour %d" % i)
