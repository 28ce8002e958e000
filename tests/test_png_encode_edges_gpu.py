"""png.Encode on the GPU (csrc/ipx_png.hip) at the edges of its coders: every frame of tests/png_encode_corpus.py through the public
entries, byte for byte against tests/png_model.py, and independently inflated by zlib to the filtered rows of the corpus' plain
per-byte filter loop.  What each frame reaches (Huffman limits, forced distance symbols, the window, stored blocks, match caps, filter
ties) is asserted on the CPU by tests/test_encode_edge_corpus.py."""
import numpy as np
import pytest

import png_encode_corpus as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _check(got, f, what):
    assert got == pc.model_stream(f), what
    pc.check_stream(got, f)


@pytest.mark.parametrize("rec", pc.recipes(), ids=["%s-%dx%d-%d" % r for r in pc.recipes()])
def test_corpus_frame(ctx, rec):
    f = pc.frame(*rec)
    _check(ctx.png_encode(f), f, rec)


def test_known_answers(ctx):
    """the hand-derived filter types and filtered bytes of golden/png_kats.json, after inflating the GPU's stream"""
    for case, f in pc.kat_frames():
        got = ctx.png_encode(f)
        _check(got, f, case["name"])
        _, data = pc.inflate(got)
        n = 1 + case["w"] * case["bpp"]
        assert len(data) == n * case["h"], case["name"]
        assert [data[y * n] for y in range(case["h"])] == case["types"], case["name"]
        assert [list(data[y * n + 1:(y + 1) * n]) for y in range(case["h"])] == case["filtered"], case["name"]


@pytest.mark.parametrize("k", range(len(pc.BATCHES)), ids=["%dx%d" % b[:2] for b in pc.BATCHES])
def test_batch_dev(ctx, k):
    """frames of one shape through the batch entry: colour types 2 and 6, stored and dynamic segments and a limit-reaching frame side
    by side; the streams are the single-frame entry's"""
    w, h, _ = pc.BATCHES[k]
    frames = pc.batch_frames(k)
    d = ctx.alloc(len(frames) * w * h * 4).upload(np.stack(frames))
    got = ctx.png_encode_batch_dev(d.ptr, w, h, len(frames))
    assert len(got) == len(frames)
    for i, f in enumerate(frames):
        _check(got[i], f, "frame %d of batch %d" % (i, k))


@pytest.mark.parametrize("k,extra_stride,extra_frame", [(0, 12, 20), (2, 4, 0), (1, 0, 36)])
def test_batch_dev_strided(ctx, k, extra_stride, extra_frame):
    """rows and frames further apart than the pixels need; the padding is 0xA5 in every byte, alpha included"""
    w, h, _ = pc.BATCHES[k]
    frames = pc.batch_frames(k)
    buf, stride, fs = pc.lay_out(frames, extra_stride, extra_frame)
    d = ctx.alloc(buf.nbytes).upload(buf)
    got = ctx.png_encode_batch_dev(d.ptr, w, h, len(frames), stride=stride, frame_stride=fs)
    for i, f in enumerate(frames):
        _check(got[i], f, "frame %d of batch %d" % (i, k))
