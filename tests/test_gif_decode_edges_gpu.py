"""gif.Decode on the GPU on LZW streams Pillow never writes (tests/gif_edge_corpus.py): every literal width 2 .. 8, tables frozen at 4095
for most of a 1024 x 768 frame, clear codes every N codes, doubled clears, no leading clear, sub-blocks of 1 .. 255 bytes.  Every status,
index and palette byte against the frame the test built and against tests/gif_decode_model.py; beside Pillow's files, in several
decode groups and through run_gif_gif."""
import numpy as np
import pytest

import gif_corpus
import gif_decode_model as dm
import gif_edge_corpus as ge
from test_gif_decode_gpu import _check_batch, _expected_leg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _check_cases(ctx, cases, extra=()):
    files = [c[1] for c in cases] + list(extra)
    assert _check_batch(ctx, files) == [dm.OK] * len(files)
    info, _ = ctx.gif_decode_batch(files)
    for i, (name, _, idx, pal, _) in enumerate(cases):
        np.testing.assert_array_equal(info["index"][i], idx, err_msg=name)
        np.testing.assert_array_equal(info["palettes"][i][:len(pal), :3], pal, err_msg=name)


def _by_size(cases):
    out = {}
    for c in cases:
        out.setdefault(c[2].shape, []).append(c)
    return out


def test_corpus_beside_pillow_files(ctx):
    for (h, w), cases in _by_size(ge.corpus()).items():
        pil = [gif_corpus.make(w, h, 70 + k, ("photo", "flat")[k], ncol=(256, 5)[k], interlace=bool(k)) for k in range(2)]
        _check_cases(ctx, cases, pil)


def test_large_frames(ctx):
    """1024 x 768: frozen tables at every literal width and the other clear policies at width 8, with Pillow's files, one call"""
    cases = ge.large()
    assert max(c[4] for c in cases) >= 100000
    pil = [gif_corpus.make(1024, 768, 80 + k, ("photo", "flat")[k], ncol=256, interlace=bool(k)) for k in range(2)]
    _check_cases(ctx, cases, pil)


def test_scratch_groups(ctx, monkeypatch):
    """a 1 MiB code scratch: the 256 x 200 files and Pillow's in several groups"""
    cases = [ge.make("frozen noise #%d" % k, 256, 200, 8, 8, 900 + k, "noise", clear=("never", "full", "every")[k % 3], every=3,
                     sub=(255, 1, "random")[k % 3], interlace=k % 2 == 1) for k in range(6)]
    pil = [gif_corpus.make(256, 200, 90 + k, "photo", ncol=256) for k in range(3)]
    monkeypatch.setenv("IPX_GIF_DEC_SCRATCH_MB", "1")
    _check_cases(ctx, cases, pil)


def test_run_gif_gif(ctx):
    """the GIF-in, GIF-out leg on these streams equals the host leg fed with the model's frames"""
    cases = [c for c in ge.corpus() if c[2].shape == (120, 160)][:8]
    files = [c[1] for c in cases]
    plan = ctx.plan(160, 120, resize=(50, 30, False), thumbnail=(32, True))
    try:
        got, st = plan.run_gif_gif(files, quality=80, want=("resize", "thumbnail"))
        ref, want_st = _expected_leg(plan, files, 80, ("resize", "thumbnail"))
        assert st == want_st == [dm.OK] * len(files)
        for k in got:
            assert got[k] == ref[k], k
    finally:
        plan.close()
