"""png.Decode on the GPU on streams zlib never writes (tests/png_edge_corpus.py): far and overlapping matches up to 32768 back through
the 32 KiB LDS ring, Go-style code-length sequences, 15-bit codes on hot symbols, stored blocks at every offset and length, block
sequences, raw lengths at the 16 KiB flush units; up to 1920 x 1080.  Every status, frame and palette byte against the frame the test
built and against tests/png_decode_model.py; alone, beside zlib's files, in several decode groups and through run_png_png.  And the
unfilter's 64-row band edges for every row of the type table."""
import numpy as np
import pytest

import png_corpus as pc
import png_decode_model as dm
import png_edge_corpus as pe
from helpers import DEFAULT_COL, text_glyphs
from test_png_decode_gpu import _check_batch, _host_outputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _zlib_twin(c, seed):
    """a file zlib wrote of the case's size and kind (gray / RGB / RGBA 8)"""
    ctype = {dm.GRAY: 0, dm.RGBA: 2, dm.NRGBA: 6}[c.kind]
    return pc.of_type(ctype, 8, False, c.h, c.w, seed=seed, filters=(seed % 5, 4))


def _check_cases(ctx, cases, extra=()):
    """one call of the cases (one size and kind) and zlib's files: the model's statuses and frames, and every case's frame is the
    one the test built"""
    files = [c.data for c in cases] + list(extra)
    assert _check_batch(ctx, files, fast=True) == [dm.OK] * len(files)
    info, st = ctx.png_decode_batch(files)
    for i, c in enumerate(cases):
        np.testing.assert_array_equal(info["pix"][i], c.frame, err_msg=c.name)


def _by_size(cases):
    out = {}
    for c in cases:
        out.setdefault((c.w, c.h, c.kind), []).append(c)
    return out


@pytest.fixture(scope="module")
def corpus():
    return pe.corpus()


def test_corpus_beside_zlib_files(ctx, corpus):
    """each size's cases in one call, a zlib file of that size and kind on either side"""
    for k, cases in enumerate(_by_size(corpus).values()):
        twin = _zlib_twin(cases[0], 50 + k)
        _check_cases(ctx, cases, [twin])
        assert _check_batch(ctx, [twin] + [c.data for c in cases] + [twin], fast=True)[1:-1] == [dm.OK] * len(cases)


def test_large_frames(ctx):
    """1920 x 1080 RGB 8 and 1024 x 768 RGBA 8: far matches and long codes over many flush units, beside zlib's file"""
    for c in pe.large():
        _check_cases(ctx, [c], [_zlib_twin(c, 7)])


def test_scratch_groups(ctx, monkeypatch):
    """a 1 MiB scratch budget: the far / long-code files of one size in several decode groups, zlib's files among them"""
    cases = [pe.far_case("far rgba8 97x150 #%d" % k, 97, 150, 6, 8, 400 + k, nblocks=3 + k) for k in range(8)]
    twins = [_zlib_twin(cases[0], 60 + k) for k in range(4)]
    monkeypatch.setenv("IPX_PNG_DEC_SCRATCH_MB", "1")
    _check_cases(ctx, cases, twins)


def test_run_png_png(ctx):
    """the PNG-in, PNG-out leg on far / long-code files equals the host leg on the frames the test built"""
    sw, sh = 500, 160
    gs = ctx.glyphset(text_glyphs(sw, sh), DEFAULT_COL)
    plan = ctx.plan(sw, sh, resize=(160, 120, True), thumbnail=(50, True), watermark=gs)
    try:
        cases = [pe.far_case("far gray8 500x160 #%d" % k, sw, sh, 0, 8, 500 + k) for k in range(3)]
        out, st = plan.run_png_png([c.data for c in cases])
        assert st == [dm.OK] * 3
        want = _host_outputs(plan, dm.GRAY, [{"pix": c.frame} for c in cases])
        for k in want:
            for i in range(3):
                assert out[k][i] == ctx.png_encode(want[k][i]), (k, i)
    finally:
        plan.close()
        gs.close()


@pytest.mark.parametrize("name,ctype,depth,trns", pc.TYPES, ids=[t[0] for t in pc.TYPES])
def test_unfilter_band_edges(ctx, name, ctype, depth, trns):
    """heights either side of the 64-row bands, 1 and 6 columns, Up / Average / Paeth / a mix: the model's frames and the frames
    of the samples the test chose"""
    for h in (63, 64, 65, 128, 129, 192):
        for w in (1, 6):
            files, want = [], []
            for j, fl in enumerate(((2,), (3,), (4,), (2, 3, 4, 0, 1))):
                seed = 1000 + 10 * h + w + j
                kind = ("photo", "flat")[j % 2]
                f = pc.of_type(ctype, depth, trns, h, w, seed=seed, kind=kind, filters=fl)
                _, fields = dm.parse(f)
                s = pc.samples_of_type(ctype, depth, h, w, seed, kind)
                want.append(dm.convert(pc.pack_rows(s, ctype, depth), ctype, depth, w, h, fields["trns"]))
                files.append(f)
            assert _check_batch(ctx, files) == [dm.OK] * 4
            info, _ = ctx.png_decode_batch(files)
            for i in range(4):
                np.testing.assert_array_equal(info["pix"][i], want[i], err_msg="%s %dx%d file %d" % (name, w, h, i))
