"""The parallel GIF code walk on the GPU (csrc/ipx_gif_dec_par.hip, IPX_GIF_PAR=1) at its own edges: data longer than the LDS staging
window under every sub-block framing, the EOF code in the first and the last lane of its round, garbage behind a clear code, 1024 x 768
files, every stream it must leave to the serial walk between two valid neighbours, and several decode groups.  Streams:
tests/gif_par_corpus.py; every comparison against the frames the test built, tests/gif_decode_model.py and the same call with the switch
unset; the counts against tests/gif_par_model.py."""
import numpy as np
import pytest

import gif_corpus
import gif_decode_model as dm
import gif_edge_corpus as ge
import gif_par_corpus as gpc
import gif_par_model as pm
from test_gif_par_gpu import env, one

pytestmark = pytest.mark.gpu

WINDOW = 4096                # kParWin of ipx_gif_dec_par.hip: bytes of LZW data staged at a time


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


@pytest.mark.parametrize("sub", [1, 255, "random"])
@pytest.mark.parametrize("interlace", [False, True])
def test_data_longer_than_the_staging_window(ctx, sub, interlace):
    """several windows' worth of codes of every width; a code straddles a window's edge wherever the round before ended"""
    for lit, bits, pol in ((8, 8, dict(clear="full")), (8, 8, dict(clear="never")), (3, 3, dict(clear="every", every=777))):
        name, data, idx, _, _ = ge.make("window lit %d %s" % (lit, pol), 160, 120, bits, lit, 5, "noise", sub=sub, interlace=interlace, **pol)
        assert len(pm.stream_of(data).data) > 2 * WINDOW
        d, _ = one(ctx, name, data, idx)
        assert d[1] == 1, name


@pytest.mark.parametrize("lane", [0, 63])
def test_eof_code_in_this_lane(ctx, lane):
    data, idx = gpc.eof_in_lane(lane)
    d, par = one(ctx, "EOF code in lane %d" % lane, data, idx)
    assert d[1] == 1 and gpc.last_round(par) == (lane, 2)


def test_garbage_behind_a_clear_code(ctx):
    data, idx = gpc.garbage_behind_a_clear()
    d, _ = one(ctx, "garbage behind a clear", data, idx)
    assert d[1] == 1


def test_large_files(ctx):
    """1024 x 768: Pillow's photo-like file and a table frozen for most of the frame; the record counts by the serial walk's model
    (the two models' records are equal: test_gif_par_model.py)"""
    name, frozen, idx, _, n = ge.make("1024x768 frozen", 1024, 768, 8, 8, 9, "photo", clear="never", interlace=True)
    assert n > 100000
    photo = gif_corpus.make(1024, 768, 80, "photo", ncol=256)
    for what, data, want_idx in (("pillow photo", photo, None), (name, frozen, idx)):
        ser = pm.serial_walk(pm.stream_of(data))
        assert ser.status == 0 and ser.how == "eof"
        d, _ = one(ctx, what, data, want_idx, records=len(ser.records))
        assert d[1] == 1, what


def test_redo_cases_between_valid_neighbours(ctx):
    """every case the parallel walk must not decide: the status is the model's, the neighbours' frames are exact, the counts say who
    walked what"""
    left = ge.make("left", 160, 120, 8, 8, 41, "noise", clear="full")
    right = ge.make("right", 160, 120, 4, 4, 42, "runs", clear="never", interlace=True)
    nrec = [len(pm.par_walk(pm.stream_of(c[1])).records) for c in (left, right)]
    cases = gpc.redo_cases()
    assert [name for name, _, _ in cases] == ["truncated data", "EOF before the frame is full", "one byte too many", "code above hi in lane 0",
                                              "code above hi in lane 63", "literal past a short palette", "extra sub-block behind the EOF code",
                                              "missing EOF code, complete frame"]
    for name, data, want_st in cases:
        par = pm.par_walk(pm.stream_of(data))
        assert par.redo, name
        assert want_st == (dm.OK if name.startswith("missing EOF") else dm.INVALID), name
        if "lane" in name:
            assert gpc.last_round(par) == (int(name.split()[-1]), 4) and par.rounds == 3, name
        files = [left[1], data, right[1]]
        with env():
            ref, ref_st = ctx.gif_decode_batch(files)
        before = ctx.gif_decode_counts()
        with env(IPX_GIF_PAR=1):
            got, st = ctx.gif_decode_batch(files)
        d = [a - b for a, b in zip(ctx.gif_decode_counts(), before)]
        assert st == ref_st == [dm.OK, want_st, dm.OK], name
        for i in (0, 2):
            np.testing.assert_array_equal(got["index"][i], (left, right)[i // 2][2], err_msg=name)
            np.testing.assert_array_equal(got["index"][i], ref["index"][i], err_msg=name)
            np.testing.assert_array_equal(got["palettes"][i], ref["palettes"][i], err_msg=name)
        if want_st == dm.OK:
            np.testing.assert_array_equal(got["index"][1], dm.decode(data)["index"], err_msg=name)
            np.testing.assert_array_equal(got["index"][1], ref["index"][1], err_msg=name)
        assert d == [3, 2, 1, sum(nrec)], (name, d)
        # and alone: [1, 0, 1, 0]
        d, _ = one(ctx, name, data)
        assert d == [1, 0, 1, 0], (name, d)


def test_scratch_groups(ctx):
    """a 1 MiB code scratch: the 256 x 200 files in several groups, a file for the serial walk among them"""
    cases = [ge.make("group #%d" % k, 256, 200, 8, 8, 900 + k, "noise", clear=("never", "full", "every")[k % 3], every=3,
                     sub=(255, 1, "random")[k % 3], interlace=k % 2 == 1) for k in range(6)]
    nrec = [len(pm.par_walk(pm.stream_of(c[1])).records) for c in cases]
    assert sum(nrec) * 12 > 2 << 20
    files = [c[1] for c in cases]
    files.insert(3, files[0][:len(files[0]) // 2])
    with env():
        ref, ref_st = ctx.gif_decode_batch(files)
    before = ctx.gif_decode_counts()
    with env(IPX_GIF_PAR=1, IPX_GIF_DEC_SCRATCH_MB=1):
        got, st = ctx.gif_decode_batch(files)
    d = [a - b for a, b in zip(ctx.gif_decode_counts(), before)]
    assert st == ref_st == [dm.OK] * 3 + [dm.INVALID] + [dm.OK] * 3
    for i, c in enumerate(cases):
        j = i + (i >= 3)
        np.testing.assert_array_equal(got["index"][j], c[2], err_msg=c[0])
        np.testing.assert_array_equal(got["palettes"][j], ref["palettes"][j], err_msg=c[0])
    assert d == [7, 6, 1, sum(nrec)]
