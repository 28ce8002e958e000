"""The parallel inflate on the GPU (csrc/ipx_png_dec_par.hip, IPX_PNG_PAR=1) at its ring, match-list and redo edges: the cases of
tests/png_par_corpus.py that tests/test_png_par_corpus.py proves to reach them, at the sizes EDGE_SUBS (the default, 48, 254 -- a round
of 5461 matches -- and 1000, where every window restages); the older corpus at the two sizes it never ran at; the clamp of
IPX_PNG_PAR_SUB; streams in order with a byte or a chunk behind the Adler-32, which only a serial walk (png_inflate_redo_kernel) that got
every token, every flush and the checksum right answers with IPX_ERR_UNSUPPORTED; and one launch of files that take very different
paths.  Every status and frame is the model's and the one of the same call with the switch unset, and the counts are the model's."""
import numpy as np
import pytest

import png_decode_model as dm
import png_edge_corpus as pe
import png_par_corpus as ppc
import png_par_model as pm
from test_png_par_gpu import File, _one, env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


_FILES, _UNSET = {}, {}


def file_of(c, exact=True):
    """the File of a corpus case, made once (the model's answer, and its token counts by size)"""
    if c.name not in _FILES:
        fast = getattr(c, "damage", "") in ("", "trailing byte", "trailing idat")      # zlib takes these streams; the broken ones it does not
        _FILES[c.name] = File(c.name, c.data, getattr(c, "adam7", False), getattr(c, "tags", ()), fast=fast, exact=exact)
    return _FILES[c.name]


def unset(ctx, f):
    """the file's answer with the switch unset, asked once"""
    if f.name not in _UNSET:
        with env(IPX_PNG_ADAM7=1 if f.adam7 else None):
            _UNSET[f.name] = ctx.png_decode_batch([f.data])
    return _UNSET[f.name]


EDGE = [c for c in ppc.corpus(edges=True) if c.tags[0] in ppc.EDGE_TAGS]
OLD = [c for c in ppc.corpus() if not c.damage]
TWINS = ppc.trailing_twins()


@pytest.mark.parametrize("sub", ppc.EDGE_SUBS)
@pytest.mark.parametrize("tag", ppc.EDGE_TAGS)
def test_every_edge_case_alone(ctx, tag, sub):
    files = [file_of(c) for c in EDGE if c.tags[0] == tag]
    assert files
    for f in files:
        assert f.want["status"] == dm.OK and not f.redo
        _one(ctx, f, sub, unset(ctx, f))


@pytest.mark.parametrize("sub", [254, pm.SUB_MAX])
@pytest.mark.parametrize("part", range(3))
def test_the_older_corpus_at_the_sizes_it_lacked(ctx, part, sub):
    """a third of its clean files per row"""
    assert sub not in ppc.SUBS and len(OLD) == 38
    for c in OLD[part::3]:
        f = file_of(c)
        _one(ctx, f, sub, unset(ctx, f))


@pytest.mark.parametrize("part", range(2))
def test_the_edge_corpus_at_1000(ctx, part):
    """tests/png_edge_corpus.py, whose large files the model parses at the default size only: the sum of the counts (half per row)"""
    for c in pe.corpus()[part::2]:
        f = file_of(c, exact=False)
        _one(ctx, f, pm.SUB_MAX, unset(ctx, f))


@pytest.mark.parametrize("part", range(3))
def test_trailing_twins_alone(ctx, part):
    """Something behind the Adler-32 of a stream in order.  The parallel kernel enters the file, does not finish it and hands it back;
    ipx_png_decode_files counts nothing of a file whose redo bit is set (it skips the token words), so the counts move by [1, 0, 1, 0,
    0]; the redo kernel's walk of the whole stream answers IPX_ERR_UNSUPPORTED, as the serial kernel does with the switch unset."""
    for c in TWINS[part::3]:
        f = file_of(c)
        assert f.want["status"] == dm.UNSUPPORTED and f.redo and f.parsed, c.name
        before = ctx.png_decode_counts()
        _one(ctx, f, pm.SUB_DEFAULT, unset(ctx, f))
        assert [a - b for a, b in zip(ctx.png_decode_counts(), before)] == [1, 0, 1, 0, 0], c.name
        assert unset(ctx, f)[1] == [dm.UNSUPPORTED], c.name


def test_trailing_twins_at_1000(ctx):
    twins = [c for c in TWINS if c.tags[0] in ("alias", "wrap", "list", "far") and c.damage == "trailing byte"]
    assert {c.tags[0] for c in twins} == {"alias", "wrap", "list", "far"} and len(twins) == 7
    for c in twins:
        f = file_of(c)
        before = ctx.png_decode_counts()
        _one(ctx, f, pm.SUB_MAX, unset(ctx, f))
        assert [a - b for a, b in zip(ctx.png_decode_counts(), before)] == [1, 0, 1, 0, 0], c.name
        assert unset(ctx, f)[1] == [dm.UNSUPPORTED], c.name


# env_int (csrc/ipx_runtime_internal.h) is atoi of a value that is set and not empty, else the default: "abc" is 0, which the clamp makes
# 48; "" is the default, 256
@pytest.mark.parametrize("value,sub", [("0", 48), ("47", 48), ("-3", 48), ("1001", 1000), ("100000", 1000), ("abc", 48), ("", 256)])
def test_the_size_is_clamped(ctx, value, sub):
    for tag in ("parts", "list", "budget-lone"):
        f = file_of(next(c for c in OLD + EDGE if c.tags[0] == tag))
        lanes, uniform = f.counts(sub)
        if tag == "budget-lone":     # the lanes take every token of the other two at any size; this file's split tells the three apart
            assert len({f.counts(probe) for probe in (48, 256, 1000)}) == 3
        before = ctx.png_decode_counts()
        with env(IPX_PNG_PAR=1, IPX_PNG_PAR_SUB=value):
            info, st = ctx.png_decode_batch([f.data])
        d = [a - b for a, b in zip(ctx.png_decode_counts(), before)]
        assert st == [dm.OK] and d == [1, 1, 0, lanes, uniform], (f.name, value, d)
        np.testing.assert_array_equal(info["pix"][0], f.want["pix"], err_msg=f.name)


@pytest.mark.parametrize("sub", [pm.SUB_DEFAULT, pm.SUB_MIN])
def test_one_launch_of_many_paths(ctx, sub):
    """37 files of one frame size in one call, then in reversed order: clean files that take 64 passes a window, fill the match list,
    reach the uniform loop, hold three tokens or hundreds of blocks, and between them files that are redone -- in order with a byte
    behind them, and damaged"""
    cases = ppc.mixed_launch()
    files = [file_of(c) for c in cases]
    assert len(files) >= 32 and sum(1 for c in cases if c.damage) >= 6
    want = [f.want["status"] for f in files]
    assert want == [dm.OK if not c.damage else dm.UNSUPPORTED if c.damage == "trailing byte" else dm.INVALID for c in cases]
    runs = [f.counts(sub) for f, c in zip(files, cases) if not c.damage]
    expect = [len(files), len(runs), len(files) - len(runs), sum(r[0] for r in runs), sum(r[1] for r in runs)]
    blobs = [f.data for f in files]
    with env():
        ref, ref_st = ctx.png_decode_batch(blobs)
    assert ref_st == want
    for order in (list(range(len(files))), list(range(len(files)))[::-1]):
        before = ctx.png_decode_counts()
        with env(IPX_PNG_PAR=1, IPX_PNG_PAR_SUB=sub):
            info, st = ctx.png_decode_batch([blobs[i] for i in order])
        d = [a - b for a, b in zip(ctx.png_decode_counts(), before)]
        assert st == [want[i] for i in order], order[0]
        assert (info["w"], info["h"], info["kind"]) == (ref["w"], ref["h"], ref["kind"]) == (ppc.MIXED_LENGTH - 1, 1, files[0].want["kind"])
        for k, i in enumerate(order):
            if want[i] == dm.OK:
                np.testing.assert_array_equal(info["pix"][k], files[i].want["pix"], err_msg=files[i].name)
                np.testing.assert_array_equal(info["pix"][k], ref["pix"][i], err_msg=files[i].name)
        assert d == expect, (order[0], d, expect)
