"""The parallel inflate on the GPU (csrc/ipx_png_dec_par.hip, IPX_PNG_PAR=1) through ipx_png_decode_batch, one call per file: the corpus of
tests/png_par_corpus.py, the known answers of tests/golden/png_dec_kats.json and the corpus of tests/png_edge_corpus.py, at three
sub-sequence sizes (IPX_PNG_PAR_SUB).  Every status, frame and palette byte is the model's (tests/png_decode_model.py) and the one of the
same call with the switch unset; ipx_png_decode_counts shows that the parallel kernel did the work -- a kernel that handed every file
to the serial decoder would pass every byte comparison -- and its token counts are those of tests/png_par_model.py."""
import contextlib
import json
import os

import numpy as np
import pytest

import png_adam7_model as a7m
import png_decode_model as dm
import png_edge_corpus as pe
import png_par_corpus as ppc
import png_par_model as pm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "png_dec_kats.json")) as f:
    KATS = json.load(f)
SWITCHES = ("IPX_PNG_PAR", "IPX_PNG_PAR_SUB", "IPX_PNG_ADAM7")


@contextlib.contextmanager
def env(**kw):
    """the three switches as given (a missing one unset) for the block; what was there before comes back"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if kw.get(k) is not None:
                os.environ[k] = str(kw[k])
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


class File:
    """one file of a set: its bytes, the model's answer, and the model of the parallel parse of its stream"""
    def __init__(self, name, data, adam7=False, tags=(), damage="", fast=False, exact=True):
        self.name, self.data, self.adam7, self.tags, self.damage = name, bytes(data), adam7, tags, damage
        self.exact, self.runs = exact, {}
        self.want = a7m.decode(self.data, adam7=adam7, fast=fast)
        self.parsed = self.want["stage"] == "data"
        self.model = pm.Model(ppc.idat_of(self.data)) if self.parsed else None
        # the parallel kernel leaves every stream that is not in order, or has bytes behind it; a filter byte above 4 is the unfilter's
        self.redo = self.parsed and self.want["status"] != dm.OK and self.want["why"] != "bad filter type"

    def counts(self, sub):
        """(tokens of the lanes, tokens of the uniform loop) at this size; not exact (the large files of the edge corpus): the model
        runs once, at the default size, and only the sum is known at the others (it does not depend on the size)"""
        at = sub if self.exact else pm.SUB_DEFAULT
        if at not in self.runs:
            self.runs[at] = self.model.run(at)
        r = self.runs[at]
        assert not r.redo, (self.name, r.why)
        return (r.lane_tokens, r.uniform_tokens) if at == sub else (r.lane_tokens + r.uniform_tokens, None)


def _sets():
    return {"par": [File(c.name, c.data, c.adam7, c.tags, c.damage, fast=not c.damage) for c in ppc.corpus()],
            "kats": [File(k["name"], bytes.fromhex(k["data"])) for k in KATS],
            "edge": [File(c.name, c.data, fast=True, exact=False) for c in pe.corpus()]}


@pytest.fixture(scope="module")
def sets():
    return _sets()


@pytest.fixture(scope="module")
def unset(ctx, sets):
    """every file's answer with the switch unset: (info, status) by set and name"""
    out = {}
    for sname, files in sets.items():
        for f in files:
            with env(IPX_PNG_ADAM7=1 if f.adam7 else None):
                out[sname, f.name] = ctx.png_decode_batch([f.data])
    return out


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert (a["w"], a["h"], a["kind"]) == (b["w"], b["h"], b["kind"]), what
        np.testing.assert_array_equal(a["pix"], b["pix"], err_msg=what)
        assert (a["palettes"] is None) == (b["palettes"] is None), what
        if a["palettes"] is not None:
            np.testing.assert_array_equal(a["palettes"], b["palettes"], err_msg=what)


def _one(ctx, f, sub, ref):
    what = "%s (sub %d)" % (f.name, sub)
    before = ctx.png_decode_counts()
    with env(IPX_PNG_PAR=1, IPX_PNG_PAR_SUB=sub, IPX_PNG_ADAM7=1 if f.adam7 else None):
        info, st = ctx.png_decode_batch([f.data])
    d = [a - b for a, b in zip(ctx.png_decode_counts(), before)]
    assert st == [f.want["status"]], (what, f.want["why"])
    assert st == ref[1], what
    _same(info, ref[0], what)
    if st == [dm.OK]:
        np.testing.assert_array_equal(info["pix"][0], f.want["pix"], err_msg=what)
        if f.want["palette"] is not None:
            np.testing.assert_array_equal(info["palettes"][0], f.want["palette"], err_msg=what)
    assert d[0] == d[1] + d[2] == (1 if f.parsed else 0), (what, d)
    assert d[2] == (1 if f.redo else 0), (what, d, f.want["why"])     # a valid stream is never handed back; a damaged one always is
    if f.damage:
        assert d[2] == 1 and st == [dm.INVALID], (what, d)
    if d[1]:
        lanes, uniform = f.counts(sub)
        assert (d[3], d[4]) == (lanes, uniform) if uniform is not None else d[3] + d[4] == lanes, (what, d, lanes, uniform)
        if "literal-only" in f.tags:
            assert d[4] == 0 and d[3] > 0, (what, d)
        if "budget-lone" in f.tags and sub == pm.SUB_DEFAULT:
            assert d[4] > 0, (what, d)
    else:
        assert d[3] == d[4] == 0, (what, d)


@pytest.mark.parametrize("sub", ppc.SUBS)
@pytest.mark.parametrize("sname", ["par", "kats", "edge"])
def test_every_file_alone(ctx, sets, unset, sname, sub):
    for f in sets[sname]:
        _one(ctx, f, sub, unset[sname, f.name])


def test_sets_hold_what_the_counts_are_asked_on(sets):
    par = sets["par"]
    assert sum(1 for f in par if f.damage) >= 12 and all(f.redo for f in par if f.damage)
    assert all(f.want["status"] == dm.OK for f in par if not f.damage)
    assert sum(1 for f in par if "literal-only" in f.tags and not f.damage) >= 4
    assert sum(1 for f in sets["kats"] if f.redo) >= 20 and any(not f.parsed for f in sets["kats"])
    assert any(f.parsed and not f.redo and f.want["status"] != dm.OK for f in sets["kats"])          # the filter byte above 4


@pytest.mark.parametrize("sub", ppc.SUBS)
def test_mixed_batch(ctx, sub):
    """damaged files between clean neighbours of their size and kind, one call"""
    clean = [c for c in ppc.corpus() if c.tags and c.tags[0] == "level"]
    twins = ppc.damaged([clean[1]] * 3, 77)
    files = [File(c.name, c.data, damage=c.damage, fast=not c.damage) for c in (clean[0], twins[0], clean[1], twins[1], clean[2], twins[2], clean[0])]
    blobs = [f.data for f in files]
    with env():
        ref, ref_st = ctx.png_decode_batch(blobs)
    before = ctx.png_decode_counts()
    with env(IPX_PNG_PAR=1, IPX_PNG_PAR_SUB=sub):
        info, st = ctx.png_decode_batch(blobs)
    d = [a - b for a, b in zip(ctx.png_decode_counts(), before)]
    assert st == ref_st == [f.want["status"] for f in files] == [dm.OK, dm.INVALID] * 3 + [dm.OK]
    for i, f in enumerate(files):
        if st[i] == dm.OK:
            np.testing.assert_array_equal(info["pix"][i], f.want["pix"], err_msg=f.name)
            np.testing.assert_array_equal(info["pix"][i], ref["pix"][i], err_msg=f.name)
    runs = [f.counts(sub) for f in files if not f.damage]
    assert d == [7, 4, 3, sum(r[0] for r in runs), sum(r[1] for r in runs)]


@pytest.mark.parametrize("value", [None, "0", "2", "true"])
def test_other_values_leave_everything_as_it_was(ctx, sets, unset, value):
    files = [f for f in sets["par"] if f.tags and f.tags[0] in ("parts", "budget-lone", "far", "level")]
    assert len(files) >= 8                                               # clean files and damaged twins
    before = ctx.png_decode_counts()
    for f in files:
        with env(IPX_PNG_PAR=value, IPX_PNG_PAR_SUB=48):
            info, st = ctx.png_decode_batch([f.data])
        assert st == unset["par", f.name][1] == [f.want["status"]], f.name
        _same(info, unset["par", f.name][0], f.name)
    assert ctx.png_decode_counts() == before


def test_the_switch_is_read_on_every_call(ctx, sets, unset):
    f = next(f for f in sets["par"] if f.tags and f.tags[0] == "same-round" and not f.damage)
    c0 = ctx.png_decode_counts()
    with env(IPX_PNG_PAR=1):
        a = ctx.png_decode_batch([f.data])
    c1 = ctx.png_decode_counts()
    with env():
        b = ctx.png_decode_batch([f.data])
    c2 = ctx.png_decode_counts()
    with env(IPX_PNG_PAR=1):
        c = ctx.png_decode_batch([f.data])
    c3 = ctx.png_decode_counts()
    assert c1[0] - c0[0] == 1 and c2 == c1 and c3[0] - c2[0] == 1 and c3[3] - c2[3] == c1[3] - c0[3] > 0
    for got in (a, b, c):
        assert got[1] == [dm.OK]
        _same(got[0], unset["par", f.name][0], f.name)


def test_counts_start_at_zero_and_refuse_a_null_argument(ctx):
    import imageprocessor_amd as m
    with m.Context(lanes=1) as fresh:
        assert fresh.png_decode_counts() == [0] * 5
        assert m.lib().ipx_png_decode_counts(fresh.handle, None) == dm.INVALID
    assert m.lib().ipx_png_decode_counts(None, None) == dm.INVALID
