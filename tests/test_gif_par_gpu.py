"""The parallel GIF code walk on the GPU (csrc/ipx_gif_dec_par.hip, IPX_GIF_PAR=1) through ipx_gif_decode_batch, one call per file: clear
codes at and around the round's 64 lanes, doubled clears, no leading clear, every width step, KwKwK chains as deep as a round and across
rounds, frozen tables and deferred clears, the edge corpus, Pillow's files and the known answers.  Every status, index and palette byte
is the frame the test built, the model's (tests/gif_decode_model.py) and the one of the same call with the switch unset;
ipx_gif_decode_counts shows that the parallel lanes did the work -- a kernel that handed every file to the serial walk would pass every
byte comparison -- and its record count is that of tests/gif_par_model.py."""
import contextlib
import json
import os

import numpy as np
import pytest

import gif_corpus
import gif_decode_model as dm
import gif_edge_corpus as ge
import gif_par_corpus as gpc
import gif_par_model as pm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "gif_dec_kats.json")) as f:
    KATS = json.load(f)
SWITCHES = ("IPX_GIF_PAR", "IPX_GIF_DEC_SCRATCH_MB")


@contextlib.contextmanager
def env(**kw):
    """the switches as given (a missing one unset) for the block; what was there before comes back"""
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


def same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert (a["w"], a["h"]) == (b["w"], b["h"]), what
        np.testing.assert_array_equal(a["index"], b["index"], err_msg=what)
        np.testing.assert_array_equal(a["palettes"], b["palettes"], err_msg=what)


def one(ctx, name, data, idx=None, records=None):
    """the file alone, without and with the switch -> (the rise of the counts, the parallel walk's model or None)"""
    want = dm.decode(data)
    reaches = want["stage"] != "container" and dm.entry_status(want) != dm.UNSUPPORTED
    par = None
    if reaches and records is None:
        par = pm.par_walk(pm.stream_of(data))
        records = None if par.redo else len(par.records)
    with env():
        ref, ref_st = ctx.gif_decode_batch([data])
    before = ctx.gif_decode_counts()
    with env(IPX_GIF_PAR=1):
        got, st = ctx.gif_decode_batch([data])
    d = [a - b for a, b in zip(ctx.gif_decode_counts(), before)]
    assert st == ref_st == [dm.entry_status(want)], (name, want["error"])
    if st == [dm.OK]:
        same(got, ref, name)
        np.testing.assert_array_equal(got["index"][0], want["index"], err_msg=name)
        np.testing.assert_array_equal(got["palettes"][0], want["palette"], err_msg=name)
        if idx is not None:
            np.testing.assert_array_equal(got["index"][0], idx, err_msg=name)
    if not reaches:
        assert d == [0, 0, 0, 0], (name, d)
    elif records is None:
        assert d == [1, 0, 1, 0], (name, d)
    else:
        assert st == [dm.OK] and d == [1, 1, 0, records], (name, d, records)
    return d, par


def accepted(ctx, case):
    name, data, idx = case[:3]
    d, _ = one(ctx, name, data, idx)
    assert d[1] == 1, (name, d)


# ---- round edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 2, 63, 64, 65, 127, 128, 300])
def test_a_clear_every_n_codes(ctx, every):
    """the clear code in every lane position relative to the round: 64 puts it in lane 0 of every other round, 63 and 65 walk it
    through the lanes"""
    for k, (lit, bits, kind) in enumerate(((8, 8, "noise"), (3, 3, "runs"))):
        accepted(ctx, ge.make("every %d lit %d" % (every, lit), 160, 120, bits, lit, 40 + every + k, kind, clear="every", every=every,
                              interlace=bool(k)))


@pytest.mark.parametrize("kw", [dict(clear="every", every=64, double=True), dict(clear="full", double=True), dict(clear="full", lead=False),
                                dict(clear="never", lead=False), dict(clear="every", every=65, lead=False, double=True)],
                         ids=lambda kw: " ".join("%s=%s" % i for i in kw.items()))
def test_doubled_clears_and_no_leading_clear(ctx, kw):
    accepted(ctx, ge.make("noise %s" % kw, 160, 120, 8, 8, 61, "noise", **kw))
    accepted(ctx, ge.make("photo %s" % kw, 160, 120, 5, 5, 62, "photo", sub="random", **kw))


@pytest.mark.parametrize("lit,bits", [(2, 2), (2, 1), (3, 3), (8, 8), (8, 3)])
def test_width_steps(ctx, lit, bits):
    """lit 2 and 3: every width step 3 .. 12 falls inside the first 4095 ordinals, several of them on no round boundary
    (step to width x at ordinal (1 << (x - 1)) - eof: 3, 11, 27, 59, 123, ... for lit 2)"""
    for k, pol in enumerate((dict(clear="full"), dict(clear="never"), dict(clear="full", lead=False))):
        name, data, idx, _, _ = ge.make("lit %d %s" % (lit, pol), 160, 120, bits, lit, 70 + k, ("noise", "photo", "noise")[k], **pol)
        d, par = one(ctx, name, data, idx)
        assert d[1] == 1 and max(t0 + nv for t0, nv, _, _ in par.trace) > 2048, name     # a segment that reaches width 12


# ---- KwKwK chains ------------------------------------------------------------------------------------------------------------------
def test_kwkwk_chain_as_deep_as_a_round(ctx):
    """a one-colour frame: every code is KwKwK of the one before -- lane 63's length hangs on lane 62's, ... on lane 0's"""
    import lzw_writer as lw
    for lit, colour in ((2, 0), (8, 200), (5, 31)):
        idx = np.full((120, 160), colour, np.uint8)
        data, _ = lw.gif(idx, gpc.palette(1 << lit, lit), lit=lit, clear="never")
        d, par = one(ctx, "one colour lit %d" % lit, data, idx)
        codes = [r[2] & 4095 for r in par.records]
        assert d[1] == 1 and len(codes) > 128 and all(b == a + 1 for a, b in zip(codes[1:-1], codes[2:-1]))    # (the last: what is left)


@pytest.mark.parametrize("lit,bits", [(8, 8), (4, 4), (2, 2)])
def test_kwkwk_chains_across_rounds(ctx, lit, bits):
    for pol in (dict(clear="full"), dict(clear="never"), dict(clear="every", every=100)):
        accepted(ctx, ge.make("runs lit %d %s" % (lit, pol), 160, 120, bits, lit, 81, "runs", **pol))


# ---- the frozen table, a deferred clear ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lit,bits,kw", [(8, 8, dict(clear="never")), (2, 2, dict(clear="never")), (8, 8, dict(clear="every", every=6000))],
                         ids=["lit 8 never", "lit 2 never", "every 6000"])
def test_frozen_table_and_deferred_clear(ctx, lit, bits, kw):
    name, data, idx, _, frozen = ge.make("frozen %s" % kw, 256, 200, bits, lit, 91, "noise", **kw)
    assert frozen > 1500
    d, par = one(ctx, name, data, idx)
    assert d[1] == 1 and any((1 << lit) + 1 + t0 + nv > 4200 for t0, nv, _, _ in par.trace)


# ---- the corpora, every file alone -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_corpus():
    return ge.corpus()


@pytest.mark.parametrize("part", range(4))
def test_edge_corpus(ctx, edge_corpus, part):
    for case in edge_corpus[part::4]:
        accepted(ctx, case)


def test_pillow_corpus(ctx):
    for name, data in gif_corpus.corpus():
        d, _ = one(ctx, name, data)
        assert d[1] == 1, name


def test_known_answers(ctx):
    rises = {k["name"]: one(ctx, k["name"], bytes.fromhex(k["data"]))[0] for k in KATS}
    assert sum(d[1] for d in rises.values()) >= 10 and sum(d[2] for d in rises.values()) >= 5
    assert any(d == [0, 0, 0, 0] for d in rises.values())               # refused by the container parser: never walked


# ---- the switch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [None, "0", "2", "true"])
def test_other_values_leave_everything_as_it_was(ctx, value):
    cases = [ge.make("value %s #%d" % (value, k), 160, 120, 8, 8, 50 + k, ("noise", "runs", "photo")[k], clear=("full", "never", "every")[k],
                     every=64) for k in range(3)]
    before = ctx.gif_decode_counts()
    for name, data, idx, _, _ in cases:
        with env():
            ref = ctx.gif_decode_batch([data])
        with env(IPX_GIF_PAR=value):
            got = ctx.gif_decode_batch([data])
        assert got[1] == ref[1] == [dm.OK], name
        same(got[0], ref[0], name)
        np.testing.assert_array_equal(got[0]["index"][0], idx, err_msg=name)
    assert ctx.gif_decode_counts() == before


def test_the_switch_is_read_on_every_call(ctx):
    name, data, idx, _, _ = ge.make("now and then", 160, 120, 8, 8, 55, "photo", clear="full")
    c0 = ctx.gif_decode_counts()
    with env(IPX_GIF_PAR=1):
        a = ctx.gif_decode_batch([data])
    c1 = ctx.gif_decode_counts()
    with env():
        b = ctx.gif_decode_batch([data])
    c2 = ctx.gif_decode_counts()
    with env(IPX_GIF_PAR=1):
        c = ctx.gif_decode_batch([data])
    c3 = ctx.gif_decode_counts()
    assert c1[0] - c0[0] == 1 and c2 == c1 and c3[0] - c2[0] == 1 and c3[3] - c2[3] == c1[3] - c0[3] > 0
    for got in (a, b, c):
        assert got[1] == [dm.OK]
        np.testing.assert_array_equal(got[0]["index"][0], idx)


def test_counts_start_at_zero_and_refuse_a_null_argument(ctx):
    import imageprocessor_amd as m
    with m.Context(lanes=1) as fresh:
        assert fresh.gif_decode_counts() == [0] * 4
        assert m.lib().ipx_gif_decode_counts(fresh.handle, None) == dm.INVALID
    assert m.lib().ipx_gif_decode_counts(None, None) == dm.INVALID
