"""The decoder that is parallel inside a scan (csrc/ipx_jpeg_dec_par.hip) on the files of tests/jpeg_par_corpus.py: stuffed pairs on
sub-sequence, word and 16-byte boundaries, dense stuffing, scan lengths on the sub-sequence sizes and the routing threshold, tails and
cuts, boundaries inside long symbols, streams that do not fall into step by themselves, MCU counts on the DC pass's tiles and DC
values at the ends of int16.  Every file through ipx_jpeg_decode_batch at every sub-sequence size, rows staged or not, and through the
piece kernels; statuses and planes byte for byte against tests/jpeg_decode_model.py and the oracle.  The sync rounds the driver reports
are held to the plain-Python restatement of the passes (jpeg_par_corpus.SpecModel)."""
import re

import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_par_corpus as pc
import oracle
from test_jpeg_decode import picture, pil_jpeg

pytestmark = pytest.mark.gpu

SUB_ENVS = [None, "128", "256", "512", "1024"]
ROUND_LINE = re.compile(r"jpeg par sync round (\d+): (\d+) entries changed")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    return pc.corpus()


@pytest.fixture(scope="module")
def by_name(corpus):
    return {c.name: c for c in corpus}


_WANT = {}


def want(c):
    """the planes of a decodable file, from the oracle and the model (which have to agree), once per file"""
    if c.name not in _WANT:
        o, m = oracle.jpeg_decode(c.data), dm.decode(c.data)
        keys = ("y", "cb", "cr") if o["ratio"] != 4 else ("y",)
        for k in keys:
            np.testing.assert_array_equal(o[k], m[k], err_msg="%s: oracle and model differ in %s" % (c.name, k))
        assert bool(o["dc_wide"]) == bool(m["dc_wide"]) == (c.status == -4), c.name
        _WANT[c.name] = {k: o[k] for k in keys}
    return _WANT[c.name]


def setenv(monkeypatch, sub=None, stage=None, **more):
    for k in ("IPX_JPEG_PAR_SUB", "IPX_JPEG_PAR_STAGE", "IPX_JPEG_PAR", "IPX_JPEG_PAR_ROUNDS", "IPX_DEBUG"):
        monkeypatch.delenv(k, raising=False)
    if sub is not None:
        monkeypatch.setenv("IPX_JPEG_PAR_SUB", sub)
    if stage is not None:
        monkeypatch.setenv("IPX_JPEG_PAR_STAGE", stage)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def by_shape(cases):
    out = {}
    for c in cases:
        out.setdefault((c.w, c.h, c.ratio), []).append(c)
    return list(out.values())


def check(ctx, cases, extra=(), missed=None):
    """one call: the cases' files (one geometry) and any extra files behind them.  Every file's status is the case's, every decodable
    file's planes are the oracle's and the model's; all the files that miss are named (a caller that passes `missed` collects them
    over several calls and fails itself).  -> (statuses, planes per decodable case, info)"""
    info, st = ctx.jpeg_decode_batch([c.data for c in cases] + list(extra))
    got, collect = {}, missed is not None
    missed = missed if collect else []
    for i, c in enumerate(cases):
        if st[i] != c.status:
            missed.append("%s: status %d, not %d" % (c.name, st[i], c.status))
        elif c.status == 0:
            got[c.name] = {k: info[k][i] for k in want(c)}
            for k, w in want(c).items():
                if not np.array_equal(got[c.name][k], w):
                    bad = np.argwhere(got[c.name][k][:, :w.shape[1]] != w)
                    missed.append("%s: plane %s differs in %d bytes, first at row %d column %d" % (c.name, k, len(bad), bad[0][0], bad[0][1]))
    if missed and not collect:
        pytest.fail("\n".join(missed))
    return st, got, info


@pytest.mark.parametrize("stage", ["0", "1"], ids=["scan-through-l2", "scan-rows-in-lds"])
@pytest.mark.parametrize("sub", SUB_ENVS, ids=lambda s: "sub-%s" % (s or "unset"))
def test_every_file_at_every_sub_sequence_size(ctx, corpus, monkeypatch, sub, stage):
    setenv(monkeypatch, sub, stage)
    missed = []
    for cases in by_shape(corpus):
        check(ctx, cases, missed=missed)
    if missed:
        pytest.fail("\n".join(missed))


def test_the_piece_kernels_give_the_same(ctx, corpus, monkeypatch):
    """IPX_JPEG_PAR=0 sends the same calls to the piece kernels: identical statuses and planes"""
    for cases in by_shape(corpus):
        setenv(monkeypatch)
        st, got, _ = check(ctx, cases)
        setenv(monkeypatch, IPX_JPEG_PAR="0")
        st0, got0, _ = check(ctx, cases)
        assert st0 == st
        for name in got:
            for k in got[name]:
                np.testing.assert_array_equal(got0[name][k], got[name][k], err_msg="%s plane %s" % (name, k))


@pytest.mark.parametrize("sub", SUB_ENVS, ids=lambda s: "sub-%s" % (s or "unset"))
def test_both_sides_of_the_routing_threshold_give_equal_planes(ctx, by_name, monkeypatch, sub):
    """scans of 4095, 4096 and 4097 stuffed bytes that code the same coefficients: the first goes to the piece kernels"""
    setenv(monkeypatch, sub)
    trio = [by_name["len_%d" % n] for n in (4095, 4096, 4097)]
    for group in (trio, trio[1:], trio[:1]):
        st, got, _ = check(ctx, group)
        assert st == [0] * len(group)
        for c in group:
            np.testing.assert_array_equal(got[c.name]["y"], want(trio[0])["y"])


@pytest.mark.parametrize("stage", ["0", "1"], ids=["scan-through-l2", "scan-rows-in-lds"])
@pytest.mark.parametrize("sub", [None, "128", "1024"], ids=lambda s: "sub-%s" % (s or "unset"))
def test_one_call_mixes_long_short_progressive_and_refused_files(ctx, by_name, monkeypatch, sub, stage):
    """129 sub-sequences beside 32 beside a scan for the piece kernels, a progressive file (the host's scans) and files the host or the
    kernels refuse: sub_off = k * max_nsub, and the lanes of the short files' rows beyond their nsub are dead"""
    setenv(monkeypatch, sub, stage)
    names = ["len_16385", "len_4096", "cut_on_ff_no_eoi", "len_4095", "unstuff_dense", "cut_mid_symbol", "sync_extra_blocks", "tail_behind_rst",
             "len_8064", "unstuff_pairs", "cut_on_ff", "len_16384"]
    cases = [by_name[n] for n in names]
    img = picture(pc.GW, pc.GH, seed=5)[..., 0]
    prog, small = pil_jpeg(img, quality=90, progressive=True), pil_jpeg(img, quality=20)
    assert pc.scan_of(small)[1] < pc.ROUTE_BYTES
    st, _, info = check(ctx, cases, extra=[prog, small])
    assert st[-2:] == [0, 0]
    for i, f in ((len(cases), prog), (len(cases) + 1, small)):
        np.testing.assert_array_equal(info["y"][i], oracle.jpeg_decode(f)["y"])


def test_a_dc_difference_beyond_int16_is_handed_back_by_the_in_scan_route_only(ctx, monkeypatch):
    """known behaviour, not a goal: the values 32767 and -32768 in neighbouring MCUs are 65535 apart.  The piece kernels keep running
    values and decode the file as Go does; the in-scan route stores DC differences in int16 before it sums them, so it answers
    IPX_ERR_UNSUPPORTED and the file goes back to the caller's CPU path -- never wrapped pixels"""
    c = pc.dc_wide_step_case()
    o = oracle.jpeg_decode(c.data)
    assert not o["dc_wide"]
    np.testing.assert_array_equal(o["y"], dm.decode(c.data)["y"])
    setenv(monkeypatch)
    _, st = ctx.jpeg_decode_batch([c.data])
    assert st == [-4]
    setenv(monkeypatch, IPX_JPEG_PAR="0")
    info, st = ctx.jpeg_decode_batch([c.data])
    assert st == [0]
    np.testing.assert_array_equal(info["y"][0], o["y"])


def rounds_reported(capfd):
    return [(int(a), int(b)) for a, b in ROUND_LINE.findall(capfd.readouterr().err)]


ROUND_CASES = ["shared_tables_444", "own_tables_444", "sync_straddles", "unstuff_dense", "len_16385", "dc_tile_2049_bpm6"]


@pytest.mark.parametrize("sub", SUB_ENVS[1:])
@pytest.mark.parametrize("name", ROUND_CASES)
def test_sync_rounds_are_the_predicted_ones(ctx, by_name, monkeypatch, capfd, name, sub):
    """the driver reports, round by round, how many entries changed: the rounds that change one are those of the restated passes (a
    correction crosses one wave boundary per round), and one round that changes none follows"""
    c = by_name[name]
    predicted = pc.SpecModel(c, int(sub)).solve()
    setenv(monkeypatch, sub, IPX_DEBUG="1")
    capfd.readouterr()
    check(ctx, [c])
    lines = rounds_reported(capfd)
    print("%s at %s bytes: predicted %d rounds that change an entry, reported %s" % (name, sub, predicted, lines))
    assert [n for n, _ in lines] == list(range(1, predicted + 2)), (predicted, lines)
    assert all(m > 0 for _, m in lines[:-1]) and lines[-1][1] == 0, (predicted, lines)


def test_a_scan_that_does_not_settle_goes_to_the_bytewise_kernel(ctx, by_name, monkeypatch, capfd):
    """the shared-table file needs 8 rounds at 128 bytes.  With IPX_JPEG_PAR_ROUNDS at 8 or 7 no round reports 0, and every parallel
    image of the call -- the settled ones too -- is handed to the byte-wise kernel; with 9 the scan settles.  The planes are the same."""
    c, twin = by_name["shared_tables_444"], by_name["own_tables_444"]
    r = pc.SpecModel(c, 128).solve()
    assert r >= 3
    for limit, settles in ((r, False), (r - 1, False), (r + 1, True)):
        setenv(monkeypatch, "128", IPX_DEBUG="1", IPX_JPEG_PAR_ROUNDS=str(limit))
        capfd.readouterr()
        check(ctx, [c])
        lines = rounds_reported(capfd)
        assert [n for n, _ in lines] == list(range(1, limit + 1)), (limit, lines)
        assert (lines[-1][1] == 0) == settles and all(m > 0 for _, m in lines[:-1]), (limit, lines)
        # beside files that settle at once
        capfd.readouterr()
        check(ctx, [twin, c, twin])
        lines = rounds_reported(capfd)
        assert (lines[-1][1] == 0) == settles, (limit, lines)
