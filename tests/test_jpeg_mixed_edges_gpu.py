"""ipx_jpeg_decode_mixed and ipx_run_jpeg_jpeg_mixed at their record, search and cut edges (tests/mixed_edge_cases.py builds the inputs,
tests/test_mixed_edge_cases.py proves on the CPU that they reach the edges).

Decode: the engineered corpora that so far ran one shape per call -- tests/jpeg_par_corpus.py and tests/jpeg_edge_corpus.py -- in ONE
mixed call each, so that a scan with more blocks than its frame, a short scan or a cut one stands in the slot before an image of
another shape, and the parallel passes' rows (max_nsub) are used very unequally; the host route's pinned halves with groups of unequal
sizes, with and without the lane's arena.  Statuses and planes byte for byte against the oracle and tests/jpeg_decode_model.py.

Leg: every sampling class the entry takes, baseline and progressive; scan failures at the first and the last file of a run; per-file
texts where an output is encoded per chunk; a file whose plan makes an empty output.  Streams byte for byte against
ipx_plan_run_jpeg_jpeg per size and class, a few also against the oracle's decoder, operators and encoder."""
import numpy as np
import pytest

import mixed_edge_cases as mx
import oracle
from test_jpeg_decode_edges_gpu import PATH_IDS, PATHS, model
from test_jpeg_mixed_gpu import (INVALID, LEG_ENVS, LEG_SIZES, OUTS, QUALITY, UNSUPPORTED, alone, clear_env, leg_glyphs, leg_text, make, ops_of,
                                 oracle_of, same_planes, uniform_leg)
from test_jpeg_par_edges_gpu import want

pytestmark = pytest.mark.gpu

DEC_ENVS = ("IPX_JPEG_PAR_SUB", "IPX_JPEG_PAR_STAGE", "IPX_JPEG_PAR", "IPX_JPEG_PAR_ROUNDS", "IPX_JPEG_PIECE", "IPX_JPEG_SHARED_TABLES",
            "IPX_JPEG_HOST_GROUP", "IPX_JPEG_LANE_ARENA", "IPX_JPEG_PROG_GPU", "IPX_JPEG_411", "IPX_JPEG_CMYK")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


def setenv(monkeypatch, env):
    for k in DEC_ENVS + LEG_ENVS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- A. decode -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def par_cases():
    return mx.par_corpus()


def planes_of(c):
    """a decodable case's planes: the oracle's and the model's (held to agree) for the engineered files, the oracle's for Pillow's"""
    if c.props.get("pillow"):
        d = oracle_of(c.data)
        return {"y": d["y"]}
    return want(c)


def check_call(ctx, cases, what):
    """one mixed call over the cases in this order: every status the case's, every decodable file's planes its reference's over the
    MCU-padded extent, every other frame absent; all the files that miss are named"""
    frames, st = ctx.jpeg_decode_mixed([c.data for c in cases])
    missed = []
    for i, c in enumerate(cases):
        if st[i] != c.status:
            missed.append("%s (%d of %s): status %d, not %d" % (c.name, i, what, st[i], c.status))
        elif c.status != 0:
            if frames[i] is not None:
                missed.append("%s (%d of %s): a frame beside status %d" % (c.name, i, what, st[i]))
        else:
            if (frames[i]["w"], frames[i]["h"], frames[i]["ratio"]) != (c.w, c.h, c.ratio):
                missed.append("%s (%d of %s): %r" % (c.name, i, what, (frames[i]["w"], frames[i]["h"], frames[i]["ratio"])))
                continue
            for k, w in planes_of(c).items():
                g = frames[i][k]
                if g.shape != w.shape:
                    missed.append("%s (%d of %s): plane %s is %r, not %r" % (c.name, i, what, k, g.shape, w.shape))
                elif not np.array_equal(g, w):
                    bad = np.argwhere(g != w)
                    missed.append("%s (%d of %s): plane %s differs in %d bytes, first at row %d column %d" % (c.name, i, what, k, len(bad), bad[0][0], bad[0][1]))
    if missed:
        pytest.fail("\n".join(missed))
    return st


A1_ENVS = [{}, {"IPX_JPEG_PAR_SUB": "128"}, {"IPX_JPEG_PAR_SUB": "1024"}, {"IPX_JPEG_PAR": "0"}, {"IPX_JPEG_PAR": "0", "IPX_JPEG_PIECE": "0"}]
A1_IDS = ["sub-unset", "sub-128", "sub-1024", "pieces", "bytewise"]


@pytest.mark.parametrize("env", A1_ENVS, ids=A1_IDS)
def test_the_par_corpus_in_one_call(ctx, par_cases, monkeypatch, env):
    """A1.  The 54 files of tests/jpeg_par_corpus.py (31 shapes, four classes) and one long Gray file in one call, in corpus order and
    in an order that alternates the classes and puts every over-long, short and cut scan in the slot before a decodable image of
    another shape: the write guards of the MIXED kernels come from the image's own record, so the neighbour's coefficients stay its own.
    The Gray scans run from 4096 to 159 442 bytes (38 x) in one launch set.  Under the default the route counter shows that the files
    reached the GPU's Huffman kernels."""
    setenv(monkeypatch, env)
    before = ctx.jpeg_decode_counts()
    check_call(ctx, par_cases, "corpus order")
    grown = [a - b for a, b in zip(ctx.jpeg_decode_counts(), before)]
    if not env:
        routes = [ctx.jpeg_scan_route(c.data) for c in par_cases]
        assert all(r == (0, ctx.JPEG_ROUTE_PAR) for r, c in zip(routes, par_cases) if c.par)
        assert sum(c.par for c in par_cases) >= 50
        # every file the marker parser takes reaches route 0, and no other route is used
        assert sum(c.par for c in par_cases) <= grown[0] <= sum(1 for st, _ in routes if st == 0) and grown[1:] == [0, 0, 0], grown
    check_call(ctx, mx.interleaved(par_cases), "interleaved order")


@pytest.mark.parametrize("seed", [1, 2])
def test_the_par_corpus_in_any_order(ctx, par_cases, monkeypatch, seed):
    """A3: a seeded shuffle of A1's call: per file the same statuses and planes (those of its references)"""
    setenv(monkeypatch, {})
    perm = mx.shuffled(par_cases, seed)
    assert perm != sorted(perm)
    check_call(ctx, [par_cases[p] for p in perm], "shuffle %d" % seed)


@pytest.fixture(scope="module")
def edge_files():
    return mx.edge_mix()


SWITCHED_ON = {"IPX_JPEG_PROG_GPU": "1", "IPX_JPEG_411": "1", "IPX_JPEG_CMYK": "1"}


@pytest.mark.parametrize("env", PATHS + [SWITCHED_ON], ids=PATH_IDS + ["opt-in-switches-set"])
def test_the_edge_corpus_in_one_call(ctx, edge_files, monkeypatch, env):
    """A2.  tests/jpeg_edge_corpus.py (4:4:0 included) with a Pillow file per class in one call, by the status contract of
    tests/test_jpeg_decode_edges_gpu.py: -1 <-> the model says malformed; -4 <- the model says unsupported (and the file is not
    progressive) or a DC value beyond int16; else 0 and every plane the oracle's and the model's.  include/ipx.h keeps the GPU scan
    walk, 4:1:1, 4:1:0 and four-component files out of this entry whatever the switches say: with the three switches set the
    answers are the same, and the multi-scan files still go to the host route (the scan walk's counter stands still)."""
    setenv(monkeypatch, env)
    before = ctx.jpeg_decode_counts()
    frames, st = ctx.jpeg_decode_mixed([f for _, f in edge_files])
    grown = [a - b for a, b in zip(ctx.jpeg_decode_counts(), before)]
    assert grown[1] >= 4 and grown[2:] == [0, 0], grown              # (four files of the corpus have several scans)
    missed, oks = [], 0
    for i, (name, f) in enumerate(edge_files):
        verdict, m = model(f)
        o = None
        if verdict == "malformed":
            expect = INVALID
        elif verdict == "unsupported" and b"\xff\xc2" not in f:
            expect = UNSUPPORTED
        else:
            o = oracle.jpeg_decode(f)
            expect = UNSUPPORTED if o["dc_wide"] else 0
        if st[i] != expect:
            missed.append("%s: status %d, not %d" % (name, st[i], expect))
            continue
        if expect != 0:
            assert frames[i] is None, name
            continue
        oks += 1
        for k in ("y", "cb", "cr") if o["ratio"] != 4 else ("y",):
            for ref, who in ((o, "oracle"), (m, "model")):
                if ref is not None and not (frames[i][k].shape == ref[k].shape and np.array_equal(frames[i][k], ref[k])):
                    missed.append("%s: plane %s differs from the %s's" % (name, k, who))
    if missed:
        pytest.fail("\n".join(missed))
    assert oks >= 30 and {frames[i]["ratio"] for i in range(len(st)) if st[i] == 0} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("arena", [None, "0"], ids=["lane-arena", "stream-ordered"])
@pytest.mark.parametrize("group", ["1", "2", "16"])
@pytest.mark.parametrize("reverse", [False, True], ids=["in-order", "reversed"])
def test_host_route_halves(ctx, monkeypatch, reverse, group, arena):
    """A4.  Five progressive files of (17 x 17, 257 x 40, 64 x 48, 200 x 120, 33 x 15) in one class with two baseline files between
    them: dec_upload stages each group of IPX_JPEG_HOST_GROUP files in one half of a pinned block sized for the largest group, at
    offsets that start again with every group.  At 2 the groups hold 21 450, 45 240 and 1170 words: the largest is not the first."""
    files, host = mx.host_route_files(reverse)
    setenv(monkeypatch, {})
    refs = [alone(ctx, f) for f in files]
    assert [s for _, s in refs] == [0] * 7
    env = {"IPX_JPEG_HOST_GROUP": group}
    if arena is not None:
        env["IPX_JPEG_LANE_ARENA"] = arena
    setenv(monkeypatch, env)
    before = ctx.jpeg_decode_counts()
    frames, st = ctx.jpeg_decode_mixed(files)
    grown = [a - b for a, b in zip(ctx.jpeg_decode_counts(), before)]
    assert st == [0] * 7 and grown == [2, 5, 0, 0], (st, grown)
    for i, f in enumerate(files):
        same_planes(frames[i], refs[i][0], "file %d against the uniform entry" % i)
        same_planes(frames[i], oracle_of(f), "file %d against the oracle" % i)


# ---- B. the leg ------------------------------------------------------------------------------------------------------------------

def chroma_shape(w, h, ratio):
    return {0: (h, w), 1: (h, (w + 1) // 2), 2: ((h + 1) // 2, (w + 1) // 2), 3: ((h + 1) // 2, w)}[ratio]


@pytest.fixture(scope="module")
def classes_case(ctx):
    from helpers import DEFAULT_COL
    files, sizes = mx.leg_classes_case()
    gs = ctx.glyphset(leg_glyphs(), DEFAULT_COL)
    try:
        ref = {ka: uniform_leg(ctx, files, sizes, ka, glyphset=gs) for ka in (False, True)}
    finally:
        gs.close()
    return files, sizes, ref


@pytest.mark.parametrize("env", [{}, {"IPX_JPEG_MIXED_GROUP": "3", "IPX_JPEG_MIXED_CHUNK_MB": "0"}], ids=["default-budgets", "groups-of-three-chunk-per-file"])
@pytest.mark.parametrize("keep_aspect", [False, True], ids=["encode-per-chunk", "encode-per-run"])
def test_leg_every_class(ctx, classes_case, monkeypatch, keep_aspect, env):
    """B1.  {Gray, 4:2:0, 4:2:2, 4:4:0, 4:4:4} x {33 x 15, 64 x 48} x {baseline, progressive}, interleaved: Gray runs read a source
    without chroma planes (cstride and the chroma frame stride 0), progressive files come from the host route inside a decode group.
    A class the uniform leg refuses carries the same status and no stream.  Four YCbCr files also against the oracle."""
    from helpers import DEFAULT_COL
    from test_sources_gpu import _expect_ycbcr_ops
    files, sizes, ref = classes_case
    want_out, want_st = ref[keep_aspect]
    setenv(monkeypatch, env)
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(keep_aspect, (leg_glyphs(), DEFAULT_COL)), files, quality=QUALITY)
    assert st == want_st
    assert sum(s == 0 for s in st) >= 16                  # (the YCbCr classes at the least)
    for k in OUTS:
        for i in range(20):
            if st[i] != 0:
                assert got[k][i] is None, (k, i, sizes[i])
            else:
                assert got[k][i] is not None and got[k][i] == want_out[k][i], (k, i, sizes[i])
    for i in (1, 7, 13, 19):                               # 4:2:0, 4:2:2, 4:4:0 and 4:4:4; the last two progressive
        assert st[i] == 0
        (w, h), d = sizes[i][:2], oracle.jpeg_decode(files[i])
        ch, cw = chroma_shape(w, h, d["ratio"])
        exp = _expect_ycbcr_ops(np.ascontiguousarray(d["y"][:h, :w]), np.ascontiguousarray(d["cb"][:ch, :cw]), np.ascontiguousarray(d["cr"][:ch, :cw]),
                                d["ratio"], (64, 48, keep_aspect), (32, True), leg_glyphs(), DEFAULT_COL)
        for k in OUTS:
            assert got[k][i] == oracle.jpeg_encode_rgba(exp[k], QUALITY), (k, i, sizes[i])
    assert {oracle.jpeg_decode(files[i])["ratio"] for i in (1, 7, 13, 19)} == {0, 1, 2, 3}


_RUN_REF = {}


def run_ref(ctx, variant, keep_aspect):
    if (variant, keep_aspect) not in _RUN_REF:
        files, sizes, bad, run = mx.run_ends_case(variant)
        _RUN_REF[variant, keep_aspect] = uniform_leg(ctx, files, sizes, keep_aspect), [alone(ctx, files[i])[1] for i in bad]
    return _RUN_REF[variant, keep_aspect]


@pytest.mark.parametrize("env", [{}, {"IPX_JPEG_MIXED_GROUP": "2"}], ids=["one-group", "group-boundary-in-the-run"])
@pytest.mark.parametrize("keep_aspect", [False, True], ids=["encode-per-chunk", "encode-per-run"])
@pytest.mark.parametrize("variant", list(mx.RUN_VARIANTS))
def test_leg_scan_failures_at_the_ends_of_a_run(ctx, monkeypatch, variant, keep_aspect, env):
    """B2.  Four 129 x 65 files (one run) between runs of 64 x 48 and 200 x 120; the run's first file, its last, or all but one fail in
    the scan.  A run starts from its first file's planes and takes its planes one frame stride apart: with the first file failed the
    files run one by one; with keep_aspect = 0 the chunk's one encode meets the failed file's frame, which nobody wrote, and drops it."""
    files, sizes, bad, run = mx.run_ends_case(variant)
    setenv(monkeypatch, {})
    (want_out, want_st), alone_st = run_ref(ctx, variant, keep_aspect)
    assert all(s != 0 for s in alone_st) and [want_st[i] for i in bad] == alone_st
    setenv(monkeypatch, env)
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(keep_aspect), files, quality=QUALITY)
    assert st == want_st and [i for i in range(8) if st[i] != 0] == bad
    for k in OUTS:
        for i in range(8):
            if i in bad:
                assert got[k][i] is None and want_out[k][i] is None, (k, i)
            else:
                assert got[k][i] is not None and got[k][i] == want_out[k][i], (k, i, sizes[i])


@pytest.fixture(scope="module")
def texts_case(ctx):
    """twelve files of six sizes and two classes with a text each, and the uniform texts leg's streams with keep_aspect = 0"""
    import imageprocessor_amd as ipx
    files, sizes = [], []
    for i in range(12):
        w, h = LEG_SIZES[i % 6]
        cls = ("420", "444")[(i // 3) % 2]
        files.append(make(w, h, cls, seed=1000 + i))
        sizes.append((w, h, cls))
    texts = [leg_text(ipx, i, w, h) for i, (w, h, _) in enumerate(sizes)]
    return files, sizes, texts, uniform_leg(ctx, files, sizes, False, texts=texts), uniform_leg(ctx, files, sizes, False)


@pytest.mark.parametrize("env", [{}, {"IPX_JPEG_MIXED_GROUP": "2"}, {"IPX_JPEG_MIXED_CHUNK_MB": "0"}, {"IPX_JPEG_MIXED_GROUP": "5", "IPX_JPEG_MIXED_CHUNK_MB": "0"}],
                         ids=["whole", "groups-of-two", "chunk-per-file", "groups-of-five-chunk-per-file"])
def test_leg_texts_where_outputs_are_encoded_per_chunk(ctx, texts_case, monkeypatch, env):
    """B3: a text per file with keep_aspect = 0, under decode groups and chunks that end inside the runs: the text of file i lands on
    file i's watermark whatever group, chunk and run it is in"""
    files, sizes, texts, (want_out, want_st), (plain, _) = texts_case
    drawn = [i for i in range(12) if want_out["watermark"][i] != plain["watermark"][i]]
    print("files whose text changes their watermark stream:", drawn)
    assert want_st == [0] * 12 and len(drawn) >= 6 and want_out["resize"] == plain["resize"]
    setenv(monkeypatch, env)
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(False), files, quality=QUALITY, texts=texts)
    assert st == want_st
    for k in OUTS:
        for i in range(12):
            assert got[k][i] is not None and got[k][i] == want_out[k][i], (k, i, sizes[i])


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_leg_an_empty_output_among_files_that_have_it(ctx, monkeypatch, where):
    """B4.  600 x 1 kept in aspect inside 64 x 48 has a resize output of no rows: has() is false for it, and the chunk's resize outputs,
    otherwise all 64 x 48, are encoded per run instead of per chunk.  The file first, in the middle and last of the chunk's order."""
    files, sizes, at = mx.empty_output_case(where)
    setenv(monkeypatch, {})
    plan = ctx.plan(*mx.EMPTY_SIZE, resize=(64, 48, True), thumbnail=(32, True), watermark=True)
    try:
        assert plan.info.resize_bytes == 0
    finally:
        plan.close()
    want_out, want_st = uniform_leg(ctx, files, sizes, True)
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(True), files, quality=QUALITY)
    assert st == want_st == [0] * 5
    assert got["resize"][at] is None and want_out["resize"][at] is None
    for k in OUTS:
        for i in range(5):
            assert got[k][i] == want_out[k][i], (k, i, sizes[i])
            assert (got[k][i] is None) == (k == "resize" and i == at), (k, i)
