"""The edge corpora of the PNG and GIF encoders (tests/png_encode_corpus.py, tests/gif_encode_corpus.py) on the CPU: every case has the
property it is there for (the measured figure is printed: run with -s), and the models the GPU is held to agree with the independent
references on the whole corpus -- the plain per-byte filter loop and zlib for png_model, the reader of compress/lzw and Pillow for
gif_model, the per-pixel trace of drawPaletted for both forms of the dither.  The last tests break the models the way a kernel could
be broken and see a property or an independent check notice."""
import zlib

import numpy as np
import pytest

import gif_encode_corpus as gc
import gif_model as gm
import png_encode_corpus as pc
import png_model as pm


# ---- PNG -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reports():
    cache = {}

    def get(rec):
        if rec not in cache:
            cache[rec] = pc.report(pc.frame(*rec))
        return cache[rec]
    return get


@pytest.mark.parametrize("name,rec,prop", pc.CASES, ids=[c[0] for c in pc.CASES])
def test_png_case_has_its_property(reports, name, rec, prop):
    ok, figure = pc.PROPERTIES[prop](reports(rec))
    print("%s %r: %s" % (name, rec, figure))
    assert ok, figure


def test_png_no_frame_reaches_the_distance_limit(reports):
    """said in the corpus' docstring and in DESIGN.md: the deepest distance tree of the corpus stays within the limit"""
    deepest = max(g.depth_dist for _, rec, _ in pc.CASES for g in reports(rec))
    print("deepest distance tree without the limit: %d" % deepest)
    assert deepest <= pm.LIMIT_LITLEN


def _all_png_frames():
    out = [pc.frame(*rec) for rec in pc.recipes()]
    for k in range(len(pc.BATCHES)):
        out += pc.batch_frames(k)
    return out + [f for _, f in pc.kat_frames()]


def test_png_model_agrees_with_the_plain_loop_and_zlib():
    """the filtered stream of png_model is the plain loop's, and zlib inflates the model's stream to it"""
    for f in _all_png_frames():
        bpp, types, want = pc.reference(f)
        mbpp, w, h, data = pm.filtered_stream(f)
        assert (mbpp, data.tobytes()) == (bpp, want), f.shape
        pc.check_stream(pc.model_stream(f), f)
        assert len(pc.model_stream(f)) <= pm.stream_bound(w, h, bpp)
    f = pc.frame("aba", 5462, 5, 1)
    assert len(pc.model_stream(f)) == pm.stream_bound(5462, 5, 3) == 82025


def test_png_filter_cases():
    """every filter takes a row on its own, and every tie between neighbours of Go's order goes to the earlier one"""
    names = {0: "None", 1: "Sub", 2: "Up", 3: "Average", 4: "Paeth"}
    ties = set()
    for name, rec, row, tie in pc.FILTER_CASES:
        f = pc.frame(*rec)
        _, types, _, scores = pc.plain_filter(f, want_scores=True)
        lo = min(scores[row].values())
        assert tuple(t for t in pc.GO_ORDER if scores[row][t] == lo) == tie, name
        assert types[row] == tie[0], name
        assert " = ".join(names[t] for t in tie) == name
        print("%s %r row %d: scores %s" % (name, rec, row, {names[t]: scores[row][t] for t in pc.GO_ORDER}))
        ties.add(tie)
    assert ties == {(t,) for t in range(5)} | {(pc.GO_ORDER[i], pc.GO_ORDER[i + 1]) for i in range(4)}


def test_png_kats_against_the_plain_loop():
    for case, f in pc.kat_frames():
        bpp, types, stream = pc.plain_filter(f)
        n = 1 + case["w"] * bpp
        assert (bpp, types) == (case["bpp"], case["types"]), case["name"]
        assert [list(stream[y * n + 1:(y + 1) * n]) for y in range(case["h"])] == case["filtered"], case["name"]


# ---- GIF -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(gc.lzw_cases())), ids=[c[0] for c in gc.lzw_cases()])
def test_gif_lzw_case_has_its_property(k):
    name, idx, prop = gc.lzw_cases()[k]
    ok, figure = prop(gc.trace_lzw(idx), idx.size)
    print("%s: %s" % (name, figure))
    assert ok, figure


def test_gif_index_frames_dither_to_their_indices():
    """drawPaletted line by line (dither_scalar) returns the indices of every LZW case; the batch frames go through dither_wavefront.  (Why: each palette colour picks
    its own index and leaves no error in any channel, so no pixel of such a frame ever sees an error term.)"""
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    idx, clamps, ties = gc.trace_dither(gc.index_frame(every))
    assert (idx == every).all() and ties == 0 and clamps == {"low": [0] * 4, "high": [0] * 4}
    for name, idx, _ in gc.lzw_cases():
        np.testing.assert_array_equal(gm.dither_scalar(gc.index_frame(idx)), idx, err_msg=name)
    for _, _, frames in gc.lzw_batches():
        for idx in frames:
            np.testing.assert_array_equal(gm.dither_wavefront(gc.index_frame(idx)), idx)    # held to the trace below


def test_gif_model_agrees_with_the_reader_and_pillow():
    """the model's streams decode to the indices; the trace's byte count is the model's; the known answers are the model's data"""
    hexes = {"kat: " + c["name"]: c["lzw_hex"] for c in gc.kats()}
    frames = [(n, i) for n, i, _ in gc.lzw_cases()] + [("batch", i) for _, _, fr in gc.lzw_batches() for i in fr]
    for name, idx in frames:
        stream = gm.encode_index(idx)
        gc.check_stream(stream, idx)
        data, sizes = gc.lzw_payload(stream, idx.shape[1], idx.shape[0])
        assert len(data) == gc.trace_lzw(idx)["nbytes"], name
        assert len(stream) <= gm.size_bound(idx.shape[1], idx.shape[0]), name
        if name in hexes:
            assert data.hex() == hexes[name], name
    # the three endings of the last sub-block
    for r, n in gc.RESIDUE_PREFIX.items():
        _, sizes = gc.lzw_payload(gm.encode_index(gc.no_repeats()[:n].reshape(1, -1)), n, 1)
        assert sizes[-1] == (r or 255)


@pytest.mark.parametrize("k", range(len(gc.dither_cases())), ids=[c[0] for c in gc.dither_cases()])
def test_gif_dither_case(k):
    """both forms of the model's dither are the per-pixel trace; the extremes reach every clamp that can fire"""
    name, f, _ = gc.dither_cases()[k]
    idx, clamps, ties = gc.trace_dither(f)
    print("%s: sums below 0 %s, above 0xffff %s (r g b a), %d ties" % (name, clamps["low"], clamps["high"], ties))
    np.testing.assert_array_equal(gc.dither_reference(k), idx)
    np.testing.assert_array_equal(gm.dither_wavefront(f), idx)
    assert clamps["high"][3] == 0            # the alpha error is never positive
    if name.startswith("extremes"):
        assert min(clamps["low"]) > 0 and min(clamps["high"][:3]) > 0
    if name.startswith("tie"):
        assert ties > 0
    gc.check_stream(gm.encode_index(idx), idx)


def test_gif_tie_colours_go_to_the_first_entry():
    frames, first = gc.tie_frames()
    assert len(frames) >= 100
    for f, want in zip(frames, first):
        idx, _, ties = gc.trace_dither(f)
        assert ties == 1 and idx[0, 0] == want
        assert gm.dither_scalar(f)[0, 0] == want


# ---- the models, broken the way a kernel could be --------------------------------------------------------------------------------
def test_broken_code_length_limit_is_noticed(monkeypatch):
    """without the limit of 7 the code-length code has a length of 8, which three bits cannot say: no inflater takes the stream"""
    f = pc.frame("fib", 252, 172, 0)
    monkeypatch.setattr(pm, "LIMIT_CL", 64)
    stream = pm.png_encode(f)
    with pytest.raises((zlib.error, AssertionError)):
        pc.check_stream(stream, f)


def test_broken_literal_limit_is_noticed(monkeypatch):
    """without the limit of 15 a literal has a length of 16, which the code-length alphabet cannot say"""
    f = pc.frame("fib", 109, 286, 0)
    monkeypatch.setattr(pm, "LIMIT_LITLEN", 64)
    stream = pm.png_encode(f)
    with pytest.raises((zlib.error, AssertionError)):
        pc.check_stream(stream, f)


def test_broken_window_test_is_noticed(monkeypatch):
    """2 * stride < window instead of <=: the tokens at distance 32768 are gone"""
    monkeypatch.setattr(pm, "WINDOW", 32767)
    ok, figure = pc.PROPERTIES["distance 32768"](pc.report(pc.frame("aba", 5461, 5, 1)))
    assert not ok, figure


def _literal_stream(seq, final_inc_hi=True):
    """the writer's data for a sequence that never matches, from the width schedule alone (golden/make_gif_kats.py), with the incHi of
    Close left out on request"""
    width, hi, overflow = 9, 257, 512
    codes = [(256, 9)]

    def inc_hi():
        nonlocal width, hi, overflow
        hi += 1
        if hi == overflow:
            width += 1
            overflow <<= 1
        if hi == 4095:
            codes.append((256, width))
            width, hi, overflow = 9, 257, 512
    for v in seq[:-1]:
        codes.append((int(v), width))
        inc_hi()
    codes.append((int(seq[-1]), width))
    if final_inc_hi:
        inc_hi()
    codes.append((257, width))
    bits = nbits = 0
    out = bytearray()
    for c, wd in codes:
        bits |= c << nbits
        nbits += wd
        while nbits >= 8:
            out.append(bits & 0xFF)
            bits >>= 8
            nbits -= 8
    if nbits:
        out.append(bits & 0xFF)
    return bytes(out)


def test_broken_inc_hi_at_close_is_noticed():
    """N = 3838: without the incHi of Close no clear goes out and EOF is 12 bits wide -- still a stream every reader takes, so only the
    bytes show it, and the hand-derived width schedule says which bytes are Go's.  N = 255, 767, 1791: the wider EOF code adds one
    zero bit, and the codes before it always fill whole bytes there (256 x 9, + 512 x 10, + 1024 x 11 bits), so the bytes are the same
    either way; those prefixes pin the width schedule, not the call."""
    import gif_decode_model as gd
    for n in (255, 767, 1791, 3838):
        seq = gc.no_repeats()[:n]
        good = _literal_stream(seq)
        assert good == gm.lzw_encode(seq)
        pix, how, used = gd.lzw_decode(good, 8, n)
        assert (pix, how, used) == (seq.tobytes(), "eof", len(good))
        bad = _literal_stream(seq, final_inc_hi=False)
        assert (bad != good) == (n == 3838)
