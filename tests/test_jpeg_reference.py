"""CPU: what pins the colour path of oracle/ipx_jpeg_oracle.c -- the float64 reference of tests/jpeg_encode_reference.py, written from
T.81 and the quoted rules of Go's writer rather than from the oracle's C -- and what keeps the corpus of tests/jpeg_encode_corpus.py
honest.  The GPU half is tests/test_jpeg_reference_gpu.py.

The 8K frame and the four 65535-long frames of the corpus are NOT run through the reference here (the 8K frame alone is 50 M float64
coefficients; the long ones add nothing the 80 small geometries and the 4K frame do not already give the reference); on the GPU they
are held to the oracle byte for byte."""
import numpy as np
import pytest

import jpeg_decode_model as jdm
import jpeg_encode_corpus as C
import jpeg_encode_reference as R
import oracle


def test_integer_colour_formulas_are_the_jfif_matrix():
    """All 2^24 R, G, B triples: every channel of color.RGBToYCbCr's integer formulas is within 0.5 + 2^-7 of the real (clamped) JFIF
    matrix value.  Only this makes the formulas of jpeg_encode_reference.ycbcr the definition the rest relies on."""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = np.zeros(3)
    for r in range(256):
        got = np.stack(R.ycbcr(np.full_like(g, r), g, b))
        assert got.min() >= 0 and got.max() <= 255
        worst = np.maximum(worst, np.abs(got - R.jfif_real(np.full_like(g, r), g, b)).max(axis=(1, 2)))
    print("largest |integer - real| per channel:", worst)
    assert (worst <= R.COLOUR_TOLERANCE).all(), worst


@pytest.fixture(scope="module")
def cases():
    """[(recipe, frame, oracle stream, oracle coefficients, Ref)]"""
    out = []
    for kind, w, h, seed, q in C.reference_cases():
        f = C.frame(kind, w, h, seed)
        data, coefs = oracle.jpeg_encode_rgba(f, q, want_coefs=True)
        out.append(((kind, w, h, seed, q), f, data, coefs, R.reference(f, R.dqt_tables(data))))
    return out


def test_oracle_coefficients_against_the_reference(cases):
    for recipe, f, data, coefs, ref in cases:
        R.assert_matches(coefs, ref, R.cap(recipe[4]), what="oracle %r" % (recipe,))


def test_alpha_does_not_matter():
    for kind, w, h, seed in C.GEOMETRIES:
        if kind == "translucent":
            f = C.frame(kind, w, h, seed)
            opaque = f.copy()
            opaque[..., 3] = 255
            assert oracle.jpeg_encode_rgba(f, 85) == oracle.jpeg_encode_rgba(opaque, 85)
            assert (R.real_coefficients(f) == R.real_coefficients(opaque)).all()


def test_error_bound_holds_on_the_cpu():
    """E of the reference is 1.5 x the largest error of the oracle's fixed-point transform seen at quality 100 (all quantisers 1);
    recomputed here over the same frames, it stays under E and has not drifted from the figure written beside the constant."""
    worst = 0.0
    for kind, w, h, seed in C.GEOMETRIES + C.LARGE[:1]:
        f = C.frame(kind, w, h, seed)
        data, coefs = oracle.jpeg_encode_rgba(f, 100, want_coefs=True)
        dqt = R.dqt_tables(data)
        assert (dqt[0] == 1).all() and (dqt[1] == 1).all()
        worst = max(worst, float(np.abs(coefs - R.real_coefficients(f)).max()) - 0.5)
    print("largest fdct error, unquantised units: %.4f (E_SEEN %.4f, E %.4f)" % (worst, R.E_SEEN, R.E))
    assert worst <= R.E_SEEN + 5e-5 and abs(R.E - 1.5 * R.E_SEEN) < 1e-3


def test_ambiguous_shares_stay_under_their_caps(cases):
    seen = {}
    for recipe, f, data, coefs, ref in cases:
        q = recipe[4]
        seen[q] = max(seen.get(q, 0.0), ref.ambiguous)
        assert ref.ambiguous <= R.cap(q), recipe
    print("largest ambiguous share per quality:", seen)
    for q, v in seen.items():
        assert v <= R.SEEN_AMBIGUOUS[q] + 5e-5, (q, v)            # the written figure is the one this suite shows
        assert R.MAX_AMBIGUOUS[q] <= max(2.2 * R.SEEN_AMBIGUOUS[q], 0.01), q


def test_host_entropy_coder_round_trips_through_the_decoder_model(cases):
    """csrc/ipx_jpeg_host.cpp writes the coefficients it is given: tests/jpeg_decode_model.py (Go's reader, restated on its own) reads
    every stream back to them, with the size and the 2x2 / 1x1 sampling of SOF0"""
    import imageprocessor_amd as ipx
    n = 0
    for recipe, f, data, coefs, ref in cases:
        kind, w, h, seed, q = recipe
        if w * h > 20000 or q == 50:
            continue                                              # the Python Huffman reader is slow
        stream = ipx.jpeg_entropy_encode(coefs, w, h, q)
        d = jdm.decode(stream, want_coefs=True)
        assert (d["w"], d["h"], d["ratio"]) == (w, h, 2), recipe
        np.testing.assert_array_equal(R.scan_order_of(d["coefs"]), coefs, err_msg=repr(recipe))
        n += 1
    assert n >= 200


@pytest.mark.parametrize("name,recipe", C.STREAM_RECIPES, ids=[n for n, _ in C.STREAM_RECIPES])
def test_stream_length_edges_are_present(name, recipe):
    """an edit of the corpus cannot quietly drop an edge the stuffing kernel is tested on"""
    kind, w, h, seed, q = recipe
    hdr, scan, u = C.scan_of(oracle.jpeg_encode_rgba(C.frame(kind, w, h, seed), q))
    assert C.PROPERTIES[name](u), (name, len(u))
    assert len(scan) - len(u) == u.count(b"\xff")


def test_stream_recipes_cover_every_edge():
    assert [n for n, _ in C.STREAM_RECIPES] == list(C.PROPERTIES)


def test_phase_recipe_shows_all_sixteen_shifts():
    kind, w, h, seed, q = C.PHASE_RECIPE
    assert q == 100
    assert C.phases(oracle.jpeg_encode_rgba(C.frame(kind, w, h, seed), q)) == set(range(16))


def test_corpus_holds_what_the_gpu_tests_rely_on():
    assert {(w, h) for _, w, h, _ in C.GEOMETRIES} >= {(w, h) for w in C.WIDTHS for h in C.HEIGHTS}
    for kind in C.KINDS:
        assert sum(1 for g in C.GEOMETRIES if g[0] == kind) >= 10, kind
    f = C.frame("edge", 145, 33, 1).astype(int)
    assert np.abs(f[:, -1, :3] - f[:, -2, :3]).mean() > 40 and np.abs(f[-1, :, :3] - f[-2, :, :3]).mean() > 40
    for name, es, ef, off in C.LAYOUTS:
        frames = np.stack([C.frame("noise", 17, 5, i) for i in range(2)])
        buf, o, stride, fs = C.lay_out(frames, es, ef, off)
        for i in range(2):
            rows = np.lib.stride_tricks.as_strided(buf[o + i * fs:], (5, 68), (stride, 1))
            assert (rows == frames[i].reshape(5, 68)).all(), name
    assert any(fs % 16 for _, es, ef, _ in C.LAYOUTS for fs in [5 * (68 + es) + ef])
    assert {off for *_, off in C.LAYOUTS} >= {0, 4, 8, 12} and {es for _, es, _, _ in C.LAYOUTS} >= {4, 12, 16}
