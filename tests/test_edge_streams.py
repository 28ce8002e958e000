"""The PNG and GIF decoders' models on streams zlib and Pillow never write (tests/png_edge_corpus.py, tests/gif_edge_corpus.py), against
references that are not the models: the filtered bytes and index frames the tests built, zlib.decompress, and Pillow.  And a coverage
test, so that an edit of the corpora cannot quietly drop the edges the GPU tests (test_png_decode_edges_gpu.py,
test_gif_decode_edges_gpu.py) rely on."""
import io
import zlib

import numpy as np
import pytest

import deflate_writer as dw
import gif_decode_model as gdm
import gif_edge_corpus as ge
import lzw_writer as lw
import png_decode_model as pdm
import png_edge_corpus as pe


@pytest.fixture(scope="module")
def png_cases():
    return pe.corpus()


@pytest.fixture(scope="module")
def gif_cases():
    return ge.corpus()


def test_png_streams_inflate_to_the_built_bytes(png_cases):
    """zlib.decompress, the model's bit-by-bit inflater and the writer's own table-driven one give the filtered stream the test
    built, and the model's frame is the one the test meant"""
    for c in png_cases:
        assert len(c.raw) <= 256 << 10, c.name
        assert zlib.decompress(c.stream) == c.raw, c.name
        raw, end = pdm.inflate(c.stream, len(c.raw))
        assert raw == c.raw and end == len(c.stream), c.name
        assert dw.stats(c.stream)[1] == c.raw, c.name
        r = pdm.decode(c.data)
        assert r["status"] == pdm.OK and r["kind"] == c.kind, (c.name, r["why"])
        np.testing.assert_array_equal(r["pix"], c.frame, err_msg=c.name)


def test_gif_streams_decode_to_the_built_frames(gif_cases):
    """the model gives the index frame and palette the test built; Pillow decodes every file to the same indices"""
    from PIL import Image
    for name, data, idx, pal, _ in gif_cases:
        r = gdm.decode(data)
        assert r["ok"], (name, r["error"])
        np.testing.assert_array_equal(r["index"], idx, err_msg=name)
        np.testing.assert_array_equal(r["palette"][:len(pal), :3], pal, err_msg=name)
        assert (r["palette"][:len(pal), 3] == 255).all() and not r["palette"][len(pal):].any()
        im = Image.open(io.BytesIO(data))
        im.load()
        np.testing.assert_array_equal(np.array(im), idx, err_msg=name)


def test_writers_refuse_what_go_or_zlib_would_not_take():
    """incomplete codes are refused; the code-length emitters differ only in where the runs may cross HLIT"""
    tok = dw.literals(b"abcabc")
    lit = [0] * 286
    lit[ord("a")], lit[ord("b")], lit[ord("c")], lit[256] = 2, 2, 2, 3         # Kraft sum 7/8: incomplete
    with pytest.raises(AssertionError):
        dw.write([{"kind": "dynamic", "tokens": tok, "lit": lit}], b"abcabc")
    assert dw.codegen([5, 5], [5, 5, 5], "go") == [(5, 0, 0), (16, 1, 2)]
    assert dw.codegen([5, 5], [5, 5, 5], "zlib") == [(5, 0, 0)] * 5


def test_lzw_writer_widths_follow_the_reader():
    """a frame long enough to fill the table at width 2: every code the reader sees is the writer's, at the width the writer chose
    (the model decodes it) and the table frozen for the rest of the frame serves the codes the writer counted"""
    idx = np.random.default_rng(4).integers(0, 4, (200, 200)).astype(np.uint8)
    data, frozen = lw.lzw(idx, 2, clear="never")
    pix, how, _ = gdm.lzw_decode(data, 2, idx.size)
    assert how == "eof" and pix == idx.tobytes() and frozen > 1000


def test_coverage(png_cases, gif_cases):
    """the corpora still reach every edge the issue named"""
    from collections import Counter
    agg = {"max_dist": 0, "far": 0, "cross": 0, "at_hlit": 0, "stored": [], "stored_offsets": set()}
    lens = {"lit": Counter(), "len": Counter(), "dist": Counter()}
    long_dist_syms = set()
    kinds = []
    for c in png_cases:
        st, _ = dw.stats(c.stream)
        agg["max_dist"] = max(agg["max_dist"], st["max_dist"])
        for k in ("far", "cross", "at_hlit"):
            agg[k] += st[k]
        agg["stored"] += st["stored"]
        agg["stored_offsets"] |= st["stored_offsets"]
        lens["lit"].update(st["lit_lens"])
        lens["len"].update(st["len_lens"])
        for (s, n), v in st["dist_lens"].items():
            lens["dist"][n] += v
            if n >= 9:
                long_dist_syms.add(s)
        kinds.append([k for k, _ in st["blocks"]])
    assert agg["max_dist"] == 32768 and agg["far"] >= 100
    assert lens["lit"][15] >= 100 and lens["len"][15] >= 100 and lens["dist"][15] >= 100
    assert long_dist_syms == set(range(30))                              # codes of 9 .. 15 bits on every distance symbol
    assert agg["cross"] >= 1 and agg["at_hlit"] >= 1
    assert 65535 in agg["stored"] and agg["stored"].count(0) >= 2 and {8191, 8192, 8193, 16383, 16384, 16385} <= set(agg["stored"])
    assert agg["stored_offsets"] == set(range(8))
    raw_lens = {len(c.raw) for c in png_cases}
    for k in (1, 2):
        assert {k * 16384 - 1, k * 16384, k * 16384 + 1} <= raw_lens
    assert any(len(b) >= 400 for b in kinds)                             # hundreds of one-symbol blocks
    assert any(("dynamic", "fixed") in zip(b, b[1:]) for b in kinds)     # fixed tables rebuilt after a dynamic block
    assert any("rle" in c.name for c in png_cases) and any("huffman" in c.name for c in png_cases)
    assert max(g[4] for g in gif_cases) >= 10000                         # a frozen table serving 12-bit codes
    assert {g[1][10 + 3 * (1 << ((g[1][10] & 7) + 1)) + 3 + 10] for g in gif_cases} == set(range(2, 9))
