"""The pins of tests/jpeg_411_model.py, the numpy restatement of Go's decode of 4:1:1 / 4:1:0 JPEGs (the rules are
recalled, not read, so none of this pins parity with Go):

  1. hand known answers (tests/golden/jpeg_411_kats.json, written by tests/golden/make_jpeg_411_kats.py without the model): one-MCU
     files, 1 x 1, and 33 x 9 = 2 x 2 MCUs, with the planes, strides and YCbCrAt samples spelled out
  2. an independent identity: the coefficient blocks of ONE component, written as a single-component file, decode through the existing
     Gray oracle to that component's plane -- compared over the component's whole blocks (entropy coding, dequantisation, IDCT, and where
     each block lands)
  3. the entropy decoder against the writer: interleaved scans, restart intervals, non-interleaved scans
  4. libjpeg (Pillow) opens every corpus file at the right size.  That checks the writer only: libjpeg's chroma upsampling is not Go's
     sample replication, so pixels are not compared."""
import io
import json
import os

import numpy as np
import pytest

import jpeg_411_corpus as c4
import jpeg_411_model as model
import jpeg_edge_corpus as ec
import jpeg_writer as jw
from jpeg_decode_model import Malformed, Unsupported

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_SIZES = [(v0, w, h) for v0 in (1, 2) for w, h in c4.SIZES[v0]]


@pytest.fixture(scope="module")
def oracle():
    import oracle
    oracle.build()
    return oracle


def _kats():
    with open(os.path.join(HERE, "golden", "jpeg_411_kats.json")) as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("case", _kats(), ids=lambda c: c["name"])
def test_known_answers(case):
    got = model.decode(bytes.fromhex(case["file"]))
    assert (got["w"], got["h"], got["ratio"]) == (case["w"], case["h"], case["ratio"])
    assert got["y"].shape == (case["yrows"], case["ystride"]) and got["cb"].shape == got["cr"].shape == (case["crows"], case["cstride"])
    assert model.chroma_size(case["ratio"], case["w"], case["h"]) == (case["cw"], case["ch"])
    for k in ("y", "cb", "cr"):
        assert np.array_equal(got[k], np.asarray(case[k], np.uint8)), k
    vs = 2 if case["ratio"] == model.RATIO_410 else 1
    for x, y, yy, cb, cr in case["at"]:                       # YCbCrAt: YOffset and COffset on the flat planes
        ci = (y // vs) * case["cstride"] + x // 4
        assert (int(got["y"].ravel()[y * case["ystride"] + x]), int(got["cb"].ravel()[ci]), int(got["cr"].ravel()[ci])) == (yy, cb, cr), (x, y)
    up = model.upsample(got["cb"], case["ratio"], case["w"], case["h"])
    assert up.shape == (case["h"], case["w"]) and all(int(up[y, x]) == cb for x, y, _, cb, _ in case["at"])


def test_the_known_answer_files_are_what_the_writer_writes_today():
    """(the stored streams pin the writer; a change to it shows here and not as a puzzling plane difference)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_jpeg_411_kats", os.path.join(HERE, "golden", "make_jpeg_411_kats.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for case in _kats():
        assert gen.stream(case["w"], case["h"], case["v0"], case["y_blocks"], case["cb_blocks"], case["cr_blocks"]).hex() == case["file"], case["name"]


@pytest.mark.parametrize("v0,w,h", ALL_SIZES)
def test_each_component_equals_the_gray_oracle(oracle, v0, w, h):
    fr = c4.frame(w, h, v0)
    b = c4.blocks(fr, 500 + w + v0)
    m = model.from_blocks(fr, b, c4.Q)
    d = model.decode(c4.baseline(fr, b))
    dc, ac, _ = ec.tables_short()
    for comp, k in enumerate(("y", "cb", "cr")):
        rows, cols = fr.grid(comp)
        gray = ec.file(cols * 8, rows * 8, [(1, 1, 1, 0)], [b[comp]], {(0, 0): dc, (1, 0): ac}, {0: (c4.QV, 0)})
        want = oracle.jpeg_decode(gray)
        assert want["ratio"] == 4 and want["y"].shape == (rows * 8, cols * 8)
        assert np.array_equal(m[k], want["y"]), k
        assert np.array_equal(d[k], want["y"]), k
    assert d["ratio"] == m["ratio"] == (model.RATIO_411 if v0 == 1 else model.RATIO_410)
    assert d["y"].shape == (8 * v0 * fr.myy, 32 * fr.mxx) and d["cb"].shape == (8 * fr.myy, 8 * fr.mxx)


@pytest.mark.parametrize("v0,w,h", ALL_SIZES)
def test_sequential_decode_equals_the_blocks(v0, w, h):
    fr = c4.frame(w, h, v0)
    b = c4.blocks(fr, 600 + w + v0)
    want = model.from_blocks(fr, b, c4.Q)
    for data in (c4.baseline(fr, b, ri=1), c4.baseline(fr, b, ri=fr.mxx)):
        got = model.decode(data)
        assert all(np.array_equal(got[k], want[k]) for k in ("y", "cb", "cr"))
    # non-interleaved scans carry no data for the blocks outside the image by the component's own grid: those stay zero
    got = model.decode(c4.multiscan(fr, b))
    for comp, k in enumerate(("y", "cb", "cr")):
        rows, cols = fr.grid(comp)
        keep = (np.arange(rows)[:, None] * 8 < h) & (np.arange(cols)[None, :] * 8 < w)
        assert np.array_equal(got[k], want[k] * np.kron(keep, np.ones((8, 8), bool)).astype(np.uint8)), k


def test_what_go_refuses_and_the_switch():
    fr = c4.frame(33, 9, 1)
    good = c4.baseline(fr, c4.blocks(fr, 1))
    assert model.status_of(good) == model.OK and model.status_of(good, enabled=False) == model.UNSUPPORTED
    for name, kw in c4.REFUSED:
        with pytest.raises(Unsupported):
            model.decode(c4.refused_file(40, 24, **kw))
    with pytest.raises(Malformed):
        model.decode(c4.cut_in_scan(good))
    import jpeg_decode_model as jm
    with pytest.raises(Unsupported):                          # the shared model is as it was once decode() returns
        jm.decode(good)


def test_libjpeg_opens_every_file_at_its_size():
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for v0, w, h in ALL_SIZES:
        fr = c4.frame(w, h, v0)
        b = c4.blocks(fr, 700 + w, amp=60, ac=12, density=0.1)
        for k, data in enumerate((c4.baseline(fr, b), c4.baseline(fr, b, ri=1), c4.multiscan(fr, b), c4.progressive(fr, b))):
            im = Image.open(io.BytesIO(data))
            # the sequential files are decoded in full.  The progressive writer's per-scan tables (built to reach 16-bit codes) make
            # streams libjpeg does not decode at ANY sampling, 4:4:4 included: for those files the frame header is what is checked
            if k < 3:
                im.load()
            assert im.size == (w, h) and im.mode in ("YCbCr", "RGB")
            assert [tuple(l[1:3]) for l in im.layer] == [(4, v0), (1, 1), (1, 1)]      # libjpeg's view of the sampling factors
            n += 1
    assert n == 4 * len(ALL_SIZES)
