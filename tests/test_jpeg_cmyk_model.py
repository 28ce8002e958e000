"""The three pins of tests/jpeg_cmyk_model.py, the numpy restatement of Go's four-component JPEG decode (the
rules are recalled, not read, so none of this pins parity with Go):

  1. the three-component oracle: the writer's three-component file and Gray file of the same coefficients go through the existing
     oracle decoder; Y, Cb, Cr and K must equal the model's planes byte for byte (entropy coding, IDCT, the progressive rule)
  2. hand known answers for applyBlack (tests/golden/jpeg_cmyk_kats.json)
  3. libjpeg (Pillow) as an independent decoder on 11 11 11 11 files: Pillow's own CMYK files and the writer's transform-2 files"""
import io
import json
import os

import numpy as np
import pytest

import jpeg_cmyk_model as model
import jpeg_cmyk_writer as cw
from jpeg_decode_model import Malformed, Unsupported

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1, 1), (9, 7, 1), (17, 15, 1), (16, 16, 2), (17, 15, 2), (33, 31, 2), (1, 1, 2)]
# The largest difference between the model and libjpeg measured over the corpus of test 3: 2 grey levels, the
# three-component decoder's own figure (idct.go against jidctint.c, and the rounding of the two YCbCr -> RGB tables).
PILLOW_MEASURED = 2


@pytest.fixture(scope="module")
def oracle():
    import oracle
    oracle.build()
    return oracle


@pytest.mark.parametrize("w,h,v", SIZES)
def test_sequential_decode_equals_the_blocks(w, h, v):
    """the entropy decoder of the model against the writer: baseline, restart intervals, every transform"""
    f = cw.frame4(w, h, v)
    b = cw.blocks4(f, 100 + w + v)
    for transform, dri in ((0, 0), (1, 1), (2, 3)):
        want = model.from_blocks(f, b, cw.quants(), transform)
        got = model.decode(cw.cmyk_file(f, b, transform=transform, dri=dri))
        assert (got["w"], got["h"], got["v"], got["transform"]) == (w, h, v, transform)
        for k in ("y", "cb", "cr", "k", "pix"):
            assert np.array_equal(got[k], want[k]), (k, transform, dri)


@pytest.mark.parametrize("progressive", [False, True])
@pytest.mark.parametrize("w,h,v", SIZES)
def test_planes_equal_the_three_component_oracle(oracle, w, h, v, progressive):
    f = cw.frame4(w, h, v)
    b = cw.blocks4(f, 200 + w + v)
    m = model.from_blocks(f, b, cw.quants(), 2, progressive)
    f3, fk = cw.split_files(f, b, progressive=progressive)
    d3, dk = oracle.jpeg_decode(f3), oracle.jpeg_decode(fk)
    assert d3["ratio"] == (2 if v == 2 else 0)
    for k in ("y", "cb", "cr"):
        assert np.array_equal(d3[k], m[k]), k
    want_k = dk["y"]
    if progressive:                                   # the Gray file covers the whole padded plane; K's blocks outside the image stay zero
        rows, cols = f.grid(3)
        keep = (np.arange(rows)[:, None] * 8 < h) & (np.arange(cols)[None, :] * 8 < w)
        want_k = want_k * np.kron(keep, np.ones((8, 8), bool)).astype(np.uint8)
        assert np.any(m["k"][:8, :8])                 # (not all of it)
    assert np.array_equal(want_k, m["k"])


def _kats():
    with open(os.path.join(HERE, "golden", "jpeg_cmyk_kats.json")) as fh:
        return json.load(fh)["cases"]


def kat_inputs(case):
    """-> (frame, blocks, quantisers) of a known-answer case: DC-only blocks, q = 8, DC = sample - 128"""
    f = cw.frame4(case["w"], case["h"], case["v"])
    blocks = []
    for c in range(4):
        s = np.asarray(case["samples"][c], np.int64)
        assert s.shape == f.grid(c), (case["name"], c)
        b = np.zeros(s.shape + (64,), np.int64)
        b[..., 0] = s - 128
        blocks.append(b)
    return f, blocks, cw.quants(flat=8)


def kat_expected(case, oracle):
    """-> [(x, y, (C, M, Y, K))]"""
    if case["expect"] != "oracle":
        return [(x, y, tuple(p)) for x, y, p in case["expect"]]
    v, w, h = case["v"], case["w"], case["h"]
    y, cb, cr, k = (np.kron(np.asarray(case["samples"][c], np.uint8), np.ones((8, 8), np.uint8)) for c in range(4))
    rgba = oracle.draw_ycbcr(np.zeros((h, w, 4), np.uint8), (0, 0, w, h), y, cb, cr, 2 if v == 2 else 0)
    return [(x, yy, (int(rgba[yy, x, 0]), int(rgba[yy, x, 1]), int(rgba[yy, x, 2]), 255 - int(k[yy, x]))) for yy in range(h) for x in range(w)]


@pytest.mark.parametrize("case", _kats(), ids=lambda c: c["name"])
def test_apply_black_known_answers(oracle, case):
    f, blocks, q = kat_inputs(case)
    for got in (model.from_blocks(f, blocks, q, case["transform"]), model.decode(cw.cmyk_file(f, blocks, transform=case["transform"], q=q))):
        for x, y, p in kat_expected(case, oracle):
            assert tuple(int(c) for c in got["pix"][y, x]) == p, (x, y)


def test_what_go_refuses():
    f = cw.frame4(16, 16, 1)
    b = cw.blocks4(f, 5)
    for kind in ("absent", "short"):
        with pytest.raises(Unsupported):
            model.decode(cw.cmyk_file(f, b, app14=kind))
    for name, hv in cw.ILLEGAL_VECTORS.items():
        fi = cw.frame4(16, 16, hv=hv)
        with pytest.raises(Unsupported):
            model.decode(cw.cmyk_file(fi, cw.blocks4(fi, 6)))
    good = cw.cmyk_file(f, b)
    with pytest.raises(Malformed):
        model.decode(good[:len(good) - 20])


def pillow_corpus():
    """[(name, file)]: 11 11 11 11 files only (libjpeg upsamples the other vector's chroma differently from Go's replication)"""
    from PIL import Image
    out = []
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:40, 0:56]
    smooth = np.stack([(xx * 4) % 256, (yy * 6) % 256, (xx + yy) * 2 % 256, 255 - (xx * 3 + yy) % 256], -1).astype(np.uint8)
    noise = rng.integers(0, 256, (23, 37, 4), dtype=np.uint8)
    for name, a in (("smooth", smooth), ("noise", noise)):
        for quality in (60, 90, 100):
            buf = io.BytesIO()
            Image.fromarray(a, "CMYK").save(buf, "JPEG", quality=quality, subsampling=0)
            out.append(("pillow %s q%d" % (name, quality), buf.getvalue()))
    for seed, (w, h) in enumerate([(17, 15), (40, 24), (9, 7)]):
        f = cw.frame4(w, h, 1)
        out.append(("writer transform 2 %dx%d" % (w, h), cw.cmyk_file(f, cw.blocks4(f, 300 + seed, amp=60, ac=12, density=0.1), transform=2)))
    return out


def pillow_differences():
    from PIL import Image
    out = []
    for name, data in pillow_corpus():
        im = Image.open(io.BytesIO(data))
        assert im.mode == "CMYK"
        got = model.decode(data)["pix"]
        ref = np.frombuffer(im.tobytes(), np.uint8).reshape(got.shape)
        out.append((name, int(np.abs(got.astype(int) - ref.astype(int)).max())))
    return out


def test_model_against_libjpeg():
    pytest.importorskip("PIL")
    diffs = pillow_differences()
    print(diffs)
    assert len(diffs) == 9
    assert max(d for _, d in diffs) <= PILLOW_MEASURED + 1, diffs
