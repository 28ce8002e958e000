"""JPEG streams libjpeg never writes (tests/jpeg_edge_corpus.py, tests/jpeg_writer.py) and the Python restatement of Go's reader
(tests/jpeg_decode_model.py), pinned four ways: a float64 IDCT, hand-derived known answers (golden/jpeg_dec_kats.json), byte equality
with the C oracle on Pillow's files and the writer's, and libjpeg within +-2 where it opens the file.  CPU only."""
import io
import json
import os

import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_edge_corpus as je
import oracle
from test_jpeg_decode import picture, pil_jpeg


@pytest.fixture(scope="module")
def corpus():
    return je.corpus()


def _verdict(f, data):
    try:
        return f(data), "ok"
    except ValueError as e:
        return None, str(e).split(":")[0]


def test_model_decodes_writer_streams_to_their_coefficients(corpus):
    for c in corpus:
        if c.path == "unsupported":
            continue
        d = dm.decode(c.data, want_coefs=True)
        assert (d["w"], d["h"], d["ratio"]) == (c.w, c.h, c.ratio), c.name
        for k, want in enumerate(c.coefs):
            np.testing.assert_array_equal(d["coefs"][k], want, err_msg="%s component %d" % (c.name, k))


def _pillow_files():
    out = []
    for i, (w, h, kw) in enumerate([(17, 9, {}), (33, 70, dict(subsampling=0)), (40, 24, dict(subsampling=1, restart_marker_blocks=2)),
                                    (64, 48, dict(quality=100, optimize=True)), (23, 31, dict(quality=5)), (1, 1, {}),
                                    (50, 50, dict(progressive=True)), (96, 64, dict(restart_marker_rows=1, subsampling=2))]):
        img = picture(w, h, seed=i)
        out += [pil_jpeg(img, **kw), pil_jpeg(img[..., 0], **kw)]
    return out


def test_model_and_oracle_agree_on_every_file(corpus):
    """planes and verdict, on the writer's corpus and on Pillow's files (the model's scope ends at SOF2: progressive files are
    'unsupported' there, and the oracle decodes them)"""
    for k, data in enumerate([c.data for c in corpus] + _pillow_files()):
        m, mv = _verdict(dm.decode, data)
        o, ov = _verdict(oracle.jpeg_decode, data)
        if mv == "unsupported" and b"\xff\xc2" in data and ov == "ok":
            continue                      # progressive: outside the model
        assert mv == ov, (k, mv, ov)
        if mv == "ok":
            assert m["dc_wide"] == o["dc_wide"]
            for p in ("y", "cb", "cr"):
                np.testing.assert_array_equal(m[p], o[p], err_msg="file %d plane %s" % (k, p))


def test_model_and_oracle_agree_on_damaged_edge_files(corpus):
    """bit flips and truncations of the corpus: the same verdict, and the same planes where both decode"""
    rng = np.random.default_rng(3)
    for t in range(300):
        c = corpus[t % len(corpus)]
        f = bytearray(c.data)
        sos = f.rindex(b"\xff\xda")
        if t % 3 == 0:
            f[int(rng.integers(sos + 4, len(f)))] ^= 1 << int(rng.integers(0, 8))
        elif t % 3 == 1:
            f = f[:int(rng.integers(2, len(f)))]
        else:
            f[int(rng.integers(2, len(f)))] = int(rng.integers(0, 256))
        m, mv = _verdict(dm.decode, bytes(f))
        o, ov = _verdict(oracle.jpeg_decode, bytes(f))
        assert mv == ov, (t, c.name, mv, ov)
        if mv == "ok":
            for p in ("y", "cb", "cr"):
                np.testing.assert_array_equal(m[p], o[p], err_msg="case %d (%s) plane %s" % (t, c.name, p))


def test_corpus_covers_every_edge(corpus):
    """the coverage the corpus promises: header edges as its cases say, scan edges as the model saw them while decoding"""
    seen = set()
    for c in corpus:
        if c.path != "unsupported":
            dm.decode(c.data, stats=seen)
    assert je.SCAN_EDGES - seen == set()
    assert je.HEADER_EDGES - set().union(*[c.edges for c in corpus]) == set()
    assert {c.path for c in corpus} == {"gpu", "host", "unsupported"}


def test_the_wrap_cases_need_the_row_shortcut(corpus):
    """the files tagged idct_wrap decode differently without idct.go's row shortcut (the kernel's arithmetic before the fix): they
    are what tells a kernel without it apart"""
    n = 0
    for c in corpus:
        if "idct_wrap" not in c.edges:
            continue
        a, b = dm.decode(c.data), dm.decode(c.data, shortcut=False)
        assert any(not np.array_equal(a[p], b[p]) for p in ("y", "cb", "cr")), c.name
        n += 1
    assert n >= 5


def _fdct(px):
    """float64 forward DCT of (n, 8, 8) level-shifted samples (T.81 A.3.3)"""
    k = np.arange(8)
    cu = np.where(k == 0, np.sqrt(0.5), 1.0)
    m = cu[:, None] * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) / 2      # m[u, x]
    return np.einsum("ux,nxy,vy->nuv", m, px, m)


def _idct_f64(coef):
    k = np.arange(8)
    cu = np.where(k == 0, np.sqrt(0.5), 1.0)
    m = cu[:, None] * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) / 2
    return np.einsum("ux,nuv,vy->nxy", m, coef, m)


def test_idct_against_float64():
    """IEEE 1180-style blocks: the forward DCT of random 8-bit blocks, rounded and clamped to +-2048, through the model's idct.go and a
    float64 IDCT: every pixel within 1 of clip(round(float) + 128), at most 2 % of them off by one, and no position biased by more than
    0.015 on average"""
    rng = np.random.default_rng(1180)
    for lo, hi in ((-256, 255), (-5, 5), (-300, 300)):
        n = 4000
        px = rng.integers(lo, hi + 1, (n, 8, 8)).astype(np.float64)
        coef = np.clip(np.round(_fdct(px)), -2048, 2047)
        want = np.clip(np.round(_idct_f64(coef)) + 128, 0, 255).astype(np.int64)
        got = np.clip(dm.idct(coef.reshape(n, 64).astype(np.int64)), -128, 127).reshape(n, 8, 8) + 128
        diff = got - want
        assert np.abs(diff).max() <= 1, (lo, hi)
        assert np.count_nonzero(diff) <= 0.02 * diff.size, (lo, hi, np.count_nonzero(diff))
        assert np.abs(diff.mean(axis=0)).max() <= 0.015, (lo, hi)


def test_known_answers():
    kats = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "jpeg_dec_kats.json")))
    assert len(kats) >= 15
    for k in kats:
        data = bytes.fromhex(k["jpeg"])
        want = np.array(k["y"], np.uint8)
        np.testing.assert_array_equal(dm.decode(data)["y"], want, err_msg=k["name"])
        np.testing.assert_array_equal(oracle.jpeg_decode(data)["y"], want, err_msg=k["name"])


def test_close_to_libjpeg(corpus):
    """where libjpeg (Pillow) opens a writer file whose coefficients stay in the ordinary range, its luma is within 2 of the model's"""
    from PIL import Image
    n = 0
    for c in corpus:
        if c.path == "unsupported" or c.edges & {"idct_wrap", "dqt16"} or c.name.startswith(("big", "symbols")):
            continue                      # (libjpeg reads the magnitude bits of a run past zig 63, Go does not)
        try:
            p = Image.open(io.BytesIO(c.data))
            p.draft("YCbCr" if c.ratio != 4 else "L", (c.w, c.h))
            p.load()
        except OSError:
            continue
        ref = np.asarray(p).astype(int)
        ref = ref if ref.ndim == 2 else ref[..., 0]
        d = dm.decode(c.data)
        diff = np.abs(d["y"][:c.h, :c.w].astype(int) - ref)
        assert diff.max() <= 2, (c.name, diff.max())
        n += 1
    assert n >= 15
