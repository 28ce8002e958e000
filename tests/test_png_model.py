"""The PNG model (tests/png_model.py) on the CPU: Go's decisions against hand-derived known answers (tests/golden/png_kats.json), the
stream against zlib and Pillow (inflates to exactly the filtered rows, decodes to the expected pixels, every chunk CRC checks), the
size against the stored bound and zlib level 1, the Huffman limits, and the constants shared with csrc/ipx_png.h.  The GPU encoder is
held to this model in test_png_gpu.py."""
import io
import json
import os
import re
import zlib

import numpy as np
import pytest

import png_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "png_kats.json")) as f:
    KATS = json.load(f)


@pytest.mark.parametrize("c", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_filters_against_known_answers(c):
    rgba = np.array(c["rgba"], np.uint8).reshape(c["h"], c["w"], 4)
    bpp, raw = pm.raw_rows(rgba)
    assert bpp == c["bpp"]
    types, filtered = pm.filter_rows(raw, bpp)
    assert types.tolist() == c["types"]
    assert filtered.tolist() == c["filtered"]


def test_unpremultiply_every_alpha():
    for c, a, want in KATS["unpremultiply"]:
        got = pm.unpremultiply(np.array([[[c, c, c, a]]], np.uint8))[0, 0]
        assert got.tolist() == [want, want, want, a], (c, a)
    px = np.array([[[9, 8, 7, 0], [9, 8, 7, 255]]], np.uint8)
    assert pm.unpremultiply(px).tolist() == [[[0, 0, 0, 0], [9, 8, 7, 255]]]


def _corpus():
    rng = np.random.default_rng(2026)
    out = {}
    for w, h in ((96, 64), (200, 200), (333, 129), (640, 480)):
        yy, xx = np.mgrid[0:h, 0:w]
        noise = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        noise[..., 3] = 255
        out["noise %dx%d" % (w, h)] = noise
        flat = np.zeros((h, w, 4), np.uint8)
        flat[..., 3] = 255
        flat[(yy // 24 + xx // 24) % 2 == 0, :3] = (200, 30, 90)
        flat[h // 2:h // 2 + 12, 10:w - 10, :3] = 255 * ((xx[h // 2:h // 2 + 12, 10:w - 10] // 3) % 2)[..., None]   # text-like strokes
        out["flat %dx%d" % (w, h)] = flat
        sm = np.zeros((h, w, 4), np.uint8)
        sm[..., 0] = (128 + 100 * np.sin(xx / 7.0)).astype(np.uint8)
        sm[..., 1] = (128 + 100 * np.cos(yy / 11.0)).astype(np.uint8)
        sm[..., 2] = (xx + yy) % 256
        sm[..., 3] = 255
        out["smooth %dx%d" % (w, h)] = sm
        al = sm.copy()
        al[..., 3] = np.where(rng.random((h, w)) < 0.3, rng.integers(0, 255, (h, w)), 255)
        al[..., :3] = (al[..., :3].astype(np.uint32) * al[..., 3:4] // 255).astype(np.uint8)
        out["alpha %dx%d" % (w, h)] = al
    wide = np.zeros((3, 8200, 4), np.uint8)
    wide[..., 0] = np.arange(8200) % 251
    wide[1, :, 3] = 7
    out["wide 8200x3"] = wide
    return out


CORPUS = _corpus()


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_stream_decodes_and_stays_in_bounds(name):
    from PIL import Image
    f = CORPUS[name]
    s = pm.png_encode(f)
    chunks = pm.read_chunks(s)                                  # every CRC
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}
    bpp, w, h, data = pm.filtered_stream(f)
    assert chunks[0][1] == pm.ihdr(w, h, bpp)[8:-4]
    z = b"".join(d for k, d in chunks if k == b"IDAT")
    assert z[:2] == b"\x78\x9c" and len(chunks[-2][1]) == 4
    assert zlib.decompress(z) == data.tobytes()                  # exactly the filtered rows, Adler-32 included
    assert len(chunks) - 3 == len(pm.segments(w, h, bpp))       # a chunk per segment, then the Adler chunk
    im = Image.open(io.BytesIO(s))
    assert im.mode == ("RGB" if bpp == 3 else "RGBA")
    np.testing.assert_array_equal(np.array(im), pm.raw_rows(f)[1].reshape(h, w, bpp))
    assert len(s) <= pm.stream_bound(w, h, bpp)
    assert len(z) <= 1.5 * len(zlib.compress(data.tobytes(), 1)), "the match finder lost its matches"


def test_segments_cover_whole_rows():
    for w, h, bpp in ((1, 1, 3), (100, 1000, 4), (16383, 5, 4), (8200, 3, 4), (21845, 7, 3)):
        segs = pm.segments(w, h, bpp)
        stride = 1 + w * bpp
        assert segs[0][0] == 0 and segs[-1][1] == h * stride
        for (s0, e0), (s1, _) in zip(segs, segs[1:]):
            assert e0 == s1
        for s, e in segs:
            assert s % stride == 0 and e % stride == 0
            assert e - s >= min(pm.SEG_MIN, h * stride)


def test_huffman_limits_and_completeness():
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for freq, limit in ((fib + [0] * 256, 15), (fib[:19], 7), ([5] + [0] * 29, 15), ([0] * 30, 15), ([3, 3, 3], 7)):
        ln = pm.huffman_lengths(freq, limit)
        assert max(ln) <= limit
        assert sum(2.0 ** -v for v in ln if v) == 1.0            # complete: zlib refuses an incomplete code-length code
        used = [s for s, f in enumerate(freq) if f]
        assert all(ln[s] for s in used)


def test_rle_of_code_lengths():
    seq = [0] * 140 + [5] * 8 + [0] * 2 + [3]
    out = pm.rle_code_lengths(seq)
    assert out == [(18, 127, 7), (0, 0, 0), (0, 0, 0), (5, 0, 0), (16, 3, 2), (5, 0, 0), (0, 0, 0), (0, 0, 0), (3, 0, 0)]


def test_constants_shared_with_the_kernels():
    h = open(os.path.join(HERE, "..", "imageprocessor_amd", "csrc", "ipx_png.h")).read()

    def const(name):
        return int(re.search(r"\b%s\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?;" % name, h).group(1), 0)
    assert const("kPngSegMin") == pm.SEG_MIN
    assert const("kPngTile") == pm.TILE
    assert const("kPngHashBits") == pm.HASH_BITS
    assert const("kPngHashMul") == pm.HASH_MUL
    assert const("kPngWindow") == pm.WINDOW
