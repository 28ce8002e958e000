"""The GIF model (tests/gif_model.py) on the CPU: Plan 9 against its known entries, the wavefront dither against the scalar restatement
of drawPaletted, LZW against hand-derived known answers (tests/golden/gif_kats.json), and every stream through Pillow's decoder.  The
GPU encoder is held to this model in test_gif_gpu.py."""
import io
import json
import os

import numpy as np
import pytest

import gif_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "gif_kats.json")) as f:
    KATS = json.load(f)["cases"]


def _decode(stream):
    from PIL import Image
    im = Image.open(io.BytesIO(stream))
    assert im.format == "GIF" and im.mode == "P"
    np.testing.assert_array_equal(np.array(im.getpalette()[:768], np.uint8).reshape(256, 3), gm.PLAN9)
    return np.array(im)


def _frames():
    rng = np.random.default_rng(31)
    out = {}
    f = rng.integers(0, 256, (48, 64, 4), dtype=np.uint8)
    f[..., 3] = 255
    out["noise 64x48"] = f
    yy, xx = np.mgrid[0:37, 0:29]
    g = np.zeros((37, 29, 4), np.uint8)
    g[..., 0], g[..., 1], g[..., 2], g[..., 3] = xx * 8, yy * 6, 128, 255
    out["gradient 29x37"] = g
    a = rng.integers(0, 256, (23, 41, 4), dtype=np.uint8)
    a[..., 3] = np.where(rng.random((23, 41)) < 0.5, a[..., 3], 255)
    a[:5, :5, 3] = 0
    a[..., :3] = (a[..., :3].astype(np.uint16) * a[..., 3:4] // 255).astype(np.uint8)
    out["alpha 41x23"] = a
    out["flat 16x16"] = np.full((16, 16, 4), (200, 30, 90, 255), np.uint8)
    out["one pixel"] = np.array([[[17, 200, 3, 255]]], np.uint8)
    out["column 1x40"] = rng.integers(0, 256, (40, 1, 4), dtype=np.uint8) | np.array([0, 0, 0, 255], np.uint8)
    out["row 50x1"] = rng.integers(0, 256, (1, 50, 4), dtype=np.uint8) | np.array([0, 0, 0, 255], np.uint8)
    out["white and black"] = np.tile(np.array([[[255, 255, 255, 255]], [[0, 0, 0, 255]]], np.uint8), (6, 9, 1))
    return out


def test_plan9_known_entries():
    p = gm.PLAN9
    assert p.shape == (256, 3)
    assert bytes(p[0]) == b"\x00\x00\x00" and bytes(p[1]) == b"\x00\x00\x44" and bytes(p[255]) == b"\xff\xff\xff"
    assert len({bytes(c) for c in p}) == 256
    assert bytes(p[17]) == b"\x11\x11\x11"           # a grey of the den == 0 branch: v = 1


@pytest.mark.parametrize("name", list(_frames()))
def test_wavefront_dither_is_the_scalar_loop(name):
    f = _frames()[name]
    np.testing.assert_array_equal(gm.dither_wavefront(f), gm.dither_scalar(f))


def test_dither_of_palette_colours_is_exact():
    """a frame made of Plan 9 colours quantises to those entries with zero error (the first one among equal colours)"""
    rng = np.random.default_rng(2)
    idx = rng.integers(0, 256, (12, 20))
    f = np.concatenate([gm.PLAN9[idx], np.full((12, 20, 1), 255, np.uint8)], axis=2)
    np.testing.assert_array_equal(gm.dither_scalar(f), idx)


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_lzw_known_answers(case):
    idx = np.array(case["index"], np.uint8)
    assert gm.lzw_encode(idx).hex() == case["lzw_hex"]


def test_sub_block_boundary():
    case = next(c for c in KATS if c["name"].startswith("sub-block"))
    data = bytes.fromhex(case["lzw_hex"])
    assert len(data) == 510
    blocks = gm.sub_blocks(data)
    assert blocks == b"\xff" + data[:255] + b"\xff" + data[255:] + b"\x00"
    stream = gm.encode_index(np.array(case["index"], np.uint8).reshape(1, -1))
    assert stream.endswith(b"\x00\x3b")
    np.testing.assert_array_equal(_decode(stream)[0], case["index"])


def test_header_bytes():
    h = gm.header(300, 2)
    assert h[:6] == b"GIF89a" and h[6:10] == bytes([44, 1, 2, 0]) and h[10:13] == b"\x87\x00\x00"
    assert h[13:13 + 768] == gm.PLAN9.tobytes()
    assert h[781:] == bytes([0x2C, 0, 0, 0, 0, 44, 1, 2, 0, 0, 8])
    with pytest.raises(ValueError):
        gm.encode_index(np.zeros((1, 1 << 16), np.uint8))


@pytest.mark.parametrize("name", list(_frames()))
def test_model_streams_decode_with_pillow(name):
    f = _frames()[name]
    idx = gm.dither_scalar(f)
    s = gm.encode_index(idx)
    assert len(s) <= gm.size_bound(f.shape[1], f.shape[0])
    np.testing.assert_array_equal(_decode(s), idx)


def test_long_stream_with_clears_decodes():
    """many clear codes and widths 9..12: noise indices, and the no-repeat KAT sequence"""
    rng = np.random.default_rng(8)
    idx = rng.integers(0, 256, (150, 200), dtype=np.uint8)
    idx[40:90] = 3
    s = gm.encode_index(idx)
    assert len(s) <= gm.size_bound(200, 150)
    np.testing.assert_array_equal(_decode(s), idx)
    seq = next(c for c in KATS if c["name"].startswith("no repeats"))["index"]
    np.testing.assert_array_equal(_decode(gm.encode_index(np.array(seq, np.uint8).reshape(50, 100)))[:, :], np.array(seq).reshape(50, 100))
