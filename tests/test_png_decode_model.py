"""The PNG decoder model (tests/png_decode_model.py) on the CPU: against the hand-derived known answers of
tests/golden/png_dec_kats.json, its pure-Python inflater against zlib.decompress on a seeded corpus (levels 0 to 9, the strategies,
window bits 9 to 15, IDAT chunks split at one byte or at random points, each filter forced on every row), and its 8-bit frames against
Pillow.  The GPU decoder is held to this model in test_png_decode_gpu.py.  Also: the new ABI entries refuse bad arguments without a GPU."""
import io
import json
import os
import zlib

import numpy as np
import pytest

import png_corpus as pc
import png_decode_model as dm

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "png_dec_kats.json")) as f:
    KATS = json.load(f)


@pytest.mark.parametrize("k", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(k):
    r = dm.decode(bytes.fromhex(k["data"]))
    assert r["status"] == k["status"], r["why"]
    if k["status"] != dm.OK:
        return
    assert (r["kind"], r["w"], r["h"]) == (k["kind"], k["w"], k["h"])
    assert r["pix"].tobytes().hex() == k["pix"]
    if "palette" in k:
        assert r["palette"].tobytes().hex() == k["palette"]


def test_known_answers_cover_the_rules():
    names = " ".join(k["name"] for k in KATS)
    for word in ("gray1", "gray2", "gray4", "gray8 2x2", "gray8 trns", "gray-alpha8", "rgb8 trns", "rgba8", "rgb8", "pal1", "pal2",
                 "pal4 trns", "pal8", "gray16", "rgb16", "gray16 trns", "gray-alpha16", "rgb16 trns", "rgba16", "paeth", "sub up",
                 "filter type 5", "CM 7", "CINFO 8", "FCHECK", "FDICT", "bad adler", "block type 3", "LEN vs NLEN", "symbol 286",
                 "symbol 287", "distance code 30", "distance code 31", "beyond the bytes produced", "too much pixel data",
                 "not enough pixel data", "ends early", "after the Adler-32", "IDAT after the stream", "single distance code",
                 "empty distance code", "incomplete literal code", "over-subscribed", "repeat 16 first", "repeat past", "HLIT 287",
                 "HDIST 31", "bad signature", "CRC", "Adam7", "unknown critical", "IDAT, ancillary, IDAT", "palette without PLTE",
                 "PLTE on gray", "tRNS longer than PLTE", "tRNS on sub-byte gray", "sample 256", "tRNS on rgb after PLTE",
                 "unknown chunk before IHDR"):
        assert word in names, word
    assert {k["status"] for k in KATS} == {dm.OK, dm.INVALID, dm.UNSUPPORTED}


def _corpus():
    rng = np.random.default_rng(17)
    out = []
    for level in range(10):
        for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
            ct, dp, tr = [(2, 8, False), (6, 8, False), (0, 4, False), (3, 8, True), (4, 16, False)][(level + strategy) % 5]
            wbits = 9 + (level + 2 * strategy) % 7
            fl = ((level + strategy) % 5,)
            split = (None, 1, "random")[(level * 5 + strategy) % 3]
            kind = ("photo", "flat")[level % 2]
            out.append(pc.of_type(ct, dp, tr, 9 + level, 11 + 3 * strategy, seed=int(rng.integers(1 << 30)), kind=kind, filters=fl,
                                  level=level, strategy=strategy, wbits=wbits, split=split))
    return out


def test_inflater_against_zlib():
    files = _corpus()
    wb = set()
    for f in files:
        st, fields = dm.parse(f)
        assert st == dm.OK
        stream = b"".join(fields["idat"])
        raw = zlib.decompress(stream)
        got, end = dm.inflate(stream, len(raw))
        assert got == raw and end == len(stream)
        wb.add(stream[0] >> 4)
        r = dm.decode(f)
        assert r["status"] == dm.OK, r["why"]
        np.testing.assert_array_equal(r["pix"], dm.decode(f, fast=True)["pix"])
    assert wb == set(range(1, 8))                  # window bits 9 .. 15 all seen


@pytest.mark.parametrize("mode", ["L", "RGB", "RGBA", "LA", "P"])
def test_8bit_frames_against_pillow(mode):
    from PIL import Image
    rng = np.random.default_rng(3)
    for k, (w, h) in enumerate([(1, 1), (17, 5), (64, 48)]):
        c = {"L": 1, "RGB": 3, "RGBA": 4, "LA": 2, "P": 1}[mode]
        a = pc.photo(h, w, c, 50 + k).astype(np.uint8)
        im = Image.fromarray(a[..., 0], "L").convert("P") if mode == "P" else Image.fromarray(a if c > 1 else a[..., 0], mode)
        b = io.BytesIO()
        im.save(b, "PNG", optimize=bool(k % 2))
        r = dm.decode(b.getvalue())
        assert r["status"] == dm.OK
        back = Image.open(io.BytesIO(b.getvalue()))
        if mode == "P":
            np.testing.assert_array_equal(r["pix"], np.asarray(back))
            want = np.asarray(back.convert("RGBA"))
            got = r["palette"][r["pix"]]
            np.testing.assert_array_equal(got, want)
        elif mode == "LA":
            la = np.asarray(back)
            np.testing.assert_array_equal(r["pix"].reshape(h, w, 4), np.stack([la[..., 0]] * 3 + [la[..., 1]], -1))
        else:
            want = np.asarray(back.convert("RGBA" if mode in ("RGB", "RGBA") else "L"))
            np.testing.assert_array_equal(r["pix"].reshape(want.shape), want)


def test_entries_refuse_bad_arguments_without_a_gpu():
    from imageprocessor_amd import _lib, build
    build.build()
    import ctypes as C
    import imageprocessor_amd as m
    L = m.lib()
    for name in ("ipx_png_decode_batch", "ipx_png_frames_free", "ipx_plan_run_png_png"):
        assert hasattr(L, name)
    b = _lib.PngBatch()
    w, h, k = C.c_int(0), C.c_int(0), C.c_int(-1)
    st = (C.c_int * 1)()
    own = C.c_void_p()
    assert L.ipx_png_decode_batch(None, None, None, 1, C.byref(w), C.byref(h), C.byref(k), C.byref(b), st, C.byref(own)) == -1
    assert L.ipx_plan_run_png_png(None, None, 0, None, None, None, None, None, None) == -1
