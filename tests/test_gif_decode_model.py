"""The GIF decoder model (tests/gif_decode_model.py) on the CPU: against the hand-derived known answers of
tests/golden/gif_dec_kats.json, against Pillow on a seeded corpus of Pillow-written GIFs (indices and palette colours), and on the
streams of the GIF encoder model (tests/gif_model.py), which must decode back to the indices they encode.  The GPU decoder is held to
this model in test_gif_decode_gpu.py.  Also: the new ABI entries are exported and refuse NULL arguments without a GPU."""
import io
import json
import os

import numpy as np
import pytest

import gif_corpus
import gif_decode_model as dm
import gif_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "gif_dec_kats.json")) as f:
    KATS = json.load(f)


@pytest.mark.parametrize("k", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(k):
    r = dm.decode(bytes.fromhex(k["data"]))
    assert r["ok"] == k["ok"], r["error"]
    if not k["ok"]:
        assert r["error"] and r["stage"] in ("container", "lzw")
        return
    assert list(r["rect"]) == k["rect"]
    assert r["index"].ravel().tolist() == k["index"]
    n = len(k["palette"])
    assert r["pal_len"] == n
    np.testing.assert_array_equal(r["palette"][:min(n, 256)], np.array(k["palette"], np.uint8).reshape(-1, 4)[:256])
    assert not r["palette"][n:].any()


def test_known_answers_cover_the_rules():
    names = " ".join(k["name"] for k in KATS)
    for word in ("kwkwk", "GIF87a", "clear in mid-stream", "full dictionary", "missing EOF", "after the last pixel", "runs past",
                 "1-byte sub-block", "transparent index past", "local table", "interlaced h=9", "unknown extension", "second frame"):
        assert word in names, word
    assert {k["name"] for k in KATS if k["name"].startswith("lit ")} >= {"lit %d literals" % n for n in range(2, 9)}


def _pillow(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.format == "GIF"
    im.seek(0)
    return np.array(im.convert("P") if im.mode != "P" else im), np.array(im.getpalette()[:768], np.uint8).reshape(-1, 3)


@pytest.mark.parametrize("name,data", gif_corpus.corpus(), ids=[c[0] for c in gif_corpus.corpus()])
def test_pillow_agrees(name, data):
    r = dm.decode(data)
    assert r["ok"], r["error"]
    idx, pal = _pillow(data)
    np.testing.assert_array_equal(r["index"], idx)
    used = np.unique(idx)
    opaque = used[r["palette"][used, 3] == 255]
    np.testing.assert_array_equal(r["palette"][opaque, :3], pal[opaque])
    assert dm.entry_status(r) == dm.OK


def test_pillow_transparency_is_the_zero_colour():
    data = gif_corpus.make(40, 30, 5, ncol=16, transparency=True)
    r = dm.decode(data)
    from PIL import Image
    t = Image.open(io.BytesIO(data)).info["transparency"]
    assert r["ok"] and tuple(r["palette"][t]) == (0, 0, 0, 0)
    assert (r["palette"][:r["pal_len"]][np.arange(r["pal_len"]) != t, 3] == 255).all()


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (97, 131), (200, 200)])
def test_encoder_model_round_trip(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    idx = rng.integers(0, 256, (h, w), dtype=np.uint8)
    idx[h // 4:h // 2, :] = 7                    # long runs: long strings, clear codes on the larger frames
    r = dm.decode(gm.encode_index(idx))
    assert r["ok"], r["error"]
    np.testing.assert_array_equal(r["index"], idx)
    np.testing.assert_array_equal(r["palette"][:, :3], gm.PLAN9)


def test_truncations_never_pass_as_ok_with_other_pixels():
    data = gif_corpus.make(23, 11, 3, ncol=16)
    full = dm.decode(data)
    for cut in range(len(data)):
        r = dm.decode(data[:cut])
        if r["ok"]:   # only a cut inside the trailer region can still decode, to the same image
            np.testing.assert_array_equal(r["index"], full["index"])


def test_entry_status_mapping():
    kat = {k["name"]: bytes.fromhex(k["data"]) for k in KATS}
    assert dm.entry_status(dm.decode(kat["frame at an origin"])) == dm.UNSUPPORTED
    assert dm.entry_status(dm.decode(kat["empty frame"])) == dm.UNSUPPORTED
    assert dm.entry_status(dm.decode(kat["lit2 kwkwk"]), (3, 3)) == dm.UNSUPPORTED
    assert dm.entry_status(dm.decode(kat["lit2 kwkwk"]), (2, 2)) == dm.OK
    assert dm.entry_status(dm.decode(kat["code above hi"])) == dm.INVALID
    assert dm.entry_status(dm.decode(kat["bad version"])) == dm.INVALID


def test_entries_exported_and_refuse_null_arguments_without_a_gpu():
    """the symbols exist, and a NULL context or NULL arguments are IPX_ERR_INVALID before any device is touched"""
    from imageprocessor_amd import build
    build.build()
    import ctypes as C
    import imageprocessor_amd as m
    L = m.lib()
    for name in ("ipx_gif_decode_batch", "ipx_gif_frames_free", "ipx_plan_run_gif_gif"):
        assert hasattr(L, name)
    w, h, st, owner, res = C.c_int(0), C.c_int(0), (C.c_int * 1)(), C.c_void_p(), C.c_void_p()
    b = m._lib.PalettedBatch()
    files = (m._lib.Bytes * 1)()
    assert L.ipx_gif_decode_batch(None, None, files, 1, C.byref(w), C.byref(h), C.byref(b), st, C.byref(owner)) == -1
    assert L.ipx_plan_run_gif_gif(None, None, 1, files, 85, None, None, None, st, C.byref(res)) == -1
    L.ipx_gif_frames_free(None, None)
