"""gif.Decode on the GPU (csrc/ipx_gif_dec.hip): ipx_gif_decode_batch byte for byte against tests/gif_decode_model.py (every index,
every palette byte, every status), the GPU encoder's streams decoded back, and ipx_plan_run_gif_gif against the merged GIF leg
(ipx_plan_run_host_paletted_gif) fed with the model's frames.  PARITY UNPINNED against Go itself."""
import json
import os

import numpy as np
import pytest

import gif_corpus
import gif_decode_model as dm
import gif_model as gm
from helpers import DEFAULT_COL, text_glyphs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "gif_dec_kats.json")) as f:
    KATS = json.load(f)


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _check_batch(ctx, files, w=0, h=0):
    """one call; every status, and every index and palette byte of the OK files, as the model says"""
    info, st = ctx.gif_decode_batch(files, w, h)
    res = [dm.decode(f) for f in files]
    bw = (w, h) if w else None
    if bw is None:
        for r in res:
            if r["stage"] != "container" and r["rect"] is not None and r["rect"][2] * r["rect"][3] > 0 and not r["rect"][0] and not r["rect"][1]:
                bw = tuple(r["rect"][2:])
                break
    want = [dm.entry_status(r, bw) for r in res]
    assert st == want
    if not any(s == dm.OK for s in st):
        assert info is None
        return st
    assert (info["w"], info["h"]) == bw
    for i, r in enumerate(res):
        if st[i] == dm.OK:
            np.testing.assert_array_equal(info["index"][i], r["index"], err_msg="file %d" % i)
            np.testing.assert_array_equal(info["palettes"][i], r["palette"], err_msg="file %d" % i)
    return st


@pytest.mark.parametrize("k", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(ctx, k):
    _check_batch(ctx, [bytes.fromhex(k["data"])])


def test_pillow_corpus(ctx):
    for name, data in gif_corpus.corpus():
        assert _check_batch(ctx, [data]) == [dm.OK], name


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (97, 131), (200, 200), (1024, 768), (1920, 1080)])
def test_sizes_noise_and_flat(ctx, w, h):
    rng = np.random.default_rng(w + 7 * h)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    flat = np.full((h, w), 77, np.uint8)          # strings of ~4k pixels at the larger sizes
    files = [gif_corpus.write(noise, 256, 1, interlace=False), gif_corpus.write(noise, 256, 2, interlace=True),
             gif_corpus.write(flat, 256, 3), gm.encode_index(flat)]
    assert _check_batch(ctx, files) == [dm.OK] * 4


def test_batch_of_mixed_files(ctx):
    """84 files of one size: photo-like, flat, solid; interlaced or not; 2 to 256 colours; transparency"""
    files = []
    for k in range(84):
        kind = ("photo", "flat", "solid")[k % 3]
        files.append(gif_corpus.make(64, 48, 500 + k, kind, ncol=(2, 3, 16, 100, 256)[k % 5], interlace=bool(k % 2),
                                     transparency=k % 4 == 1))
    assert _check_batch(ctx, files) == [dm.OK] * 84
    info, st = ctx.gif_decode_batch(files, download=False)
    try:
        assert st == [dm.OK] * 84 and info["w"] == 64 and info["batch"].stride == 64 and info["batch"].frame_stride >= 64 * 48
    finally:
        info["free"]()


def test_truncations_beside_valid_files(ctx):
    """a file cut at every byte offset, its full form between the cuts, in ONE call: the cuts get the model's statuses and the
    neighbours stay exact"""
    full = gif_corpus.make(23, 11, 3, "photo", ncol=16, interlace=True, transparency=True)
    files = []
    for cut in range(len(full)):
        files += [full[:cut], full]
    st = _check_batch(ctx, files, 23, 11)
    assert st[1::2] == [dm.OK] * len(full)
    assert dm.INVALID in st[0::2]


def _at_origin(idx):
    """gm.encode_index's stream with the image moved to x = 1 on a screen one pixel wider"""
    h, w = idx.shape
    s = bytearray(gm.encode_index(idx))
    s[6:8] = (w + 1).to_bytes(2, "little")
    assert s[13 + 768] == 0x2C
    s[13 + 768 + 1] = 1
    return bytes(s)


def test_other_size_and_origin_are_unsupported(ctx):
    rng = np.random.default_rng(2)
    same = [gif_corpus.make(40, 30, 600 + k, "photo") for k in range(6)]
    other = gif_corpus.make(41, 30, 9, "photo")
    moved = _at_origin(rng.integers(0, 256, (30, 40), dtype=np.uint8))
    files = same[:3] + [other, moved] + same[3:]
    st = _check_batch(ctx, files, 40, 30)
    assert st == [dm.OK] * 3 + [dm.UNSUPPORTED] * 2 + [dm.OK] * 3


def test_encoder_streams_round_trip(ctx):
    """ipx_gif_encode_batch_dev's streams decode on the GPU to the dither's indices, with the Plan 9 palette"""
    rng = np.random.default_rng(8)
    w, h, n = 120, 90, 4
    frames = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    frames[..., 3] = 255
    frames[1, 20:70] = (10, 200, 30, 255)
    src = ctx.alloc(frames.nbytes).upload(frames)
    streams = ctx.gif_encode_batch_dev(src.ptr, w, h, n)
    info, st = ctx.gif_decode_batch(streams)
    assert st == [dm.OK] * n
    for k in range(n):
        np.testing.assert_array_equal(info["index"][k], gm.dither_wavefront(frames[k]))
        np.testing.assert_array_equal(info["palettes"][k, :, :3], gm.PLAN9)
        assert (info["palettes"][k, :, 3] == 255).all()


def _leg_files():
    files = [gif_corpus.make(96, 64, 700 + k, ("photo", "flat")[k % 2], interlace=bool(k % 3 == 0), transparency=k % 4 == 2)
             for k in range(6)]
    files.insert(2, files[0][:len(files[0]) // 2])                           # truncated: INVALID
    files.insert(4, gif_corpus.make(95, 64, 9))                                # another size: UNSUPPORTED
    return files


def _expected_leg(plan, files, quality, want):
    res = [dm.decode(f) for f in files]
    st = [dm.entry_status(r, (plan._sw, plan._sh)) for r in res]
    ok = [i for i, s in enumerate(st) if s == dm.OK]
    idx = np.stack([res[i]["index"] for i in ok])
    pal = np.stack([res[i]["palette"] for i in ok])
    ref = plan.run_host_paletted_gif(idx, pal, quality=quality, want=want)
    out = {k: [None] * len(files) for k in ref}
    for k, v in ref.items():
        for j, i in enumerate(ok):
            out[k][i] = v[j]
    return out, st


@pytest.mark.parametrize("want", [("resize", "thumbnail", "watermark"), ("resize",), ("thumbnail",), ("watermark",),
                                  ("resize", "watermark")])
@pytest.mark.parametrize("crop", [True, False])
def test_run_gif_gif_is_the_host_decoded_leg(ctx, want, crop):
    files = _leg_files()
    gs = ctx.glyphset(text_glyphs(96, 64, n=5, width_px=60, height_px=20), DEFAULT_COL)
    plan = ctx.plan(96, 64, resize=(50, 30, False), thumbnail=(32, crop), watermark=gs)
    try:
        got, st = plan.run_gif_gif(files, quality=80, want=want)
        ref, want_st = _expected_leg(plan, files, 80, want)
        assert st == want_st and st[2] == dm.INVALID and st[4] == dm.UNSUPPORTED
        assert sorted(got) == sorted(ref)
        for k in got:
            assert got[k] == ref[k], k
    finally:
        plan.close()
        gs.close()


def test_run_gif_gif_chunks(ctx, monkeypatch):
    """chunks of 3 files: the statuses and streams do not depend on where the chunks fall"""
    files = _leg_files() * 2
    plan = ctx.plan(96, 64, resize=(40, 40, True), thumbnail=(24, True))
    try:
        whole, st = plan.run_gif_gif(files)
        monkeypatch.setenv("IPX_HOST_CHUNK_GIF", "3")
        parts, st2 = plan.run_gif_gif(files)
        assert st == st2 and whole == parts
        assert all(v is None for k in whole for v, s in zip(whole[k], st) if s != dm.OK)
    finally:
        plan.close()


def test_empty_and_bad_arguments(ctx):
    import ctypes as C
    import imageprocessor_amd as m
    L = m.lib()
    plan = ctx.plan(8, 8, resize=(4, 4, False))
    try:
        for run in (plan.run_gif_gif, plan.run_jpeg_jpeg, plan.run_png_png):
            out, st0 = run([])
            assert st0 == [] and "resize" in out and all(v == [] for v in out.values()), run.__name__
        assert ctx.gif_decode_batch([]) == (None, [])
        files = (m._lib.Bytes * 1)()
        st = (C.c_int * 1)(7)
        res, owner = C.c_void_p(), C.c_void_p()
        w, h = C.c_int(0), C.c_int(0)
        b = m._lib.PalettedBatch()
        assert L.ipx_plan_run_gif_gif(ctx.handle, None, 1, files, 85, None, None, None, st, C.byref(res)) == -1
        assert L.ipx_plan_run_gif_gif(ctx.handle, plan.handle, -1, files, 85, None, None, None, st, C.byref(res)) == -1
        assert L.ipx_plan_run_gif_gif(ctx.handle, plan.handle, 1, None, 85, None, None, None, st, C.byref(res)) == -1
        assert L.ipx_plan_run_gif_gif(ctx.handle, plan.handle, 1, files, 85, None, None, None, None, C.byref(res)) == -1
        assert L.ipx_gif_decode_batch(ctx.handle, None, None, 1, C.byref(w), C.byref(h), C.byref(b), st, C.byref(owner)) == -1
        assert L.ipx_gif_decode_batch(ctx.handle, None, files, 1, None, C.byref(h), C.byref(b), st, C.byref(owner)) == -1
        assert L.ipx_gif_decode_batch(ctx.handle, None, files, 1, C.byref(w), C.byref(h), None, st, C.byref(owner)) == -1
        assert L.ipx_gif_decode_batch(ctx.handle, None, files, 1, C.byref(w), C.byref(h), C.byref(b), st, None) == -1
        bad_w = C.c_int(5)
        assert L.ipx_gif_decode_batch(ctx.handle, None, files, 1, C.byref(bad_w), C.byref(h), C.byref(b), st, C.byref(owner)) == -1
        assert st[0] == 7      # nothing was written
        # a NULL file is INVALID, not an error of the call
        info, s = ctx.gif_decode_batch([b""])
        assert info is None and s == [dm.INVALID]
    finally:
        plan.close()
