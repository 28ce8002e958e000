"""png.Decode on the GPU (csrc/ipx_png_dec.hip): ipx_png_decode_batch on the hand-derived known answers of tests/golden/png_dec_kats.json
and byte for byte against tests/png_decode_model.py (every status, every frame byte, every palette), the GPU encoder's streams decoded back, and ipx_plan_run_png_png against the merged PNG legs fed with
the model's frames.  PARITY UNPINNED against Go itself."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

import png_corpus as pc
import png_decode_model as dm
from helpers import DEFAULT_COL, text_glyphs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "png_dec_kats.json")) as f:
    KATS = json.load(f)


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def _check_batch(ctx, files, w=0, h=0, kind=-1, fast=False):
    """one call; every status, and every frame and palette byte of the OK files, as the model says"""
    info, st = ctx.png_decode_batch(files, w, h, kind)
    res = [dm.decode(f, fast=fast) for f in files]
    size = (w, h) if w else next(((r["w"], r["h"]) for r in res if r["stage"] == "data"), None)
    k = kind if kind >= 0 else next((r["kind"] for r in res if r["stage"] == "data" and (r["w"], r["h"]) == size), None)
    want = [dm.entry_status(r, size, k) for r in res]
    assert st == want, [r["why"] for r in res]
    if not any(s == dm.OK for s in st):
        assert info is None
        return st
    assert (info["w"], info["h"], info["kind"]) == size + (k,)
    for i, r in enumerate(res):
        if st[i] == dm.OK:
            np.testing.assert_array_equal(info["pix"][i], r["pix"], err_msg="file %d" % i)
            if k == dm.PALETTED:
                np.testing.assert_array_equal(info["palettes"][i], r["palette"], err_msg="file %d" % i)
    return st


def _kat_matches(info, i, k):
    """frame i of a decoded batch holds the known answer's pixels and palette"""
    assert (info["w"], info["h"], info["kind"]) == (k["w"], k["h"], k["kind"])
    assert info["pix"][i].tobytes().hex() == k["pix"], k["name"]
    if "palette" in k:
        assert info["palettes"][i].tobytes().hex() == k["palette"], k["name"]


@pytest.mark.parametrize("k", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(ctx, k):
    """every hand-derived case through the host parse and the kernels, one call each (their sizes differ)"""
    assert _check_batch(ctx, [bytes.fromhex(k["data"])]) == [k["status"]]
    info, st = ctx.png_decode_batch([bytes.fromhex(k["data"])])
    assert st == [k["status"]]
    if k["status"] == dm.OK:
        _kat_matches(info, 0, k)
    else:
        assert info is None


def test_known_answers_between_valid_neighbours(ctx):
    """the 5 x 1 gray 8 known answers (most zlib / flate and container rules) in one batch between valid files of that size: every
    status as the model says for a batch of that size and kind, the OK ones' pixels as the known answers say, the neighbours intact"""
    ref = next(k for k in KATS if k["name"] == "valid reference file")
    same = [k for k in KATS if dm.parse(bytes.fromhex(k["data"]))[1]["w"] == 5 and dm.parse(bytes.fromhex(k["data"]))[1]["h"] == 1]
    assert len(same) > 40
    batch = [ref] + same + [ref]
    st = _check_batch(ctx, [bytes.fromhex(k["data"]) for k in batch], 5, 1, dm.GRAY)
    assert st[0] == st[-1] == dm.OK
    for k, s_ in zip(batch, st):
        if k["status"] != dm.OK or k.get("kind") == dm.GRAY:
            assert s_ == k["status"], k["name"]
    info, _ = ctx.png_decode_batch([bytes.fromhex(k["data"]) for k in batch], 5, 1, dm.GRAY)
    for i, k in enumerate(batch):
        if st[i] == dm.OK:
            _kat_matches(info, i, k)


def test_frames_beyond_the_span_are_unsupported(ctx):
    """ipx_frame_supported at the type's bytes per pixel: a side above 65535, a span above 2 GiB; 65535 x 1 still decodes"""
    def one(w, h, depth, ctype, raw):
        return dm.SIG + pc.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) + pc.chunk(b"IDAT", zlib.compress(raw)) + \
            pc.chunk(b"IEND", b"")
    wide = one(70000, 1, 8, 0, b"\x00" + bytes(70000))
    deep = one(65535, 4100, 16, 6, b"\x00")                          # 65535 x 4100 x 8 bytes: beyond 2 GiB, never inflated
    edge = one(65535, 1, 8, 0, b"\x00" + bytes(range(256)) * 255 + bytes(255))
    for f in (wide, deep):
        assert dm.decode(f)["status"] == dm.UNSUPPORTED
        assert _check_batch(ctx, [f]) == [dm.UNSUPPORTED]
    assert _check_batch(ctx, [edge]) == [dm.OK]


@pytest.mark.parametrize("name,ctype,depth,trns", pc.TYPES, ids=[t[0] for t in pc.TYPES])
def test_every_type_every_filter(ctx, name, ctype, depth, trns):
    """each row of the type table at 1x1, 1xn, nx1 and odd widths; the five filters per row; photo-like and flat"""
    files = []
    for k, (w, h) in enumerate([(1, 1), (1, 9), (9, 1), (13, 7), (37, 29), (70, 67)]):
        for fl in ((0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)):
            files.append(pc.of_type(ctype, depth, trns, h, w, seed=100 * k + len(fl), kind=("photo", "flat")[k % 2], filters=fl))
    for f in files:                              # one file per call: the sizes differ
        assert _check_batch(ctx, [f]) == [dm.OK]


@pytest.mark.parametrize("w,h,ctype,depth", [(1920, 1080, 2, 8), (8200, 3, 6, 8), (1024, 768, 6, 16), (333, 517, 3, 4)])
def test_large_frames(ctx, w, h, ctype, depth):
    """1920x1080, rows longer than the 32 KiB window (8200 x 3 RGBA 8), 16-bit and a sub-byte palette; zlib's own streams"""
    files = [pc.of_type(ctype, depth, False, h, w, seed=s, kind=kd, filters=fl, split=sp)
             for s, (kd, fl, sp) in enumerate([("photo", (0, 1, 2, 3, 4), None), ("flat", (4,), 8192), ("photo", (1, 3), "random")])]
    assert _check_batch(ctx, files, fast=True) == [dm.OK] * 3


def test_mixed_batch(ctx):
    """about 80 files of one size: the first decodable file's kind is the batch's, other kinds UNSUPPORTED, broken ones INVALID"""
    files = []
    for k in range(80):
        name, ctype, depth, trns = pc.TYPES[k % len(pc.TYPES)] if k % 3 else ("rgb8", 2, 8, False)
        f = pc.of_type(ctype, depth, trns, 48, 64, seed=700 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,), split=(None, 97, "random")[k % 3])
        if k % 11 == 5:
            f = f[:len(f) // 2]
        files.append(f)
    st = _check_batch(ctx, files)
    assert st.count(dm.OK) >= 20 and dm.INVALID in st and dm.UNSUPPORTED in st
    for kind in (dm.GRAY, dm.PALETTED, dm.NRGBA64):      # the batch's kind chosen by the caller
        assert dm.OK in _check_batch(ctx, files, 64, 48, kind)


def test_scratch_groups(ctx, monkeypatch):
    """a 1 MiB scratch budget cuts a batch into many decode groups, each released before the next: the same answers as one group"""
    files = [pc.of_type(6, 8, False, 120, 160, seed=300 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,)) for k in range(24)]
    files[7] = files[7][:-30]
    monkeypatch.setenv("IPX_PNG_DEC_SCRATCH_MB", "1")
    st = _check_batch(ctx, files)
    assert st.count(dm.OK) == 23 and st[7] == dm.INVALID


def _small(seed):
    return pc.of_type(2, 8, False, 6, 7, seed=seed, kind="photo", filters=(0, 1, 2, 3, 4), level=9)


def test_truncated_at_every_offset(ctx):
    good = _small(1)
    files = [good[:i] for i in range(len(good))]
    st = _check_batch(ctx, [good] + files + [good])
    assert st[0] == st[-1] == dm.OK and all(s == dm.INVALID for s in st[1:-1])


def _recrc(data):
    """every chunk's CRC recomputed (so a flipped byte reaches the inflater)"""
    out, i = bytearray(data[:8]), 8
    while i + 12 <= len(data):
        n = struct.unpack(">I", data[i:i + 4])[0]
        body = data[i + 4:i + 8 + n]
        out += data[i:i + 8 + n] + struct.pack(">I", zlib.crc32(body))
        i += 12 + n
    return bytes(out)


def _idat_span(data):
    i = 8
    while True:
        n = struct.unpack(">I", data[i:i + 4])[0]
        if data[i + 4:i + 8] == b"IDAT":
            return i + 8, n
        i += 12 + n


def test_flipped_idat_bytes(ctx):
    rng = np.random.default_rng(5)
    good = [pc.of_type(ct, dp, tr, 11, 23, seed=s, filters=(s % 5,), level=(0, 1, 6, 9)[s % 4], strategy=(zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED)[s % 2])
            for s, (ct, dp, tr) in enumerate([(2, 8, False), (6, 8, False), (0, 4, False), (3, 8, True)] * 3)]
    files = []
    for g in good:
        off, n = _idat_span(g)
        for _ in range(12):
            b = bytearray(g)
            p = off + int(rng.integers(0, n))
            b[p] ^= 1 << int(rng.integers(0, 8))
            files.append(_recrc(bytes(b)))
    for i in range(0, len(files), 12):
        batch = [good[i // 12]] + files[i:i + 12] + [good[i // 12]]
        st = _check_batch(ctx, batch)
        assert st[0] == st[-1] == dm.OK


def test_bad_crcs(ctx):
    good = _small(2)
    files = []
    i = 8
    while i < len(good):
        n = struct.unpack(">I", good[i:i + 4])[0]
        b = bytearray(good)
        b[i + 8 + n] ^= 0x40                     # this chunk's stored CRC
        files.append(bytes(b))
        i += 12 + n
    st = _check_batch(ctx, [good] + files + [good])
    assert st == [dm.OK] + [dm.INVALID] * len(files) + [dm.OK]


def test_round_trip_of_the_gpu_encoder(ctx):
    rng = np.random.default_rng(9)
    for w, h in [(1, 1), (31, 17), (640, 480), (8200, 3)]:
        frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2)]
        frames[1][..., 3] = 255
        for f in frames:                         # RGBA 8 (NRGBA) and RGB 8 (RGBA): one call each
            assert _check_batch(ctx, [ctx.png_encode(f)], fast=True) == [dm.OK]


def _plan(ctx, sw, sh):
    gs = ctx.glyphset(text_glyphs(sw, sh), DEFAULT_COL)
    return gs, ctx.plan(sw, sh, resize=(160, 120, True), thumbnail=(50, True), watermark=gs)


def test_leg_rgb8_equals_the_host_leg(ctx):
    sw, sh = 96, 72
    gs, plan = _plan(ctx, sw, sh)
    files = [pc.of_type(2, 8, False, sh, sw, seed=40 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,)) for k in range(6)]
    out, st = plan.run_png_png(files)
    assert st == [dm.OK] * 6
    frames = np.stack([dm.decode(f)["pix"].reshape(sh, sw, 4) for f in files])
    want = plan.run_host_png(frames)
    for k in want:
        assert out[k] == want[k], k
    plan.close()
    gs.close()


def _host_outputs(plan, kind, rs):
    sw, sh = plan._sw, plan._sh
    pix = np.stack([r["pix"] for r in rs])
    if kind == dm.GRAY:
        return plan.run_host_gray(pix)
    if kind in (dm.NRGBA,):
        return plan.run_host_nrgba(pix.reshape(len(rs), sh, sw, 4))
    if kind == dm.RGBA:
        return plan.run_host(pix.reshape(len(rs), sh, sw, 4))
    if kind == dm.PALETTED:
        return plan.run_host_paletted(pix, np.stack([r["palette"] for r in rs]))
    import imageprocessor_amd as m
    deep = {dm.GRAY16: m.DEEP_GRAY16, dm.RGBA64: m.DEEP_RGBA64, dm.NRGBA64: m.DEEP_NRGBA64}[kind]
    return plan.run_host_deep(pix, deep)


def test_leg_every_kind_mixed_with_broken_files(ctx):
    """one call with files of every kind, truncated and unsupported ones among them: the statuses, NULL outputs for non-OK files,
    and per kind the streams png.Encode makes of the matching run_host_* outputs on the model's frames"""
    sw, sh = 40, 30
    gs, plan = _plan(ctx, sw, sh)
    files = []
    for k, (name, ctype, depth, trns) in enumerate(pc.TYPES):
        files.append(pc.of_type(ctype, depth, trns, sh, sw, seed=900 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,)))
    good = files[3]
    files += [good[:-20], pc.of_type(2, 8, False, sh + 1, sw, seed=1)]
    il = bytearray(good)
    il[8 + 8 + 12] = 1                           # Adam7
    files.append(_recrc(bytes(il)))
    out, st = plan.run_png_png(files)
    rs = [dm.decode(f) for f in files]
    want = [dm.entry_status(r, (sw, sh)) for r in rs]
    assert st == want
    assert st[len(pc.TYPES)] == dm.INVALID and st[len(pc.TYPES) + 1] == dm.UNSUPPORTED and st[-1] == dm.UNSUPPORTED
    for k in out:
        for i, s in enumerate(st):
            assert (out[k][i] is None) == (s != dm.OK)
    by_kind = {}
    for i, r in enumerate(rs):
        if st[i] == dm.OK:
            by_kind.setdefault(r["kind"], []).append(i)
    assert len(by_kind) == 7
    for kind, idx in by_kind.items():
        host = _host_outputs(plan, kind, [rs[i] for i in idx])
        for k, frames in host.items():
            for j, i in enumerate(idx):
                assert out[k][i] == ctx.png_encode(frames[j]), (kind, k, i)
    plan.close()
    gs.close()


def _bad_idat_crc(data):
    """the IDAT's stored CRC flipped: the host parse accepts the file, the GPU's CRC check fails it"""
    off, n = _idat_span(data)
    b = bytearray(data)
    b[off + n] ^= 0x40
    return bytes(b)


def test_leg_chunks(ctx, monkeypatch):
    """output chunks of 2 inside decode groups of 3: the statuses and streams do not depend on where the chunks and groups fall.  Two
    files fail on the GPU (bad IDAT CRC) inside output chunks beside OK files -- one at the first slot of a decode group's first chunk,
    one at the second slot of a chunk -- so only the status mask keeps their slots unpublished; a truncated file fails in the host parse"""
    sw, sh = 40, 30
    gs, plan = _plan(ctx, sw, sh)
    rgb = [pc.of_type(2, 8, False, sh, sw, seed=60 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,)) for k in range(9)]
    rgb[3] = _bad_idat_crc(rgb[3])
    rgb[7] = _bad_idat_crc(rgb[7])
    # RGB files in order of their kind: decode groups [0 1 3] [5 6 7] [8 9 10], output chunks [0 1] [3] [5 6] [7] [8 9] [10]
    files = rgb[:2] + [pc.of_type(0, 8, False, sh, sw, seed=70)] + rgb[2:3] + [rgb[0][:-20]] + rgb[3:]
    gpu_bad, host_bad = (5, 9), 4
    try:
        whole, st = plan.run_png_png(files)
        rs = [dm.decode(f) for f in files]
        assert st == [dm.entry_status(r, (sw, sh)) for r in rs]
        assert [i for i, s in enumerate(st) if s != dm.OK] == sorted(gpu_bad + (host_bad,))
        assert all((v is None) == (s != dm.OK) for k in whole for v, s in zip(whole[k], st))
        ok_rgb = [i for i in range(len(files)) if st[i] == dm.OK and rs[i]["kind"] == rs[0]["kind"]]
        want = plan.run_host_png(np.stack([rs[i]["pix"].reshape(sh, sw, 4) for i in ok_rgb]))
        for k in want:
            assert [whole[k][i] for i in ok_rgb] == want[k], k
        monkeypatch.setenv("IPX_HOST_CHUNK_PNG", "2")
        monkeypatch.setenv("IPX_HOST_CHUNK_PNG_DEC", "3")
        parts, st2 = plan.run_png_png(files)
        assert st == st2 and whole == parts
    finally:
        plan.close()
        gs.close()


def test_bad_arguments(ctx):
    import imageprocessor_amd as m
    from imageprocessor_amd import _lib
    import ctypes as C
    b = _lib.PngBatch()
    st = (C.c_int * 1)()
    own = C.c_void_p()
    arr = (_lib.Bytes * 1)()
    w, h, k = C.c_int(0), C.c_int(0), C.c_int(9)
    assert m.lib().ipx_png_decode_batch(ctx.handle, None, arr, 1, C.byref(w), C.byref(h), C.byref(k), C.byref(b), st, C.byref(own)) == -1
    info, s = ctx.png_decode_batch([b"", b"\x89PNG"])
    assert info is None and s == [dm.INVALID, dm.INVALID]
