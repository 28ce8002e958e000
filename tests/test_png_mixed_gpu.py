"""PNG uploads of mixed sizes in one GPU batch (csrc/ipx_png_mixed.hip, the mixed entries of csrc/ipx_png_dec_runtime.hip and csrc/ipx_png_legs.hip):
ipx_png_decode_mixed against tests/png_decode_model.py, ipx_png_encode_mixed_dev byte for byte against tests/png_model.py and the uniform
entries, and ipx_run_png_png_mixed against the uniform leg run per size group with a plan of that size (the uniform leg is itself pinned
to the models by tests/test_png_decode_gpu.py and tests/test_texts_gpu.py)."""
import ctypes as C
import io
import json
import os
import random
import zlib

import numpy as np
import pytest

import png_adam7_corpus as ac
import png_corpus as pc
import png_decode_model as dm
import png_model as pm
from test_png_gpu import _frame

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "png_dec_kats.json")) as f:
    KATS = json.load(f)


@pytest.fixture(scope="module")
def ipx():
    import imageprocessor_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(ipx):
    c = ipx.Context(lanes=2)
    yield c
    c.close()


# ---- decode ----------------------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (5, 1), (33, 7), (64, 64)]
# one PNG type per frame kind: *image.Gray, NRGBA, RGBA, Paletted, Gray16, RGBA64, NRGBA64
KIND_TYPES = [(0, 8, False), (4, 8, False), (2, 8, False), (3, 8, True), (0, 16, False), (2, 16, False), (6, 16, False)]


def _bad_crc(data):
    i = data.index(b"IDAT")
    n = int.from_bytes(data[i - 4:i], "big")
    b = bytearray(data)
    b[i + 4 + n] ^= 0x40
    return bytes(b)


def _bad_zlib(data):
    """a byte in the middle of the zlib stream flipped, the chunk's CRC made right again: the inflate or the Adler-32 fails"""
    i = data.index(b"IDAT")
    n = int.from_bytes(data[i - 4:i], "big")
    b = bytearray(data)
    b[i + 4 + n // 2] ^= 0x55
    b[i + 4 + n:i + 8 + n] = zlib.crc32(bytes(b[i:i + 4 + n])).to_bytes(4, "big")
    return bytes(b)


def _model(f):
    try:
        return dm.decode(f, fast=True)           # zlib's inflate for the streams it takes
    except Exception:
        return dm.decode(f)


@pytest.fixture(scope="module")
def decode_case():
    """the files of one mixed call, the model's answer for each, and where the Adam7 file and its twin are"""
    files = []
    for s, (w, h) in enumerate(SIZES):
        for k, (ct, dp, tr) in enumerate(KIND_TYPES):
            files.append(pc.of_type(ct, dp, tr, h, w, seed=900 + 10 * s + k, kind=("photo", "flat")[(s + k) % 2], filters=((s + k) % 5,)))
    files.append(pc.of_type(3, 4, True, 7, 33, seed=77, kind="flat"))          # a second palette, of another size than the 5 x 1 pal8's
    files.append(pc.of_type(3, 8, True, 1, 5, seed=78, kind="photo"))
    good = pc.of_type(6, 8, False, 7, 33, seed=31, filters=(0, 1, 2, 3, 4))
    files += [_bad_crc(good), _bad_zlib(good), good[:len(good) - 20]]
    twin = ac.of_type(2, 8, False, 7, 33, seed=5, interlace=False)
    files += [ac.of_type(2, 8, False, 7, 33, seed=5), twin]
    adam7, twin_at = len(files) - 2, len(files) - 1
    oks = [bytes.fromhex(k["data"]) for k in KATS if k["status"] == dm.OK]
    assert len(oks) > 20
    # the known answers between the others: one after every second file
    mixed, at, q = [], {}, 0
    for i, f in enumerate(files):
        at[i] = len(mixed)
        mixed.append(f)
        if i % 2 == 1 and q < len(oks):
            mixed.append(oks[q])
            q += 1
    mixed += oks[q:]
    res = [_model(f) for f in mixed]
    kinds = {r["kind"] for r in res if r["status"] == dm.OK}
    assert kinds == set(range(7))
    pals = [r["palette"].tobytes() for r in res if r["status"] == dm.OK and r["kind"] == dm.PALETTED]
    assert len(set(pals)) >= 3
    st = [r["status"] for r in res]
    assert st[at[adam7]] == dm.UNSUPPORTED and st[at[twin_at]] == dm.OK
    assert [st[at[adam7 - 3 + j]] for j in range(3)] == [dm.INVALID] * 3
    return mixed, res, at[adam7], at[twin_at]


def _check_decode(ctx, files, res, adam7=None, twin=None):
    frames, st = ctx.png_decode_mixed(files)
    want = [r["status"] for r in res]
    if adam7 is not None:
        want[adam7] = dm.OK
    assert st == want
    for i, r in enumerate(res):
        fr = frames[i]
        if st[i] != dm.OK:
            assert fr is None, "file %d" % i
            continue
        r = res[twin] if i == adam7 else r
        assert (fr["w"], fr["h"], fr["kind"], fr["stride"]) == (r["w"], r["h"], r["kind"], r["w"] * dm.BPP[r["kind"]]), "file %d" % i
        np.testing.assert_array_equal(fr["pix"], r["pix"].reshape(fr["pix"].shape), err_msg="file %d" % i)
        if r["kind"] == dm.PALETTED:
            np.testing.assert_array_equal(fr["palette"], r["palette"], err_msg="file %d" % i)
        else:
            assert fr["palette"] is None


@pytest.mark.parametrize("env", [{}, {"IPX_PNG_PAR": "1"}, {"IPX_PNG_DEC_SCRATCH_MB": "0"}, {"IPX_PNG_PAR": "1", "IPX_PNG_DEC_SCRATCH_MB": "0"}],
                         ids=["plain", "par", "scratch-groups", "par-scratch-groups"])
def test_decode_mixed_matches_model(ctx, decode_case, monkeypatch, env):
    """every size and kind, broken files and the known answers in one call: no file's status depends on its neighbours"""
    files, res, _, _ = decode_case
    for k in ("IPX_PNG_ADAM7", "IPX_PNG_PAR", "IPX_PNG_DEC_SCRATCH_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_decode(ctx, files, res)


def test_decode_mixed_reversed_and_adam7(ctx, decode_case, monkeypatch):
    files, res, adam7, twin = decode_case
    monkeypatch.delenv("IPX_PNG_ADAM7", raising=False)
    _check_decode(ctx, files[::-1], res[::-1])
    monkeypatch.setenv("IPX_PNG_ADAM7", "1")           # the Adam7 file now decodes to its twin's frame
    _check_decode(ctx, files, res, adam7, twin)
    monkeypatch.setenv("IPX_PNG_PAR", "1")
    _check_decode(ctx, files, res, adam7, twin)


def test_decode_mixed_frames_are_aligned_and_device_resident(ctx, decode_case):
    files, res, _, _ = decode_case
    frames, st, free = ctx.png_decode_mixed(files, download=False)
    try:
        ok = [f for f in frames if f is not None]
        assert len(ok) == st.count(dm.OK) > 40
        assert all(f["pix"] % 256 == 0 for f in ok)
        assert len({f["pix"] for f in ok}) == len(ok)
        assert all((f["palette"] is not None and f["palette"] != 0) == (f["kind"] == dm.PALETTED) for f in ok)
    finally:
        free()


def test_decode_mixed_arguments(ipx, ctx):
    assert ctx.png_decode_mixed([]) == ([], [])
    junk = [b"", b"not a png at all", dm.SIG]
    frames, st = ctx.png_decode_mixed(junk)
    assert frames == [None] * 3 and st == [dm.decode(f)["status"] for f in junk] and dm.OK not in st
    from imageprocessor_amd import _lib
    L = ipx.lib()
    owner = C.c_void_p(1)
    assert L.ipx_png_decode_mixed(ctx.handle, None, None, 1, None, None, C.byref(owner)) == -1
    arr = (_lib.Bytes * 1)()
    fr = (_lib.PngFrame * 1)()
    st1 = (C.c_int * 1)()
    assert L.ipx_png_decode_mixed(ctx.handle, None, arr, 65536, fr, st1, C.byref(owner)) == -4


# ---- encode ----------------------------------------------------------------------------------------------------------------------

def _encode_frames():
    one_alpha = _frame(256, 200, 41, "mixed")
    one_alpha[100, 77] = (0x10, 0x20, 0xFE, 0xFE)                 # a single alpha byte 0xfe: colour type 6, 1025-byte rows
    transparent = np.zeros((1, 1, 4), np.uint8)
    return [_frame(1, 1, 1, "mixed"), transparent, _frame(3, 2, 2, "alpha"), _frame(200, 200, 3, "mixed"), _frame(256, 200, 4, "mixed"),
            one_alpha, _frame(97, 61, 5, "noise"), _frame(64, 48, 6, "flat"), _frame(17, 300, 7, "alpha")]


@pytest.fixture(scope="module")
def encode_case(ctx):
    """the frames, the model's stream of each, and one device buffer that holds them with strides beyond their rows, each starting 4, 8
    or 12 bytes past a 16-byte boundary"""
    frames = _encode_frames()
    want = [pm.png_encode(f) for f in frames]
    at, places = 0, []
    for i, f in enumerate(frames):
        h, w = f.shape[:2]
        stride = w * 4 + 4 * (1 + i % 5)
        at = (at + 15) // 16 * 16 + (4, 8, 12)[i % 3]
        places.append((at, w, h, stride))
        at += stride * h
    host = np.full(at + 64, 0xA5, np.uint8)
    for f, (o, w, h, stride) in zip(frames, places):
        host[o:o + stride * h].reshape(h, stride)[:, :w * 4] = f.reshape(h, w * 4)
    d = ctx.alloc(host.nbytes).upload(host)
    assert d.ptr % 16 == 0
    return frames, want, d, [(d.ptr + o, w, h, stride) for o, w, h, stride in places]


def test_encode_mixed_matches_model_and_uniform(ctx, encode_case):
    frames, want, d, dev = encode_case
    assert sorted({p % 16 for p, _, _, _ in dev}) == [4, 8, 12]
    got = ctx.png_encode_mixed_dev(dev)
    for i in range(len(frames)):
        assert got[i] == want[i], "frame %d" % i
    # colour types and segments as the case intends: 2 / 6, and one, two and three IDAT segments (+ the Adler-32 chunk)
    idats = [[k for k, _ in pm.read_chunks(s)].count(b"IDAT") - 1 for s in got]
    assert idats[3:6] == [1, 2, 3]
    assert [s[25] for s in got[:6]] == [2, 6, 6, 2, 2, 6]
    assert len(got[6]) == pm.stream_bound(97, 61, 3)              # the noise frame went out stored
    from PIL import Image
    for i in (2, 5, 8):
        bpp, raw = pm.raw_rows(frames[i])
        np.testing.assert_array_equal(np.array(Image.open(io.BytesIO(got[i]))), raw.reshape(frames[i].shape[0], frames[i].shape[1], bpp))
    # every frame alone through the uniform device entry, and through the host entry
    for i, (p, w, h, stride) in enumerate(dev):
        assert ctx.png_encode_batch_dev(p, w, h, 1, stride=stride, frame_stride=0) == [got[i]], "frame %d" % i
        assert ctx.png_encode_mixed_dev([dev[i]]) == [ctx.png_encode(frames[i])], "frame %d" % i


def test_encode_mixed_order_does_not_matter(ctx, encode_case):
    frames, want, d, dev = encode_case
    order = list(range(len(dev)))
    random.Random(7).shuffle(order)
    assert order != sorted(order)
    got = ctx.png_encode_mixed_dev([dev[i] for i in order])
    assert got == [want[i] for i in order]
    twice = ctx.png_encode_mixed_dev(dev + dev[::-1])              # the same frame at two places of one call
    assert twice == want + want[::-1]
    views, release = ctx.png_encode_mixed_dev(dev, copy=False)
    assert [bytes(v) for v in views] == want
    release()
    assert ctx.png_encode_mixed_dev([]) == []


def test_encode_mixed_offsets_and_bad_arguments(ipx, ctx, encode_case):
    from imageprocessor_amd import _lib
    frames, want, d, dev = encode_case
    L = ipx.lib()
    n = len(dev)
    arr = (_lib.RgbaFrame * n)(*[_lib.RgbaFrame(*f) for f in dev])
    blob, offs, lens = C.c_void_p(), (C.c_size_t * n)(), (C.c_size_t * n)()
    assert L.ipx_png_encode_mixed_dev(ctx.handle, arr, n, C.byref(blob), offs, lens) == 0
    assert all(o % 16 == 0 for o in offs) and list(lens) == [len(s) for s in want]
    assert all(offs[i] + lens[i] <= offs[i + 1] for i in range(n - 1))
    assert [C.string_at(blob.value + offs[i], lens[i]) for i in range(n)] == want
    L.ipx_host_free(ctx.handle, blob)
    p, w, h, stride = dev[3]
    bad = [(None, w, h, stride), (p, 0, h, stride), (p, w, 0, stride), (p, w, h, w * 4 - 4), (p + 1, w, h, stride), (p, w, h, stride + 2),
           (p, -3, h, stride)]
    for b in bad:                                                   # one bad frame among good ones refuses the whole call
        arr = (_lib.RgbaFrame * 3)(_lib.RgbaFrame(*dev[0]), _lib.RgbaFrame(*b), _lib.RgbaFrame(*dev[1]))
        blob = C.c_void_p(1)
        assert L.ipx_png_encode_mixed_dev(ctx.handle, arr, 3, C.byref(blob), offs, lens) == -1, b
        assert blob.value is None
    arr = (_lib.RgbaFrame * 2)(_lib.RgbaFrame(*dev[0]), _lib.RgbaFrame(p, 70000, 1, 280000))
    assert L.ipx_png_encode_mixed_dev(ctx.handle, arr, 2, C.byref(blob), offs, lens) == -4      # beyond ipx_frame_supported
    assert L.ipx_png_encode_mixed_dev(ctx.handle, arr, 65536, C.byref(blob), offs, lens) == -4  # more than 65535 frames
    arr = (_lib.RgbaFrame * 1)(_lib.RgbaFrame(*dev[0]))
    assert L.ipx_png_encode_mixed_dev(ctx.handle, arr, 1, None, offs, lens) == -1
    assert L.ipx_png_encode_mixed_dev(ctx.handle, None, 1, C.byref(blob), offs, lens) == -1
    assert L.ipx_png_encode_mixed_dev(ctx.handle, arr, -1, C.byref(blob), offs, lens) == -1


# ---- the leg ---------------------------------------------------------------------------------------------------------------------

LEG_SIZES = [(64, 48), (48, 64), (200, 150), (5, 1)]
LEG_TYPES = [(0, 8, False), (2, 8, False), (6, 8, False)]           # *image.Gray, RGBA, NRGBA
RESIZE, THUMB = (32, 24, True), (16, True)
OPS = {"resize": RESIZE, "thumbnail": THUMB, "watermark": True}
OUTS = ("resize", "thumbnail", "watermark")


def _text_for(ipx, i, w, h):
    """two glyphs anchored for a w x h frame as the watermarker anchors its text, in a colour of file i's own"""
    rng = np.random.default_rng(4000 + i)
    px, py = ipx.watermark_anchor("bottom-right", w, h, 16, 9)
    glyphs = []
    for g in range(2):
        m = rng.integers(0, 256, (9, 7), dtype=np.uint8)
        m[rng.random((9, 7)) < 0.3] = 255
        x0, y0 = px + 8 * g, py - 9
        glyphs.append({"mask": m, "dr": (x0, y0, x0 + 7, y0 + 9), "mp": (0, 0)})
    return glyphs, tuple(int(v) for v in rng.integers(1, 256, 4))


@pytest.fixture(scope="module")
def leg_case(ipx, ctx):
    """24 files of four sizes and three kinds, interleaved; a text per file; and what the uniform leg makes of every size group with a
    plan of that size, without and with the texts"""
    files, sizes = [], []
    for i in range(24):
        w, h = LEG_SIZES[i % 4]
        ct, dp, tr = LEG_TYPES[(i // 4) % 3]
        files.append(pc.of_type(ct, dp, tr, h, w, seed=1200 + i, kind=("photo", "flat")[i % 2], filters=(i % 5,)))
        sizes.append((w, h))
    texts = [_text_for(ipx, i, *sizes[i]) for i in range(24)]
    plain = {k: [None] * 24 for k in OUTS}
    texted = {k: [None] * 24 for k in OUTS}
    status = [None] * 24
    for w, h in LEG_SIZES:
        idx = [i for i in range(24) if sizes[i] == (w, h)]
        plan = ctx.plan(w, h, resize=RESIZE, thumbnail=THUMB, watermark=True)
        try:
            out, st = plan.run_png_png([files[i] for i in idx])
            outt, stt = plan.run_png_png([files[i] for i in idx], texts=[texts[i] for i in idx])
        finally:
            plan.close()
        assert st == stt == [0] * len(idx) and set(out) == set(outt) == set(OUTS)
        for j, i in enumerate(idx):
            status[i] = st[j]
            for k in OUTS:
                plain[k][i], texted[k][i] = out[k][j], outt[k][j]
    assert all(s is not None for k in OUTS for s in plain[k] + texted[k])
    assert any(plain["watermark"][i] != texted["watermark"][i] for i in range(24))
    return files, sizes, texts, plain, texted, status


def _clear_env(monkeypatch):
    for k in ("IPX_PNG_ADAM7", "IPX_PNG_PAR", "IPX_PNG_DEC_SCRATCH_MB", "IPX_PNG_MIXED_CHUNK_MB", "IPX_HOST_CHUNK_PNG_DEC", "IPX_HOST_CHUNK_PNG"):
        monkeypatch.delenv(k, raising=False)


def test_leg_matches_uniform_leg_per_size(ctx, leg_case, monkeypatch):
    files, sizes, texts, plain, texted, status = leg_case
    _clear_env(monkeypatch)
    got, st = ctx.run_png_png_mixed(OPS, files)
    assert st == status
    for k in OUTS:
        for i in range(24):
            assert got[k][i] == plain[k][i], (k, i, sizes[i])
    got, st = ctx.run_png_png_mixed(OPS, files, texts=texts)
    assert st == status
    for k in OUTS:
        for i in range(24):
            assert got[k][i] == texted[k][i], (k, i, sizes[i])


@pytest.mark.parametrize("env", [{"IPX_PNG_MIXED_CHUNK_MB": "0"}, {"IPX_PNG_MIXED_CHUNK_MB": "1", "IPX_HOST_CHUNK_PNG_DEC": "4"},
                                 {"IPX_HOST_CHUNK_PNG_DEC": "5", "IPX_PNG_PAR": "1"}], ids=["chunk-per-file", "chunks-and-groups", "groups-par"])
def test_leg_cuts_do_not_change_the_streams(ctx, leg_case, monkeypatch, env):
    """chunks and decode groups that end inside a size run (six files per size and kind pair ... two per run): the same bytes"""
    files, sizes, texts, plain, texted, status = leg_case
    _clear_env(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, st = ctx.run_png_png_mixed(OPS, files, texts=texts)
    assert st == status and got == texted


def test_leg_broken_and_interlaced_neighbours(ctx, leg_case, monkeypatch):
    files, sizes, texts, plain, texted, status = leg_case
    _clear_env(monkeypatch)
    good = pc.of_type(2, 8, False, 48, 64, seed=9)
    il = ac.of_type(2, 8, False, 48, 64, seed=10)
    batch = files[:5] + [_bad_zlib(good)] + files[5:11] + [il] + files[11:]
    got, st = ctx.run_png_png_mixed(OPS, batch)
    assert st[5] == dm.INVALID and st[12] == dm.UNSUPPORTED
    keep = [i for i in range(26) if i not in (5, 12)]
    assert [st[i] for i in keep] == status
    for k in OUTS:
        assert got[k][5] is None and got[k][12] is None
        assert [got[k][i] for i in keep] == plain[k], k
    # under IPX_PNG_ADAM7=1 the interlaced file is its twin
    monkeypatch.setenv("IPX_PNG_ADAM7", "1")
    got7, st7 = ctx.run_png_png_mixed(OPS, batch)
    twin, st_twin = ctx.run_png_png_mixed(OPS, [ac.of_type(2, 8, False, 48, 64, seed=10, interlace=False)])
    assert st7[12] == dm.OK and st_twin == [dm.OK] and all(got7[k][12] == twin[k][0] for k in OUTS)
    assert all([got7[k][i] for i in keep] == plain[k] for k in OUTS)


def test_leg_want_subsets_and_absent_operators(ipx, ctx, leg_case, monkeypatch):
    files, sizes, texts, plain, texted, status = leg_case
    _clear_env(monkeypatch)
    got, st = ctx.run_png_png_mixed(OPS, files[:9], want=("thumbnail",))
    assert st == status[:9] and got == {"thumbnail": plain["thumbnail"][:9]}
    lens, _ = ctx.run_png_png_mixed(OPS, files[:9], want=("resize", "watermark"), copy=False, texts=texts[:9])
    assert lens == {k: [len(s) for s in texted[k][:9]] for k in ("resize", "watermark")}
    # an operator ops does not ask for gives {NULL, 0}; texts without the watermark operator are checked and draw nothing
    got, st = ctx.run_png_png_mixed({"resize": RESIZE}, files[:9], texts=texts[:9])
    assert st == status[:9] and got["resize"] == plain["resize"][:9]
    assert got["thumbnail"] == [None] * 9 and got["watermark"] == [None] * 9
    assert ctx.run_png_png_mixed(OPS, []) == ({k: [] for k in OUTS}, [])
    # a size whose plan makes an empty output (400 x 1 kept in aspect inside 32 x 24: a height of 0; the plan is made all the same):
    # that file has no resize stream, as in the uniform leg, and its neighbours have theirs
    wide = pc.of_type(2, 8, False, 1, 400, seed=3)
    plan = ctx.plan(400, 1, resize=RESIZE, thumbnail=THUMB, watermark=True)
    try:
        assert plan.info.resize_bytes == 0
        alone, st1 = plan.run_png_png([wide])
    finally:
        plan.close()
    got, st = ctx.run_png_png_mixed(OPS, [files[0], wide, files[1]])
    assert st == [0, 0, 0] == st1 * 3
    for k in OUTS:
        assert got[k] == [plain[k][0], alone.get(k, [None])[0], plain[k][1]], k
    assert got["resize"][1] is None and got["thumbnail"][1] is not None


@pytest.mark.parametrize("env", [{}, {"IPX_PNG_MIXED_CHUNK_MB": "0", "IPX_HOST_CHUNK_PNG_DEC": "3"}], ids=["whole", "cut"])
def test_leg_paletted_and_16_bit_kinds(ctx, monkeypatch, env):
    """palette files of two sizes (their palettes take consecutive slots across a decode group and a run reads its own) and the 16-bit
    kinds through a run's source description, between 8-bit files: every stream as the uniform leg makes it for that size group"""
    _clear_env(monkeypatch)
    types = {"pal8": (3, 8, True), "pal4": (3, 4, True), "g16": (0, 16, False), "rgb16": (2, 16, False), "rgba16": (6, 16, False),
             "rgb8": (2, 8, False), "g8": (0, 8, False)}
    spec = [("pal8", 33, 7), ("g16", 40, 30), ("rgb8", 33, 7), ("pal4", 40, 30), ("rgba16", 33, 7), ("pal8", 40, 30), ("rgb16", 40, 30),
            ("pal4", 33, 7), ("g8", 40, 30), ("pal8", 33, 7), ("rgba16", 40, 30), ("pal8", 40, 30), ("g16", 33, 7), ("pal4", 40, 30)]
    files = [pc.of_type(*types[t], h, w, seed=2100 + i, kind=("photo", "flat")[i % 2]) for i, (t, w, h) in enumerate(spec)]
    kinds = {_model(f)["kind"] for f in files}
    assert {dm.PALETTED, dm.GRAY16, dm.RGBA64, dm.NRGBA64} <= kinds
    assert len({_model(f)["palette"].tobytes() for f in files if _model(f)["kind"] == dm.PALETTED}) >= 4
    want = {k: [None] * len(files) for k in OUTS}
    for w, h in ((33, 7), (40, 30)):
        idx = [i for i, s in enumerate(spec) if s[1:] == (w, h)]
        plan = ctx.plan(w, h, resize=RESIZE, thumbnail=THUMB, watermark=True)
        try:
            out, st = plan.run_png_png([files[i] for i in idx])
        finally:
            plan.close()
        assert st == [0] * len(idx)
        for j, i in enumerate(idx):
            for k in OUTS:
                want[k][i] = out[k][j]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, st = ctx.run_png_png_mixed(OPS, files)
    assert st == [0] * len(files)
    for k in OUTS:
        for i in range(len(files)):
            assert got[k][i] == want[k][i], (k, i, spec[i])


def test_leg_a_size_no_plan_can_be_made_for(ipx, ctx, leg_case, monkeypatch):
    """a resize output beyond the frames the kernels address: ipx_plan_create refuses every size, each file gets that status and no
    stream, and the call itself is IPX_OK; a broken file keeps its own status"""
    files = leg_case[0]
    _clear_env(monkeypatch)
    with pytest.raises(ipx.IpxError) as e:
        ctx.plan(64, 48, resize=(70000, 10, False), thumbnail=THUMB, watermark=True)
    assert e.value.status == dm.UNSUPPORTED
    got, st = ctx.run_png_png_mixed({"resize": (70000, 10, False), "thumbnail": THUMB, "watermark": True}, files[:6] + [b"junk"])
    assert st == [dm.UNSUPPORTED] * 6 + [dm.INVALID]
    assert all(v == [None] * 7 for v in got.values()) and set(got) == set(OUTS)


def test_leg_refuses_a_shared_glyph_list_and_a_frame_size(ipx, ctx, leg_case):
    from imageprocessor_amd import _lib, _glyph_array
    files = leg_case[0][:2]
    L = ipx.lib()
    arr, keep = _glyph_array(_text_for(ipx, 0, 64, 48)[0])
    sentinel = 0x5A5A

    def call(ops, texts=None):
        fa = ipx._bytes_array(files)
        outs = [(_lib.Bytes * 2)() for _ in range(3)]
        for o in outs:
            for j in range(2):
                o[j].len = sentinel
        st = (C.c_int * 2)(77, 77)
        res = C.c_void_p()
        rc = L.ipx_run_png_png_mixed(ctx.handle, C.byref(ops), 2, fa, texts, outs[0], outs[1], outs[2], st, C.byref(res))
        untouched = all(o[j].len == sentinel for o in outs for j in range(2)) and list(st) == [77, 77] and res.value is None
        return rc, untouched

    ops = _lib.PoolOps()
    ops.do_resize, ops.resize_w, ops.resize_h, ops.keep_aspect, ops.do_watermark = 1, 32, 24, 1, 1
    ops.glyphs, ops.n_glyphs = arr, 2
    assert call(ops) == (-1, True)
    ops.glyphs, ops.n_glyphs, ops.sw = None, 0, 64
    assert call(ops) == (-1, True)
    ops.sw, ops.sh = 0, 48
    assert call(ops) == (-1, True)
    # more than 256 glyphs in any text refuses the call
    ops.sh = 0
    g = {"mask": np.full((2, 2), 255, np.uint8), "dr": (0, 0, 2, 2), "mp": (0, 0)}
    tarr, tkeep = ipx._text_array([([g] * 257, (1, 2, 3, 4)), ([g], (1, 2, 3, 4))])
    assert call(ops, tarr) == (-4, True)


def test_leg_decodes_every_file_once(ctx, monkeypatch):
    """three sizes, two kinds, one call: the parallel inflate's counter of files that entered it grows by the files, once"""
    _clear_env(monkeypatch)
    monkeypatch.setenv("IPX_PNG_PAR", "1")
    files = [pc.of_type(*[(2, 8, False), (0, 8, False)][i % 2], *[(30, 40), (40, 30), (9, 9)][i % 3], seed=60 + i) for i in range(12)]
    files.append(b"\x89PNG\r\n\x1a\nbroken")                  # never reaches the inflate
    before = ctx.png_decode_counts()
    got, st = ctx.run_png_png_mixed(OPS, files)
    after = ctx.png_decode_counts()
    assert st == [0] * 12 + [dm.INVALID]
    assert after[0] - before[0] == 12 and after[1] + after[2] - before[1] - before[2] == 12
