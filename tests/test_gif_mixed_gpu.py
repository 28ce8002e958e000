"""GIF uploads of mixed sizes in one GPU batch (csrc/ipx_gif_mixed.hip, the mixed entries of csrc/ipx_gif_dec.hip):
ipx_gif_encode_mixed_dev against tests/gif_model.py and against ipx_gif_encode_batch_dev frame by frame, ipx_gif_decode_mixed against
tests/gif_decode_model.py and ipx_gif_decode_batch file by file (also under IPX_GIF_PAR=1), and ipx_run_gif_gif_mixed against
ipx_plan_run_gif_gif per size group with a plan of that size.  Byte for byte throughout."""
import ctypes as C

import numpy as np
import pytest

import gif_corpus
import gif_decode_model as dm
import gif_edge_corpus
import gif_model as gm
import gif_par_corpus as pc

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -4


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


# ---- encode ------------------------------------------------------------------------------------------------------------------------

def _noisy(w, h, seed):
    """gradients, noise and alpha of every value in places (premultiplied)"""
    rng = np.random.default_rng([seed, w, h])
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = (np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 3 % 256], axis=2) + rng.integers(-40, 41, (h, w, 3))).clip(0, 255)
    a = np.where(rng.random((h, w)) < 0.4, rng.integers(0, 256, (h, w)), 255)
    f = np.empty((h, w, 4), np.int64)
    f[..., :3] = rgb * a[..., None] // 255
    f[..., 3] = a
    return f.astype(np.uint8)


def _noise(w, h, seed):
    """opaque noise: indices with no structure, so the dictionary fills and clears and the stream comes near its bound"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.full((h, w, 1), 255, np.uint8)], axis=2)


# (w, h): the smallest frames; 64 x 64 is exactly one 4096-index LZW stage and 17 x 241 one index past it; one row; heights around a
# wave boundary inside a workgroup (63, 64, 65, 129, 130) and a second band at 1024 rows in flight (1025), each at a width of its own
# among its neighbours; the noise frame directly before the 1 x 1 frame.  A shuffled order, fixed.
ENC_SIZES = [(3, 65), (64, 64), (2, 1), (5, 129), (17, 241), (97, 131), (1, 1), (3, 1025), (257, 1), (5, 64), (7, 130), (1, 2), (3, 63), (3, 3)]
NOISE_AT = 5
PADDED = (1, 4, 5, 7, 10)           # frames whose rows lie 4 * w + 12 bytes apart


@pytest.fixture(scope="module")
def enc_case(ctx):
    """the frames in one device buffer, each at an offset that is a multiple of 4 but not of 256, some with padded rows; what the
    model writes for every frame (the model encodes all 14 in about a second: its share is the whole list); the mixed call's streams"""
    import imageprocessor_amd as m
    frames = [_noise(w, h, 9) if i == NOISE_AT else _noisy(w, h, 40 + i) for i, (w, h) in enumerate(ENC_SIZES)]
    descs, blocks, at = [], [], 0
    for i, f in enumerate(frames):
        h, w = f.shape[:2]
        stride = 4 * w + (12 if i in PADDED else 0)
        at = (at + 255) // 256 * 256 + 4 * (1 + i % 5)
        rows = np.full((h, stride), 0xA5, np.uint8)
        rows[:, :4 * w] = f.reshape(h, 4 * w)
        descs.append((at, w, h, stride))
        blocks.append((at, rows))
        at += rows.size
    buf = m.DevBuffer(ctx, at + 256)
    for off, rows in blocks:
        buf.upload(rows, off)
    descs = [(buf.ptr + off, w, h, stride) for off, w, h, stride in descs]
    model = [gm.encode(f) for f in frames]
    assert len(model[NOISE_AT]) > 0.85 * gm.size_bound(*ENC_SIZES[NOISE_AT])            # near its bound, clears included
    got = ctx.gif_encode_mixed_dev(descs)
    yield frames, descs, model, got
    buf.free()


def test_encode_is_the_models_and_the_uniform_entrys(ctx, enc_case):
    frames, descs, model, got = enc_case
    assert len(got) == len(frames)
    for i, d in enumerate(descs):
        assert got[i] == model[i], ("model", i, ENC_SIZES[i])
        ptr, w, h, stride = d
        assert ctx.gif_encode_batch_dev(ptr, w, h, 1, stride=stride, frame_stride=stride * h) == [got[i]], ("alone", i, ENC_SIZES[i])


def test_encode_does_not_depend_on_the_order_or_the_block(ctx, enc_case):
    frames, descs, model, got = enc_case
    assert ctx.gif_encode_mixed_dev(descs[::-1]) == got[::-1]
    views, release = ctx.gif_encode_mixed_dev(descs, copy=False)
    try:
        assert [bytes(v) for v in views] == got
        assert all(C.addressof(C.c_uint8.from_buffer(v)) % 16 == 0 for v in views)     # streams start 16-byte aligned in the block
    finally:
        release()


def test_encode_with_one_wave_per_frame(ctx, enc_case, monkeypatch):
    """IPX_GIF_WAVES=1: 64 rows in flight for every frame, so the frames of heights 63, 64, 65, 129 and 130 run one, two and three
    bands side by side in one launch and their carry rows share one arena; the bytes are the first call's"""
    frames, descs, model, got = enc_case
    monkeypatch.setenv("IPX_GIF_WAVES", "1")
    assert ctx.gif_encode_mixed_dev(descs) == got
    monkeypatch.setenv("IPX_GIF_WAVES", "16")
    assert ctx.gif_encode_mixed_dev(descs) == got


def _raw_encode(ctx, recs):
    import imageprocessor_amd as m
    n = len(recs)
    arr = (m._lib.RgbaFrame * max(n, 1))(*[m._lib.RgbaFrame(*r) for r in recs])
    blob, offs, lens = C.c_void_p(1), (C.c_size_t * max(n, 1))(), (C.c_size_t * max(n, 1))()
    rc = m.lib().ipx_gif_encode_mixed_dev(ctx.handle, arr, n, C.byref(blob), offs, lens)
    return rc, blob.value, m.lib().ipx_last_error().decode()


def test_encode_refusals(ctx, enc_case):
    frames, descs, model, got = enc_case
    good = descs[1]
    ptr, w, h, stride = good
    for bad, status in (((None, w, h, stride), INVALID), ((ptr, 0, h, stride), INVALID), ((ptr, w, 0, stride), INVALID),
                        ((ptr, w, h, 4 * w - 4), INVALID), ((ptr, 65536, 1, 4 * 65536), INVALID), ((ptr, 1, 65536, 4), INVALID)):
        rc, blob, text = _raw_encode(ctx, [good, bad, good])
        assert rc == status and not blob, bad
        if 65536 in bad[1:3]:
            assert text == "gif: image is too large to encode"
    rc, blob, _ = _raw_encode(ctx, [descs[6]] * 65536)
    assert rc == UNSUPPORTED and not blob
    rc, blob, _ = _raw_encode(ctx, [])
    assert rc == OK and not blob
    assert ctx.gif_encode_mixed_dev([]) == []


# ---- decode ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dec_case():
    """(files, what the model makes of each): the Pillow corpus below 1024 x 768, the hand-written streams at 160 x 120, and the
    streams that are invalid in their data plus a truncated file, each of those directly before a valid file of another size"""
    valid = [d for name, d in gif_corpus.corpus() if not name.startswith("1024x768")]
    edge = [c[1] for c in gif_edge_corpus.corpus(160, 120)]
    bad = [d for name, d, st in pc.redo_cases() if st != OK]
    bad.append(valid[20][:len(valid[20]) // 2])                          # 97 x 131, cut in its data
    assert len(bad) >= 6 and len(valid) > len(bad)
    files = []
    for i, v in enumerate(valid):                                        # (the failing files are 160 x 120 and 97 x 131; valid[:18] are neither)
        if i < len(bad):
            files.append(bad[i])
        files.append(v)
    files[2 * len(bad):2 * len(bad)] = edge
    res = [dm.decode(f) for f in files]
    for i, r in enumerate(res[:-1]):                                     # the interleaving holds what it promises
        if not r["ok"]:
            assert res[i + 1]["ok"] and tuple(res[i + 1]["rect"][2:]) != tuple(r["rect"][2:]), i
    return files, res


def _check_decode(ctx, files, res):
    frames, st = ctx.gif_decode_mixed(files)
    want = [dm.entry_status(r) for r in res]
    assert st == want and want.count(OK) > 40 and want.count(INVALID) >= 6
    for i, r in enumerate(res):
        if st[i] != OK:
            assert frames[i] is None, i
            continue
        f = frames[i]
        assert (f["w"], f["h"], f["stride"]) == (r["rect"][2], r["rect"][3], r["rect"][2]), i
        np.testing.assert_array_equal(f["index"], r["index"], err_msg="file %d" % i)
        np.testing.assert_array_equal(f["palette"], r["palette"], err_msg="file %d" % i)
    return frames, st


def test_decode_is_the_models_and_the_uniform_entrys(ctx, dec_case, monkeypatch):
    monkeypatch.delenv("IPX_GIF_PAR", raising=False)
    files, res = dec_case
    frames, st = _check_decode(ctx, files, res)
    for i, f in enumerate(files):
        info, st1 = ctx.gif_decode_batch([f])
        assert st1 == [st[i]], i
        if st[i] == OK:
            np.testing.assert_array_equal(info["index"][0], frames[i]["index"], err_msg="file %d" % i)
            np.testing.assert_array_equal(info["palettes"][0], frames[i]["palette"], err_msg="file %d" % i)
        else:
            assert info is None, i


def test_decode_under_the_parallel_walk(ctx, dec_case, monkeypatch):
    files, res = dec_case
    monkeypatch.setenv("IPX_GIF_PAR", "1")
    before = ctx.gif_decode_counts()
    _check_decode(ctx, files, res)
    c = [a - b for a, b in zip(ctx.gif_decode_counts(), before)]
    walked = sum(1 for r in res if r["stage"] != "container" and dm.entry_status(r) != UNSUPPORTED)
    assert c[0] == c[1] + c[2] == walked and c[1] > 0 and c[2] >= 6 and c[3] > 0


def test_decode_pointers_and_edges(ctx, dec_case):
    import imageprocessor_amd as m
    files, res = dec_case
    frames, st, free = ctx.gif_decode_mixed(files[:12] + [None, b"GIF89a"], download=False)
    try:
        assert st[12:] == [INVALID, INVALID] and frames[12] is None and frames[13] is None
        for f in frames:
            assert f is None or (f["index"] % 256 == 0 and f["palette"] % 4 == 0 and f["stride"] == f["w"])
    finally:
        free()
    assert ctx.gif_decode_mixed([]) == ([], [])
    assert ctx.gif_decode_mixed([b"junk", None]) == ([None, None], [INVALID, INVALID])
    owner = C.c_void_p(1)
    n = 65536
    assert m.lib().ipx_gif_decode_mixed(ctx.handle, None, (m._lib.Bytes * n)(), n, (m._lib.GifFrame * n)(), (C.c_int * n)(), C.byref(owner)) == UNSUPPORTED
    assert not owner.value


# ---- the leg -----------------------------------------------------------------------------------------------------------------------

LEG_SIZES = [(33, 15), (64, 48), (48, 64), (129, 65), (17, 17), (200, 120)]
OUTS = ("resize", "thumbnail", "watermark")
QUALITY = 85
LEG_ENVS = ("IPX_GIF_MIXED_GROUP", "IPX_GIF_MIXED_CHUNK_MB", "IPX_HOST_CHUNK_GIF", "IPX_GIF_PAR", "IPX_GIF_WAVES")
N_LEG = 24
BAD_DATA, BAD_CONTAINER = 7, 16      # (64 x 48: invalid in its data; no size at all: invalid in its container)


def leg_text(ipx, i, w, h):
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


def ops_of(keep_aspect, resize=None):
    return {"resize": resize or (64, 48, keep_aspect), "thumbnail": (32, True), "watermark": True}


def uniform_leg(ctx, files, sizes, keep_aspect, texts=None, resize=None):
    """ipx_plan_run_gif_gif (or its _texts twin) per size with a plan of that size -> ({operator: [bytes | None]}, statuses); a file
    without a size (sizes[i] is None: its container is invalid) is IPX_ERR_INVALID with no outputs"""
    n = len(files)
    want, status = {k: [None] * n for k in OUTS}, [INVALID if s is None else None for s in sizes]
    for w, h in sorted(set(s for s in sizes if s is not None)):
        idx = [i for i in range(n) if sizes[i] == (w, h)]
        plan = ctx.plan(w, h, resize=resize or (64, 48, keep_aspect), thumbnail=(32, True), watermark=True)
        try:
            out, st = plan.run_gif_gif([files[i] for i in idx], quality=QUALITY, texts=None if texts is None else [texts[i] for i in idx])
        finally:
            plan.close()
        for j, i in enumerate(idx):
            status[i] = st[j]
            for k in OUTS:
                want[k][i] = out.get(k, [None] * len(idx))[j]
    return want, status


@pytest.fixture(scope="module")
def leg_case(ctx):
    """24 files of six sizes, interleaved, one invalid in its data and one in its container, and what the uniform leg makes of every
    size group with a plan of that size: computed once, for both resize rules, with a text per file and without"""
    import imageprocessor_amd as ipx
    import lzw_writer as lw
    files, sizes = [], []
    for i in range(N_LEG):
        w, h = LEG_SIZES[i % 6]
        files.append(gif_corpus.make(w, h, 900 + i, ("photo", "flat")[i % 2], ncol=(256, 2, 100)[i % 3], interlace=bool(i % 4 == 1), transparency=i % 5 == 2))
        sizes.append((w, h))
    w, h = sizes[BAD_DATA]
    codes = pc.codes_of(lw.lzw(pc.noise(w, h, 5), 8)[0], 8)
    files[BAD_DATA] = pc.container(w, h, pc.palette(256, 5), 8, pc.pack(codes[:len(codes) // 2] + [257], 8))     # EOF before the frame is full
    files[BAD_CONTAINER], sizes[BAD_CONTAINER] = b"GIF89a\x10\x00\x10\x00\x00\x00\x00;", None                   # no image before the trailer
    texts = [leg_text(ipx, i, *(sizes[i] or (16, 16))) for i in range(N_LEG)]
    want = {(ka, tx): uniform_leg(ctx, files, sizes, ka, texts=texts if tx else None) for ka in (False, True) for tx in (False, True)}
    for (ka, tx), (out, st) in want.items():
        assert [i for i in range(N_LEG) if st[i] != OK] == [BAD_DATA, BAD_CONTAINER] and st[BAD_DATA] == st[BAD_CONTAINER] == INVALID
    assert want[(True, True)][0]["watermark"] != want[(True, False)][0]["watermark"] and want[(True, True)][0]["resize"] == want[(True, False)][0]["resize"]
    return files, sizes, want, texts


def clear_env(monkeypatch):
    for k in LEG_ENVS:
        monkeypatch.delenv(k, raising=False)


def check_leg(got, st, want):
    out, wst = want
    assert st == wst
    for k in OUTS:
        for i in range(len(st)):
            assert (got[k][i] is None) == (st[i] != OK) and got[k][i] == out[k][i], (k, i)


@pytest.mark.parametrize("texted", [False, True], ids=["no-texts", "a-text-per-file"])
@pytest.mark.parametrize("keep_aspect", [False, True], ids=["outputs-of-one-size", "outputs-of-many-sizes"])
def test_leg_streams_are_the_uniform_legs(ctx, leg_case, monkeypatch, keep_aspect, texted):
    """the resize and thumbnail streams are GIF and the watermark stream JPEG, all three byte for byte the uniform leg's; the watermark
    frames have the files' own sizes, so this call's JPEG encode is the mixed-size one"""
    files, sizes, want, texts = leg_case
    clear_env(monkeypatch)
    got, st = ctx.run_gif_gif_mixed(ops_of(keep_aspect), files, quality=QUALITY, texts=texts if texted else None)
    check_leg(got, st, want[(keep_aspect, texted)])
    ok = next(i for i in range(N_LEG) if st[i] == OK)
    assert got["resize"][ok][:6] == b"GIF89a" and got["thumbnail"][ok][:6] == b"GIF89a" and got["watermark"][ok][:2] == b"\xff\xd8"


@pytest.mark.parametrize("env", [{"IPX_GIF_MIXED_GROUP": "2"}, {"IPX_GIF_MIXED_CHUNK_MB": "0"}, {"IPX_GIF_MIXED_GROUP": "5", "IPX_GIF_MIXED_CHUNK_MB": "0"}],
                         ids=["groups-of-two", "chunk-per-file", "groups-of-five-chunk-per-file"])
def test_leg_small_budgets(ctx, leg_case, monkeypatch, env):
    """decode groups of two files and chunks of one: groups and chunks end inside the runs of one size, a chunk of one file takes the
    one-size JPEG encode, and the streams are the same"""
    files, sizes, want, texts = leg_case
    clear_env(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for keep_aspect in (False, True):
        got, st = ctx.run_gif_gif_mixed(ops_of(keep_aspect), files, quality=QUALITY, texts=texts)
        check_leg(got, st, want[(keep_aspect, True)])


def test_leg_one_size_outputs_and_parallel_walk(ctx, leg_case, monkeypatch):
    files, sizes, want, texts = leg_case
    clear_env(monkeypatch)
    out, wst = want[(True, False)]
    # files of one size only: one run, one chunk, the one-size JPEG encode over the whole chunk
    same = [i for i in range(N_LEG) if sizes[i] == LEG_SIZES[3]]
    got, st = ctx.run_gif_gif_mixed(ops_of(True), [files[i] for i in same], quality=QUALITY)
    assert st == [OK] * len(same) and all(got[k] == [out[k][i] for i in same] for k in OUTS)
    # each output array NULL in turn; an operator not asked for; no files
    for k in OUTS:
        keep = tuple(o for o in OUTS if o != k)
        got, st = ctx.run_gif_gif_mixed(ops_of(True), files, quality=QUALITY, want=keep)
        assert st == wst and got == {o: out[o] for o in keep}, k
    got, st = ctx.run_gif_gif_mixed({"resize": (64, 48, True)}, files, quality=QUALITY)
    assert st == wst and got == {"resize": out["resize"], "thumbnail": [None] * N_LEG, "watermark": [None] * N_LEG}
    assert ctx.run_gif_gif_mixed(ops_of(True), []) == ({k: [] for k in OUTS}, [])
    # the parallel walk decodes for the leg too
    monkeypatch.setenv("IPX_GIF_PAR", "1")
    before = ctx.gif_decode_counts()
    got, st = ctx.run_gif_gif_mixed(ops_of(True), files, quality=QUALITY)
    check_leg(got, st, want[(True, False)])
    c = [a - b for a, b in zip(ctx.gif_decode_counts(), before)]
    assert c[0] == c[1] + c[2] == N_LEG - 1


def test_leg_per_file_refusals(ctx, leg_case, monkeypatch):
    import imageprocessor_amd as ipx
    files, sizes, want, texts = leg_case
    clear_env(monkeypatch)
    # one size no plan can be made for -- 600 x 1 kept in aspect inside 70000 x 120 is 69960 pixels wide, beyond the span the kernels
    # address -- among sizes that have one: that file carries ipx_plan_create's status, alone
    wide, flat = (70000, 120, True), gif_corpus.make(600, 1, 3, "photo", ncol=16, interlace=False)
    with pytest.raises(ipx.IpxError) as e:
        ctx.plan(600, 1, resize=wide, thumbnail=(32, True), watermark=True)
    assert e.value.status == UNSUPPORTED
    ref, ref_st = uniform_leg(ctx, files[:4], sizes[:4], True, resize=wide)
    got, st = ctx.run_gif_gif_mixed(ops_of(True, resize=wide), files[:2] + [flat] + files[2:4], quality=QUALITY)
    assert st == [0, 0, UNSUPPORTED, 0, 0] and ref_st == [0] * 4
    for k in OUTS:
        assert got[k][2] is None and got[k][:2] + got[k][3:] == ref[k], k


def test_leg_order_of_errors(ctx, leg_case):
    """a bad argument, then the codec's refusals (texts beside a glyph list; more than 65535 files), then the texts' own rules"""
    import imageprocessor_amd as m
    from helpers import DEFAULT_COL, text_glyphs
    files, sizes, want, texts = leg_case
    L = m.lib()
    n = 65536
    ops = m._lib.PoolOps(do_watermark=1)
    bad_text = (m._lib.Text * n)()
    bad_text[0].n_glyphs = -1
    arr, st, res = (m._lib.Bytes * n)(), (C.c_int * n)(), C.c_void_p(1)
    call = lambda files_, n_, texts_: (L.ipx_run_gif_gif_mixed(ctx.handle, C.byref(ops), n_, files_, texts_, QUALITY, None, None, None, st, C.byref(res)),
                                       L.ipx_last_error().decode())
    rc, text = call(None, n, bad_text)
    assert rc == INVALID and "bad argument" in text
    rc, text = call(arr, n, bad_text)
    assert rc == UNSUPPORTED and "65535" in text and not res.value
    rc, text = call(arr, 2, bad_text)
    assert rc == INVALID and "bad argument" not in text and "65535" not in text
    with pytest.raises(m.IpxError) as e:
        ctx.run_gif_gif_mixed({"resize": (64, 48, True), "thumbnail": (32, True), "watermark": (text_glyphs(64, 48, n=3, width_px=30, height_px=10, margin=4), DEFAULT_COL)},
                              files[:2], texts=texts[:2])
    assert e.value.status == INVALID and "glyphs" in str(e.value)
