"""JPEG uploads of mixed sizes in one GPU batch (ipx_jpeg_decode_mixed, ipx_run_jpeg_jpeg_mixed; DESIGN.md sections 4.6 and 7).

The decode entry groups its files by sampling class and decodes each class in ONE set of launches whatever sizes it holds: the kernels
read an image's geometry from a per-image record instead of the launch arguments.  Every file's planes (over the image's MCU-padded
extent) and status are held against two references: the oracle's restatement of Go's decoder, and ipx_jpeg_decode_batch of that file
alone.  The shapes are the smallest at which the new indexing can go wrong: one live MCU, a ragged last workgroup of an MCU row,
images of one workgroup beside images of hundreds, every route among different sizes.  The leg's streams are held against
ipx_plan_run_jpeg_jpeg with a plan of each file's size."""
import io
import random

import numpy as np
import pytest

import oracle
from test_jpeg_decode import picture, pil_jpeg

INVALID, UNSUPPORTED = -1, -4
SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 17), (33, 15), (64, 48), (129, 65), (257, 40), (200, 120)]
CLASSES = ["444", "422", "420", "440", "gray"]


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


def make(w, h, cls, seed=0, **kw):
    """A w x h file of a sampling class.  Pillow cannot write 4:4:0: a 4:2:2 file of the transposed size has the same number of MCUs
    and of blocks per MCU, so with its size and its luma sampling bytes swapped it is a valid 4:4:0 stream (of other content)."""
    kw = {"quality": 85, **kw}
    if cls == "gray":
        return pil_jpeg(picture(w, h, seed=seed)[..., 0], **kw)
    if cls == "440":
        b = bytearray(pil_jpeg(picture(h, w, seed=seed), subsampling=1, **kw))
        i = b.index(b"\xff\xc2" if kw.get("progressive") else b"\xff\xc0")
        assert b[i + 11] == 0x21 and int.from_bytes(b[i + 5:i + 7], "big") == w and int.from_bytes(b[i + 7:i + 9], "big") == h
        b[i + 11] = 0x12
        b[i + 5:i + 7], b[i + 7:i + 9] = h.to_bytes(2, "big"), w.to_bytes(2, "big")
        return bytes(b)
    return pil_jpeg(picture(w, h, seed=seed), subsampling={"444": 0, "422": 1, "420": 2}[cls], **kw)


def entropy_segment(f):
    sos = f.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(f[sos + 2:sos + 4], "big")
    assert f[-2:] == b"\xff\xd9"
    return f[start:-2]


_oracle_of = {}


def oracle_of(f):
    """-> the oracle's planes, or the status Go's verdict maps to; computed once per file"""
    if f not in _oracle_of:
        try:
            d = oracle.jpeg_decode(f)
            _oracle_of[f] = UNSUPPORTED if d["dc_wide"] else d
        except ValueError as e:
            _oracle_of[f] = INVALID if "malformed" in str(e) else UNSUPPORTED
    return _oracle_of[f]


def alone(ctx, f):
    """ipx_jpeg_decode_batch of the file in a call of its own -> (planes dict | None, status)"""
    if f is None:
        return None, INVALID
    info, st = ctx.jpeg_decode_batch([f])
    if info is None or st[0] != 0:
        return None, st[0]
    d = {k: info[k] for k in ("w", "h", "ratio", "ystride", "cstride")}
    d.update({k: (info[k][0] if k in info else None) for k in ("y", "cb", "cr")})
    return d, 0


def same_planes(got, want, what):
    assert (got["w"], got["h"], got["ratio"]) == (want["w"], want["h"], want["ratio"]), what
    for k in ("y", "cb", "cr") if want["ratio"] != 4 else ("y",):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s of %s" % (k, what))
    if want["ratio"] == 4:
        assert got["cb"] is None and got["cr"] is None and got["cstride"] == 0, what


def check_mixed(ctx, files, against_alone=True, oracle_too=True):
    """one mixed call; every file against the oracle and against the uniform entry alone -> (frames, statuses)"""
    frames, st = ctx.jpeg_decode_mixed(files)
    assert len(frames) == len(st) == len(files)
    for i, f in enumerate(files):
        what = "file %d of %d" % (i, len(files))
        if f is not None and oracle_too:
            want = oracle_of(f)
            if isinstance(want, int):
                assert st[i] == want and frames[i] is None, (what, st[i], want)
            else:
                assert st[i] == 0, (what, st[i])
                same_planes(frames[i], want, what + " against the oracle")
        if against_alone:
            ref, ref_st = alone(ctx, f)
            assert st[i] == ref_st, (what, st[i], ref_st)
            if ref_st == 0:
                same_planes(frames[i], ref, what + " against the uniform entry")
                assert (frames[i]["ystride"], frames[i]["cstride"]) == (ref["ystride"], 0 if ref["ratio"] == 4 else ref["cstride"])
            else:
                assert frames[i] is None, what
    return frames, st


def all_sizes_and_classes():
    files = []
    for k, (w, h) in enumerate(SIZES):
        for j, cls in enumerate(CLASSES):
            if (k + j) % 5 in (0, 2, 3, 4):         # 40 of the 50 pairs; every size and every class several times
                files.append(make(w, h, cls, seed=k * 5 + j, **({"restart_marker_blocks": 2} if (k + j) % 7 == 0 else {})))
    return files


@pytest.mark.gpu
def test_sizes_and_classes_in_one_call(ctx):
    """Ten sizes in five classes, 40 files.  257 x 40 at 4:2:0 has 17 MCUs per row: two IDCT workgroups and a tail of one MCU; 1 x 1 is
    one workgroup with one live MCU."""
    files = all_sizes_and_classes()
    assert len(files) == 40
    frames, st = check_mixed(ctx, files)
    assert st == [0] * 40
    # an image's planes are its own block: MCU-padded strides, as image.NewYCbCr lays them out
    f = frames[[i for i, d in enumerate(frames) if (d["w"], d["h"], d["ratio"]) == (257, 40, 2)][0]]
    assert (f["ystride"], f["cstride"], f["y"].shape, f["cb"].shape) == (272, 136, (48, 272), (24, 136))


def route_files():
    par = [pil_jpeg(picture(w, h, seed=3 + w, noise=40.0), subsampling=0, quality=95) for (w, h) in ((160, 120), (320, 200))]
    pieces = [make(w, h, "444", seed=w, restart_marker_blocks=ri) for (w, h), ri in (((33, 15), 1), ((129, 65), 2), ((200, 120), 7))]
    host = [make(w, h, "444", seed=w + 1, progressive=True) for (w, h) in ((17, 17), (64, 48), (257, 40))]
    return par, pieces, host


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"IPX_JPEG_PAR": "0"}, {"IPX_JPEG_PAR": "0", "IPX_JPEG_PIECE": "0"}, {"IPX_JPEG_PAR_SUB": "128"},
                                 {"IPX_JPEG_PAR_ROUNDS": "0"}],
                         ids=["default", "pieces-only", "bytewise", "sub-128", "never-settles"])
def test_every_route_among_different_sizes(ctx, monkeypatch, env):
    """Long scans without restart markers (the parallel passes), restart intervals of 1, 2 and 7 MCUs (the piece kernels) and
    progressive files (the host route), each at several sizes, in one class and one call.  The switches move the same files to the
    piece kernels, to the byte-wise kernel, to 128-byte sub-sequences, and -- with no synchronisation round allowed -- from the
    parallel passes to the byte-wise kernel's whole-scan fallback."""
    par, pieces, host = route_files()
    for f in par:
        assert len(entropy_segment(f)) > 4 * 1024       # four times the largest sub-sequence (jpeg_par_sub_bytes)
    files = [pieces[0], par[0], host[0], pieces[1], host[1], par[1], pieces[2], host[2]]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    before = ctx.jpeg_decode_counts()
    frames, st = check_mixed(ctx, files, against_alone=False)
    after = ctx.jpeg_decode_counts()
    assert st == [0] * 8
    # every file reached its route's decoder: five baseline files the GPU's Huffman kernels, three the host's scan decoder
    assert [a - b for a, b in zip(after, before)] == [5, 3, 0, 0]
    for k in env:
        monkeypatch.delenv(k)
    for i, f in enumerate(files):
        ref, ref_st = alone(ctx, f)
        assert ref_st == 0
        same_planes(frames[i], ref, "file %d against the uniform entry" % i)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["small-then-large", "large-then-small", "large-between-1x1", "one-file"])
def test_search_edges_of_the_idct_grid(ctx, order):
    """The workgroup -> image search at its ends: thirty one-workgroup images before one of hundreds, the same reversed, a large image
    between two of one live MCU, and a call of one file."""
    small = [make(8, 8, "420", seed=i) for i in range(30)]
    large = make(400, 300, "420", seed=77)
    tiny = [make(1, 1, "420", seed=90 + i) for i in range(2)]
    files = {"small-then-large": small + [large], "large-then-small": [large] + small[::-1], "large-between-1x1": [tiny[0], large, tiny[1]],
             "one-file": [large]}[order]
    frames, st = check_mixed(ctx, files, against_alone=order != "large-then-small")
    assert st == [0] * len(files)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_order_does_not_matter(ctx, seed):
    files = all_sizes_and_classes()
    base, st0 = ctx.jpeg_decode_mixed(files)
    perm = list(range(len(files)))
    random.Random(seed).shuffle(perm)
    frames, st = ctx.jpeg_decode_mixed([files[p] for p in perm])
    assert st == [st0[p] for p in perm] == [0] * len(files)
    for k, p in enumerate(perm):
        same_planes(frames[k], base[p], "file %d at position %d" % (p, k))


@pytest.mark.gpu
def test_one_size_only(ctx):
    """eight files of 64 x 48: planes and statuses are ipx_jpeg_decode_batch's for the same call"""
    files = [make(64, 48, "420", seed=i, **({"restart_marker_blocks": 3} if i == 5 else {})) for i in range(8)]
    files[3] = files[3][:len(files[3]) // 2]
    frames, st = check_mixed(ctx, files, against_alone=False)
    info, want_st = ctx.jpeg_decode_batch(files)
    assert st == want_st and st[3] != 0 and sum(s == 0 for s in st) == 7
    for i in range(8):
        if st[i] == 0:
            for k in ("y", "cb", "cr"):
                np.testing.assert_array_equal(frames[i][k], info[k][i])
            assert (frames[i]["ystride"], frames[i]["cstride"]) == (info["ystride"], info["cstride"])


def cmyk_file(w, h):
    from PIL import Image
    img = picture(w, h)
    buf = io.BytesIO()
    Image.fromarray(np.dstack([img, img[..., :1]]), "CMYK").save(buf, "JPEG")
    return buf.getvalue()


def file_411():
    """A 64 x 32 4:2:0 file has 4 x 2 MCUs of four luma blocks; so has a 64 x 32 4:1:1 file (2 x 4 MCUs of 32 x 8): with the luma
    sampling byte changed it is a valid 4:1:1 stream."""
    b = bytearray(make(64, 32, "420", seed=5))
    i = b.index(b"\xff\xc0")
    assert b[i + 11] == 0x22
    b[i + 11] = 0x41
    return bytes(b)


def bad_code_file():
    """thirty-two 1 bits in the middle of the scan: no table of the file has a code of sixteen ones"""
    b = bytearray(make(129, 65, "420", seed=9))
    seg = entropy_segment(bytes(b))
    at = len(b) - 2 - len(seg) // 2
    b[at:at + 8] = b"\xff\x00" * 4
    return bytes(b)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"IPX_JPEG_411": "1"}, {"IPX_JPEG_PROG_GPU": "1"}], ids=["default", "411-switch", "gpu-scan-walk-switch"])
def test_neighbours(ctx, monkeypatch, env):
    """Broken and unsupported files among good ones of different sizes: each gets the status it gets alone, its frame is all zero, and
    every neighbour's planes are what they are without it.  The 4:1:1 file stays UNSUPPORTED under IPX_JPEG_411=1, and a progressive
    file stays IPX_OK on the host route, with the same planes, under IPX_JPEG_PROG_GPU=1."""
    good = [make(w, h, cls, seed=w) for (w, h), cls in (((33, 15), "420"), ((200, 120), "444"), ((64, 48), "gray"), ((129, 65), "420"), ((17, 17), "422"),
                                                         ((257, 40), "420"))]
    prog = make(129, 65, "420", seed=4, progressive=True)
    truncated = good[3][:len(good[3]) // 2]
    bad = [truncated, bad_code_file(), cmyk_file(64, 48), file_411(), None]
    files = [good[0], bad[0], good[1], bad[1], good[2], prog, bad[2], good[3], bad[3], good[4], bad[4], good[5]]
    want = [(alone(ctx, f)) for f in files]                 # without the switches
    assert [s for _, s in want] == [0, want[1][1], 0, INVALID, 0, 0, UNSUPPORTED, 0, UNSUPPORTED, 0, INVALID, 0] and want[1][1] != 0
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    before = ctx.jpeg_decode_counts()
    frames, st = ctx.jpeg_decode_mixed(files)
    after = ctx.jpeg_decode_counts()
    assert st == [s for _, s in want]
    assert after[2] == before[2] and after[1] - before[1] == 1        # the progressive file: the host route whatever the switch says
    for i, (ref, ref_st) in enumerate(want):
        if ref_st == 0:
            same_planes(frames[i], ref, "file %d" % i)
        else:
            assert frames[i] is None
    # the raw structs of the non-OK files are all zero
    import ctypes as C
    import imageprocessor_amd as m
    from imageprocessor_amd import _lib
    n = len(files)
    arr = m._bytes_array([f or b"" for f in files])
    arr[10].data = None
    fr = (_lib.JpegFrame * n)()
    C.memset(fr, 0xff, C.sizeof(fr))
    status, owner = (C.c_int * n)(), C.c_void_p()
    assert m.lib().ipx_jpeg_decode_mixed(ctx.handle, None, arr, n, fr, status, C.byref(owner)) == 0
    assert list(status) == st
    for i in range(n):
        if status[i] != 0:
            assert bytes(fr[i]) == bytes(C.sizeof(_lib.JpegFrame)), i
    m.lib().ipx_jpeg_planes_free(ctx.handle, owner)


@pytest.mark.gpu
@pytest.mark.parametrize("shared", ["0", "1"])
def test_tables_differ_between_sizes(ctx, monkeypatch, shared):
    """Files of different sizes, qualities and Huffman tables (Pillow's optimised ones among the Annex K defaults) in one call: the
    piece kernels group by table set; with IPX_JPEG_PIECE=0 the byte-wise kernel takes per-lane tables, or -- IPX_JPEG_SHARED_TABLES --
    one shared set when the call's files agree."""
    mixed_tables = [make(w, h, "420", seed=w, quality=q, optimize=opt) for (w, h), q, opt in
                    (((33, 15), 85, False), ((200, 120), 60, True), ((64, 48), 95, True), ((129, 65), 30, False), ((257, 40), 85, True))]
    same_tables = [make(w, h, "420", seed=w, quality=q) for (w, h), q in (((33, 15), 85), ((200, 120), 60), ((9, 7), 95))]
    monkeypatch.setenv("IPX_JPEG_SHARED_TABLES", shared)
    for piece in ("1", "0"):
        monkeypatch.setenv("IPX_JPEG_PIECE", piece)
        for files in (mixed_tables, same_tables):
            frames, st = check_mixed(ctx, files, against_alone=False)
            assert st == [0] * len(files)


@pytest.mark.gpu
def test_no_files_and_too_many(ctx):
    import ctypes as C
    import imageprocessor_amd as m
    assert ctx.jpeg_decode_mixed([]) == ([], [])
    owner = C.c_void_p(1)
    n = 65536
    assert m.lib().ipx_jpeg_decode_mixed(ctx.handle, None, (m._lib.Bytes * n)(), n, (m._lib.JpegFrame * n)(), (C.c_int * n)(), C.byref(owner)) == UNSUPPORTED
    assert not owner.value


# ---- the leg ---------------------------------------------------------------------------------------------------------------------

LEG_SIZES = [(33, 15), (64, 48), (48, 64), (129, 65), (17, 17), (200, 120)]
OUTS = ("resize", "thumbnail", "watermark")
QUALITY = 85
LEG_ENVS = ("IPX_JPEG_MIXED_GROUP", "IPX_JPEG_MIXED_CHUNK_MB", "IPX_JPEG_JPEG_CHUNK", "IPX_JPEG_JPEG_PART")


def leg_glyphs():
    from helpers import text_glyphs
    return text_glyphs(64, 48, n=3, width_px=30, height_px=10, margin=4)


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


def ops_of(keep_aspect, watermark=True, resize=None):
    return {"resize": resize or (64, 48, keep_aspect), "thumbnail": (32, True), "watermark": watermark}


def uniform_leg(ctx, files, sizes, keep_aspect, glyphset=None, texts=None, resize=None):
    """ipx_plan_run_jpeg_jpeg (or its _texts twin) per size and class -- a uniform call is one sampling -- with a plan of that size
    -> ({operator: [bytes | None]}, statuses); sizes[i] = (w, h, class)"""
    n = len(files)
    want, status = {k: [None] * n for k in OUTS}, [None] * n
    for w, h, cls in sorted(set(sizes)):
        idx = [i for i in range(n) if sizes[i] == (w, h, cls)]
        plan = ctx.plan(w, h, resize=resize or (64, 48, keep_aspect), thumbnail=(32, True), watermark=glyphset if glyphset is not None else True)
        try:
            out, st = plan.run_jpeg_jpeg([files[i] for i in idx], quality=QUALITY, texts=None if texts is None else [texts[i] for i in idx])
        finally:
            plan.close()
        for j, i in enumerate(idx):
            status[i] = st[j]
            for k in OUTS:
                want[k][i] = out.get(k, [None] * len(idx))[j]
    return want, status


@pytest.fixture(scope="module")
def leg_case(ctx):
    """24 files of six sizes and two classes, interleaved, and what the uniform leg makes of every size group with a plan of that
    size and the shared glyph set: computed once, for both resize rules"""
    import imageprocessor_amd as ipx
    from helpers import DEFAULT_COL
    files, sizes = [], []
    for i in range(24):
        w, h = LEG_SIZES[i % 6]
        cls = ("420", "444")[(i // 6) % 2]
        files.append(make(w, h, cls, seed=700 + i, **({"restart_marker_blocks": 3} if i % 5 == 0 else {})))
        sizes.append((w, h, cls))
    gs = ctx.glyphset(leg_glyphs(), DEFAULT_COL)
    try:
        want = {ka: uniform_leg(ctx, files, sizes, ka, glyphset=gs) for ka in (False, True)}
    finally:
        gs.close()
    texts = [leg_text(ipx, i, *sizes[i][:2]) for i in range(24)]
    return files, sizes, want, texts


def clear_env(monkeypatch):
    for k in LEG_ENVS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("keep_aspect", [False, True], ids=["encode-per-chunk", "encode-per-run"])
def test_leg_streams_are_the_uniform_legs(ctx, leg_case, monkeypatch, keep_aspect):
    """keep_aspect = 0: the resize output and the cropped thumbnail have one size for every file, and are encoded once per chunk;
    keep_aspect = 1: the resize output follows the file's shape and is encoded per run.  The watermark always is.  Six of the files
    also against the oracle's decoder, operators and encoder."""
    from helpers import DEFAULT_COL
    from test_sources_gpu import _expect_ycbcr_ops
    files, sizes, want, texts = leg_case
    clear_env(monkeypatch)
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(keep_aspect, (leg_glyphs(), DEFAULT_COL)), files, quality=QUALITY)
    assert st == want[keep_aspect][1] == [0] * 24
    for k in OUTS:
        for i in range(24):
            assert got[k][i] is not None and got[k][i] == want[keep_aspect][0][k][i], (k, i, sizes[i])
    for i in (0, 3, 5, 8, 13, 22):
        (w, h), d = sizes[i][:2], oracle.jpeg_decode(files[i])
        ch, cw = ((h + 1) // 2, (w + 1) // 2) if d["ratio"] == 2 else (h, w)
        ref = _expect_ycbcr_ops(np.ascontiguousarray(d["y"][:h, :w]), np.ascontiguousarray(d["cb"][:ch, :cw]), np.ascontiguousarray(d["cr"][:ch, :cw]),
                                d["ratio"], (64, 48, keep_aspect), (32, True), leg_glyphs(), DEFAULT_COL)
        for k in OUTS:
            assert got[k][i] == oracle.jpeg_encode_rgba(ref[k], QUALITY), (k, i, sizes[i])


@pytest.mark.gpu
def test_leg_texts_outputs_and_statuses(ctx, leg_case, monkeypatch):
    import ctypes as C
    import imageprocessor_amd as ipx
    files, sizes, want, texts = leg_case
    clear_env(monkeypatch)
    # a text per file, against ipx_plan_run_jpeg_jpeg_texts per size
    texted, st_t = uniform_leg(ctx, files[:12], sizes[:12], True, texts=texts[:12])
    plain, st_p = uniform_leg(ctx, files[:12], sizes[:12], True)
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(True), files[:12], quality=QUALITY, texts=texts[:12])
    assert st == st_t == [0] * 12 and got == texted and texted["watermark"] != plain["watermark"] and texted["resize"] == plain["resize"]
    # a NULL output array; an operator not asked for; no files
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(True), files[:12], quality=QUALITY, want=("thumbnail",))
    assert st == [0] * 12 and got == {"thumbnail": plain["thumbnail"]}
    got, st = ctx.run_jpeg_jpeg_mixed({"resize": (64, 48, True)}, files[:12], quality=QUALITY, texts=texts[:12])
    assert st == [0] * 12 and got == {"resize": plain["resize"], "thumbnail": [None] * 12, "watermark": [None] * 12}
    assert ctx.run_jpeg_jpeg_mixed(ops_of(True), []) == ({k: [] for k in OUTS}, [])
    # one size no plan can be made for -- 600 x 1 kept in aspect inside 70000 x 120 is 69960 pixels wide, beyond the span the kernels
    # address -- among sizes that have one: that file carries ipx_plan_create's status, alone
    wide, tall = (70000, 120, True), make(600, 1, "420", seed=3)
    with pytest.raises(ipx.IpxError) as e:
        ctx.plan(600, 1, resize=wide, thumbnail=(32, True), watermark=True)
    assert e.value.status == UNSUPPORTED
    ref, ref_st = uniform_leg(ctx, files[:4], sizes[:4], True, resize=wide)
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(True, resize=wide), files[:2] + [tall] + files[2:4], quality=QUALITY)
    assert st == [0, 0, UNSUPPORTED, 0, 0] and ref_st == [0] * 4
    for k in OUTS:
        assert got[k][2] is None and got[k][:2] + got[k][3:] == ref[k], k
    # no size has a plan: every file carries that status, a broken file its own, and the call is IPX_OK
    with pytest.raises(ipx.IpxError) as e:
        ctx.plan(64, 48, resize=(70000, 10, False), thumbnail=(32, True), watermark=True)
    assert e.value.status == UNSUPPORTED
    got, st = ctx.run_jpeg_jpeg_mixed({"resize": (70000, 10, False), "thumbnail": (32, True), "watermark": True}, files[:6] + [b"junk"])
    assert st == [UNSUPPORTED] * 6 + [INVALID] and all(v == [None] * 7 for v in got.values())
    # a broken file in the middle, and one the decoder gives up on only in its scan: the others are unaffected
    cut = files[3][:len(files[3]) // 2]
    batch = files[:5] + [b"\xff\xd8 not a jpeg"] + files[5:9] + [cut, bad_code_file()] + files[9:12]
    got, st = ctx.run_jpeg_jpeg_mixed(ops_of(True), batch, quality=QUALITY)
    bad = (5, 10, 11)
    keep = [i for i in range(15) if i not in bad]
    assert [st[i] for i in bad] == [INVALID, alone(ctx, cut)[1], INVALID] and st[10] != 0 and [st[i] for i in keep] == [0] * 12
    for k in OUTS:
        assert [got[k][i] for i in bad] == [None] * 3 and [got[k][i] for i in keep] == plain[k], k
    # texts and a glyph list of the call's own exclude each other
    from helpers import DEFAULT_COL
    with pytest.raises(ipx.IpxError) as e:
        ctx.run_jpeg_jpeg_mixed(ops_of(True, (leg_glyphs(), DEFAULT_COL)), files[:2], texts=texts[:2])
    assert e.value.status == INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"IPX_JPEG_MIXED_GROUP": "2"}, {"IPX_JPEG_MIXED_CHUNK_MB": "0"}, {"IPX_JPEG_MIXED_GROUP": "5", "IPX_JPEG_MIXED_CHUNK_MB": "0"}],
                         ids=["groups-of-two", "chunk-per-file", "groups-of-five-chunk-per-file"])
def test_leg_small_budgets(ctx, leg_case, monkeypatch, env):
    """decode groups of two files and chunks of one: groups and chunks end inside the runs of one size and class (there are two
    files per size and class), and the streams are the same"""
    from helpers import DEFAULT_COL
    files, sizes, want, texts = leg_case
    clear_env(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for keep_aspect in (False, True):
        got, st = ctx.run_jpeg_jpeg_mixed(ops_of(keep_aspect, (leg_glyphs(), DEFAULT_COL)), files, quality=QUALITY)
        assert st == [0] * 24 and got == want[keep_aspect][0]
