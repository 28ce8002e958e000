"""Adam7-interlaced PNG files on the GPU under IPX_PNG_ADAM7=1 (csrc/ipx_png_dec.hip: the host parse's raw length and
png_unfilter_kernel<true>, a wave per file and pass): ipx_png_decode_batch on the hand-derived known answers of
tests/golden/png_adam7_kats.json and byte for byte against tests/png_adam7_model.py, interlaced files against their non-interlaced twins
in the same call, and the routes above the decoder (ipx_plan_run_png_png, IPX_JOB_PNG through the pool, the micro-batcher).  With the
variable unset an interlaced file stays IPX_ERR_UNSUPPORTED.  PARITY UNPINNED against Go itself."""
import json
import os
import zlib

import numpy as np
import pytest

import png_adam7_corpus as ac
import png_adam7_model as am
import png_corpus as pc
import png_decode_model as dm
from helpers import DEFAULT_COL, text_glyphs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "png_adam7_kats.json")) as f:
    KATS = json.load(f)


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("IPX_PNG_ADAM7", "1")


def _check_batch(ctx, files, w=0, h=0, kind=-1, fast=False, res=None):
    """one call; every status, and every frame and palette byte of the OK files, as the model says (res: the model's answers, when
    the caller has them)"""
    info, st = ctx.png_decode_batch(files, w, h, kind)
    res = res or [am.decode(f, fast=fast) for f in files]
    size = (w, h) if w else next(((r["w"], r["h"]) for r in res if r["stage"] == "data"), None)
    k = kind if kind >= 0 else next((r["kind"] for r in res if r["stage"] == "data" and (r["w"], r["h"]) == size), None)
    want = [am.entry_status(r, size, k) for r in res]
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


def _plan(ctx, sw, sh):
    gs = ctx.glyphset(text_glyphs(sw, sh), DEFAULT_COL)
    return gs, ctx.plan(sw, sh, resize=(160, 120, True), thumbnail=(50, True), watermark=gs)


def _bad_idat_crc(data):
    i = data.index(b"IDAT")
    n = int.from_bytes(data[i - 4:i], "big")
    b = bytearray(data)
    b[i + 4 + n] ^= 0x40
    return bytes(b)


@pytest.mark.parametrize("value", [None, "0", "2"])
def test_off_by_default(ctx, monkeypatch, value):
    """unset, 0 or anything but 1: an interlaced file is UNSUPPORTED from both entries, its neighbour decodes"""
    if value is None:
        monkeypatch.delenv("IPX_PNG_ADAM7", raising=False)
    else:
        monkeypatch.setenv("IPX_PNG_ADAM7", value)
    il = ac.of_type(2, 8, False, 30, 40, seed=1)
    twin = ac.of_type(2, 8, False, 30, 40, seed=1, interlace=False)
    info, st = ctx.png_decode_batch([il, twin, il])
    assert st == [dm.UNSUPPORTED, dm.OK, dm.UNSUPPORTED]
    np.testing.assert_array_equal(info["pix"][1], dm.decode(twin)["pix"])
    assert ctx.png_decode_batch([il])[1] == [dm.UNSUPPORTED]
    gs, plan = _plan(ctx, 40, 30)
    try:
        out, st = plan.run_png_png([il, twin])
        assert st == [dm.UNSUPPORTED, dm.OK]
        assert all(out[k][0] is None and out[k][1] is not None for k in out)
    finally:
        plan.close()
        gs.close()


@pytest.mark.parametrize("k", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(ctx, monkeypatch, k):
    data = bytes.fromhex(k["data"])
    monkeypatch.delenv("IPX_PNG_ADAM7", raising=False)
    info, st = ctx.png_decode_batch([data])
    assert info is None and st == [k["status_off"]]
    monkeypatch.setenv("IPX_PNG_ADAM7", "1")
    assert _check_batch(ctx, [data]) == [k["status"]]
    info, st = ctx.png_decode_batch([data])
    assert st == [k["status"]]
    if k["status"] != dm.OK:
        assert info is None
        return
    assert (info["w"], info["h"], info["kind"]) == (k["w"], k["h"], k["kind"])
    assert info["pix"][0].tobytes().hex() == k["pix"], k["name"]
    if "palette" in k:
        assert info["palettes"][0].tobytes().hex() == k["palette"], k["name"]


@pytest.mark.parametrize("ctype,depth", [(0, 8), (6, 8), (0, 1)], ids=["gray8", "rgba8", "gray1"])
def test_every_small_size(ctx, on, ctype, depth):
    """every (w, h) in 1 .. 9 x 1 .. 9: every combination of empty passes; mixed filters"""
    empties = set()
    for h in range(1, 10):
        for w in range(1, 10):
            f = ac.of_type(ctype, depth, False, h, w, seed=10 * h + w, filters=(4, 2, 3, 1, 0), split=(None, 5)[(w + h) % 2])
            assert _check_batch(ctx, [f]) == [dm.OK], (w, h)
            empties.add(tuple(not (pw and ph) for pw, ph in ac.pass_sizes(w, h)))
    assert len(empties) >= 9 and (False,) * 7 in empties and (False,) + (True,) * 6 in empties


@pytest.mark.parametrize("name,ctype,depth,trns", pc.TYPES, ids=[t[0] for t in pc.TYPES])
def test_every_type_every_filter(ctx, on, name, ctype, depth, trns):
    """each row of the type table at the sizes and filter sets of test_png_decode_gpu.py's test of that name, interlaced"""
    for k, (w, h) in enumerate([(1, 1), (1, 9), (9, 1), (13, 7), (37, 29), (70, 67)]):
        for fl in ((0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)):
            f = ac.of_type(ctype, depth, trns, h, w, seed=100 * k + len(fl), kind=("photo", "flat")[k % 2], filters=fl)
            assert _check_batch(ctx, [f], fast=True) == [dm.OK], (w, h, fl)


@pytest.mark.parametrize("ctype,depth", [(2, 8), (0, 1), (6, 16)], ids=["rgb8", "gray1", "rgba16"])
def test_band_edges(ctx, on, ctype, depth):
    """some pass has 63, 64, 65, 128 or 129 rows (pass 7 has h / 2, pass 6 (h + 1) / 2, passes 4 and 5 about h / 4, 1 to 3 about h / 8):
    the hand-off between bands of 64 rows inside a pass, with Up, Average and Paeth rows across it"""
    seen = set()
    for h in (126, 127, 128, 129, 130, 256, 257, 258, 504, 512, 513, 520):
        for w in (3, 11):
            seen.update(ph for pw, ph in ac.pass_sizes(w, h) if pw)
            f = ac.of_type(ctype, depth, False, h, w, seed=h + w, filters=(4, 2, 3, 1, 0) if w == 3 else (4,))
            assert _check_batch(ctx, [f], fast=True) == [dm.OK], (w, h)
    assert {63, 64, 65, 128, 129} <= seen


@pytest.mark.parametrize("ctype", [0, 3], ids=["gray", "palette"])
def test_sub_byte_pass_widths(ctx, on, ctype):
    """widths 1 .. 17 at depths 1, 2 and 4, height 9: the last byte of a pass row holds 1 .. 8 / depth pixels"""
    for depth in (1, 2, 4):
        for w in range(1, 18):
            f = ac.of_type(ctype, depth, False, 9, w, seed=20 * depth + w, filters=(0, 1, 2, 3, 4))
            assert _check_batch(ctx, [f]) == [dm.OK], (depth, w)


def test_mixed_batch_against_twins(ctx, on):
    """one size and kind, interlaced files and their non-interlaced twins interleaved, with a truncated interlaced file, one with a bad
    IDAT CRC and one of another kind among them: each interlaced file's frame is its twin's frame from the same call"""
    w, h = 53, 41
    files, pairs = [], []
    for k in range(12):
        kw = dict(seed=40 + k, kind=("photo", "flat")[k % 2], filters=((0, 1, 2, 3, 4), (k % 5,))[k % 2], split=(None, 61, "random")[k % 3])
        pairs.append((len(files), len(files) + 1))
        files += [ac.of_type(6, 8, False, h, w, **kw), ac.of_type(6, 8, False, h, w, interlace=False, **kw)]
    il = files[0]
    broken = {5: il[:-25], 12: _bad_idat_crc(il), 19: ac.of_type(0, 8, False, h, w, seed=3)}
    for at in sorted(broken):
        files.insert(at, broken[at])
        pairs = [(a + (a >= at), b + (b >= at)) for a, b in pairs]
    info, st = ctx.png_decode_batch(files)
    res = [am.decode(f, fast=i not in broken) for i, f in enumerate(files)]
    assert st == [am.entry_status(r, (w, h), dm.NRGBA) for r in res]
    assert [i for i, s in enumerate(st) if s != dm.OK] == sorted(broken)
    assert (st[5], st[12], st[19]) == (dm.INVALID, dm.INVALID, dm.UNSUPPORTED)
    for a, b in pairs:
        assert files[a][28] == 1 and files[b][28] == 0
        assert np.array_equal(info["pix"][a], info["pix"][b]), (a, b)
        assert np.array_equal(info["pix"][b], dm.decode(files[b], fast=True)["pix"]), b     # the neighbours are intact


def test_truncation_and_raw_length(ctx, on):
    """a small interlaced RGB 8 file cut at every offset; its raw stream one byte short and long; filter type 5 in the first and the last
    row of each pass; a byte after the Adler-32"""
    w, h = 7, 6
    s = pc.samples_of_type(2, 8, h, w, seed=1)
    good = ac.write(s, 2, 8, filters=(0, 1, 2, 3, 4), level=9)
    st = ctx.png_decode_batch([good] + [good[:i] for i in range(len(good))] + [good])[1]
    assert st[0] == st[-1] == dm.OK and all(v == dm.INVALID for v in st[1:-1])
    raw, starts = ac.raw_stream(s, 2, 8, (0, 1, 2, 3, 4))
    assert len(raw) == ac.raw_length(2, 8, w, h) and None not in starts
    files = [ac.wrap(w, h, 2, 8, zlib.compress(raw[:-1], 9)), ac.wrap(w, h, 2, 8, zlib.compress(raw + b"\x00", 9))]
    for (pw, ph), at in zip(ac.pass_sizes(w, h), starts):
        rb = 1 + 3 * pw
        for row in {0, ph - 1}:
            b = bytearray(raw)
            b[at + row * rb] = 5
            files.append(ac.wrap(w, h, 2, 8, zlib.compress(bytes(b), 9)))
    nbad = len(files)
    files.append(ac.wrap(w, h, 2, 8, zlib.compress(raw, 9) + b"\x00"))
    st = _check_batch(ctx, [good] + files + [good])
    assert st == [dm.OK] + [dm.INVALID] * nbad + [dm.UNSUPPORTED, dm.OK]


@pytest.mark.parametrize("w,h,ctype,depth", [(1920, 1080, 2, 8), (1024, 768, 6, 16), (8200, 3, 6, 8), (333, 517, 3, 4)])
def test_large_frames(ctx, on, w, h, ctype, depth):
    """1920x1080, 16-bit, rows longer than the inflater's window with pass 3 empty and pass 5 of one row (8200 x 3), a sub-byte palette; the pixels
    expected are the source samples converted, so no Python unfilter runs at this size"""
    if h == 3:
        assert [ph for pw, ph in ac.pass_sizes(w, h)] == [1, 1, 0, 1, 1, 2, 1]
    files, want = [], []
    for seed, (kd, fl, sp) in enumerate([("photo", (0, 1, 2, 3, 4), None), ("flat", (4,), 8192)]):
        files.append(ac.of_type(ctype, depth, False, h, w, seed=seed, kind=kd, filters=fl, split=sp))
        want.append(dm.convert(pc.pack_rows(pc.samples_of_type(ctype, depth, h, w, seed, kd), ctype, depth), ctype, depth, w, h, None))
    info, st = ctx.png_decode_batch(files)
    assert st == [dm.OK, dm.OK]
    assert (info["w"], info["h"], info["kind"]) == (w, h, dm.kind_of(ctype, depth, False))
    for i in range(2):
        assert np.array_equal(info["pix"][i], want[i]), i
        if ctype == 3:
            plain = files[i][:28] + b"\x00" + files[i][29:]              # (the model's chunk walk does not check CRCs)
            assert np.array_equal(info["palettes"][i], dm.palette(dm.parse(plain)[1]))


def test_scratch_groups(ctx, on, monkeypatch):
    """a 1 MiB scratch budget cuts the batch into many decode groups, interlaced and not in one group: the answers of one group"""
    files = [ac.of_type(6, 8, False, 120, 160, seed=300 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,), interlace=k % 3 == 0)
             for k in range(24)]
    files[6] = files[6][:-30]
    files[7] = files[7][:-30]
    one, st1 = ctx.png_decode_batch(files)
    monkeypatch.setenv("IPX_PNG_DEC_SCRATCH_MB", "1")
    many, st2 = ctx.png_decode_batch(files)
    assert st1 == st2 == [dm.INVALID if k in (6, 7) else dm.OK for k in range(24)]
    for k in range(24):
        if st1[k] == dm.OK:
            twin = ac.of_type(6, 8, False, 120, 160, seed=300 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,), interlace=False)
            want = dm.decode(twin, fast=True)["pix"]
            assert np.array_equal(one["pix"][k], want) and np.array_equal(many["pix"][k], want), k


def _leg_files(sw, sh):
    """interlaced files of every row of the type table, each followed by a non-interlaced neighbour of another seed, then broken
    interlaced files; -> (files, their twins: the same list with every interlaced file non-interlaced, indices interlaced)"""
    files, twins, il = [], [], []
    for k, (name, ctype, depth, trns) in enumerate(pc.TYPES):
        kw = dict(seed=900 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,))
        il.append(len(files))
        files.append(ac.of_type(ctype, depth, trns, sh, sw, **kw))
        twins.append(ac.of_type(ctype, depth, trns, sh, sw, interlace=False, **kw))
        if k % 3 == 0:
            n = pc.of_type(ctype, depth, trns, sh, sw, seed=500 + k)
            files.append(n)
            twins.append(n)
    good = files[il[8]]
    for b in (good[:-20], _bad_idat_crc(good), ac.of_type(2, 8, False, sh + 1, sw, seed=1)):
        il.append(len(files))
        files.append(b)
        twins.append(b)
    return files, twins, il


def test_leg(ctx, monkeypatch):
    """ipx_plan_run_png_png on interlaced files of every kind, broken ones among them: the statuses of the model, the three streams
    of the non-interlaced twins, None exactly where the status is not OK; with the variable unset, UNSUPPORTED for exactly the
    interlaced files and the same streams for their neighbours"""
    sw, sh = 40, 30
    gs, plan = _plan(ctx, sw, sh)
    files, twins, il = _leg_files(sw, sh)
    try:
        monkeypatch.setenv("IPX_PNG_ADAM7", "1")
        out, st = plan.run_png_png(files)
        assert st == [am.entry_status(am.decode(f), (sw, sh)) for f in files]
        assert st[-3:] == [dm.INVALID, dm.INVALID, dm.UNSUPPORTED] and st[:-3] == [dm.OK] * (len(files) - 3)
        tout, tst = plan.run_png_png(twins)
        assert tst == st
        for k in ("resize", "thumbnail", "watermark"):
            for i, s in enumerate(st):
                assert (out[k][i] is None) == (s != dm.OK)
                assert out[k][i] == tout[k][i], (k, i)
        monkeypatch.delenv("IPX_PNG_ADAM7")
        off, ost = plan.run_png_png(files)
        assert ost == [dm.UNSUPPORTED if i in il else dm.OK for i in range(len(files))]
        for k in off:
            for i in range(len(files)):
                assert off[k][i] == (None if i in il else out[k][i]), (k, i)
    finally:
        plan.close()
        gs.close()


def test_pool_and_batcher(ctx, monkeypatch):
    """IPX_JOB_PNG through the pool, a job of several chunks with interlaced files among them: the leg's statuses and streams; through
    the micro-batcher an interlaced file and its twin come back with the same three streams"""
    import imageprocessor_amd as ipx
    sw, sh = 40, 30
    monkeypatch.setenv("IPX_PNG_ADAM7", "1")
    monkeypatch.setenv("IPX_POOL_PNG_CHUNK", "8")
    files, twins, il = _leg_files(sw, sh)
    glyphs = text_glyphs(sw, sh)
    ops = dict(resize=(160, 120, True), thumbnail=(50, True), glyphs=glyphs, col=DEFAULT_COL)
    gs, plan = _plan(ctx, sw, sh)
    try:
        want, want_st = plan.run_png_png(files)
    finally:
        plan.close()
        gs.close()
    assert want_st.count(dm.OK) == len(files) - 3
    with ipx.Pool(devices=(0,)) as pool:
        got, st = pool.submit_files(files, sw, sh, "png", **ops).wait()
        assert st == want_st
        for k in ("resize", "thumbnail", "watermark"):
            assert got[k] == want[k], k
        with ipx.Batcher(pool, max_batch=8, max_wait_us=2000) as b:
            ta, tb = b.submit(files[il[8]], sw, sh, **ops), b.submit(twins[il[8]], sw, sh, **ops)
            (sa, oa), (sb, ob) = b.wait(ta), b.wait(tb)
        assert sa == sb == dm.OK and oa == ob and all(v is not None and v.startswith(dm.SIG) for v in oa.values())
        assert oa == {k: want[k][il[8]] for k in oa}
