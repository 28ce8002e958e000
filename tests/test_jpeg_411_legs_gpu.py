"""4:1:1 / 4:1:0 JPEGs through the compressed-in / compressed-out leg (ipx_plan_run_jpeg_jpeg), the pool's JPEG job and the
micro-batcher, under IPX_JPEG_411=1.

The leg's streams equal the chain it is made of, run piece by piece on the same files: ipx_jpeg_decode_batch -> ipx_plan_run_dev_ycbcr
on the planes in HBM -> ipx_jpeg_encode_batch_dev; and, independently of the library, the model's planes through the oracle's operators
at 4:4:4 (chroma samples replicated: tests/test_ycbcr_411_gpu.py) and the oracle's encoder.  The batcher keeps a 4:1:1 and a 4:2:0 file
of one size in separate groups (the luma factors are in its key).  Without the switch the 4:1:x files are IPX_ERR_UNSUPPORTED, alone.
Without the feature they are UNSUPPORTED under the switch too: every test here but the switch-off one fails."""
import threading

import numpy as np
import pytest

import jpeg_411_corpus as c4
import jpeg_411_model as model
import oracle
from helpers import DEFAULT_COL, text_glyphs
from test_sources_gpu import _expect_ycbcr_ops

pytestmark = pytest.mark.gpu

W, H = 72, 40                     # 4:1:1: 3 x 5 MCUs, 4:1:0: 3 x 3; the chroma planes are 18 wide in rows of 24
RESIZE, THUMB, QUALITY = (36, 20, False), (16, True), 85
OK, UNSUPPORTED = 0, -4
KEYS = ("resize", "thumbnail", "watermark")
GLYPHS = text_glyphs(W, H, n=4, width_px=30, height_px=12)


@pytest.fixture(scope="module")
def ipx():
    import imageprocessor_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(ipx):
    with ipx.Context(device=0) as c:
        yield c


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("IPX_JPEG_411", "1")


def make(v0, seed, kind="baseline"):
    """-> (file, the model's planes)"""
    fr = c4.frame(W, H, v0)
    b = c4.blocks(fr, 4000 + seed)
    if kind == "progressive":
        return c4.progressive(fr, b), model.from_blocks(fr, b, c4.Q, progressive=True)
    data = c4.multiscan(fr, b) if kind == "multiscan" else c4.baseline(fr, b, ri=2 if kind == "restarts" else 0)
    return data, model.decode(data)


def batch(v0):
    return [make(v0, 10 * v0 + k, kind) for k, kind in enumerate(("baseline", "restarts", "progressive", "multiscan", "baseline"))]


def model_chain(planes, ratio):
    cw, ch = model.chroma_size(ratio, W, H)
    y = np.ascontiguousarray(planes["y"][:H, :W])
    cb, cr = (model.upsample(np.ascontiguousarray(planes[k][:ch, :cw]), ratio, W, H) for k in ("cb", "cr"))
    frames = _expect_ycbcr_ops(y, cb, cr, 0, RESIZE, THUMB, GLYPHS, DEFAULT_COL)
    return {k: oracle.jpeg_encode_rgba(frames[k], QUALITY) for k in KEYS}


@pytest.mark.parametrize("v0", [1, 2], ids=["411", "410"])
def test_leg_equals_its_chain(ctx, on, v0):
    cases = batch(v0)
    files = [c[0] for c in cases]
    n = len(files)
    ratio = model.RATIO_411 if v0 == 1 else model.RATIO_410
    gs = ctx.glyphset(GLYPHS, DEFAULT_COL)
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    got, st = plan.run_jpeg_jpeg(files, QUALITY)
    assert st == [OK] * n
    # the chain: decode, the plan on the planes where they lie, encode
    info, st = ctx.jpeg_decode_batch(files, download=False)
    assert st == [OK] * n and info["ratio"] == ratio
    b = info["batch"]
    i_ = plan.info
    res, th, wm = ctx.alloc(n * i_.resize_bytes), ctx.alloc(n * i_.thumb_bytes), ctx.alloc(n * i_.wm_bytes)
    plan.run_dev_ycbcr(n, b.y, b.cb, b.cr, b.ratio, b.ystride, b.cstride, b.y_frame_stride, b.c_frame_stride, res.ptr, th.ptr, wm.ptr)
    ctx.sync()
    chain = {"resize": ctx.jpeg_encode_batch_dev(res.ptr, i_.resize_w, i_.resize_h, n, QUALITY), "thumbnail": ctx.jpeg_encode_batch_dev(th.ptr, i_.thumb_w, i_.thumb_h, n, QUALITY),
             "watermark": ctx.jpeg_encode_batch_dev(wm.ptr, W, H, n, QUALITY)}
    info["free"]()
    for buf in (res, th, wm):
        buf.free()
    for i in range(n):
        for k in KEYS:
            assert got[k][i] == chain[k][i], "file %d %s: leg against chain" % (i, k)
        want = model_chain(cases[i][1], ratio)
        for k in KEYS:
            assert got[k][i] == want[k], "file %d %s: leg against model + oracle" % (i, k)
    plan.close()
    gs.close()


def mixed():
    """a 4:1:1, a 4:2:0 and a 4:1:0 file of one size, twice over"""
    f420 = c4.frame(W, H, 2, h0=2)
    return [make(1, 1)[0], c4.baseline(f420, c4.blocks(f420, 31)), make(2, 2)[0], make(1, 3, "progressive")[0], c4.baseline(f420, c4.blocks(f420, 32)), make(2, 4, "restarts")[0]]


def test_pool_job_and_micro_batcher(ipx, ctx, on, monkeypatch):
    monkeypatch.setenv("IPX_BATCHER_IDLE_FLUSH", "0")        # size and timer only: what a group holds does not depend on who ran first
    files = mixed()
    shape = [411, 420, 410, 411, 420, 410]
    gs = ctx.glyphset(GLYPHS, DEFAULT_COL)
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    want = {}
    for s in (411, 420, 410):                          # what each shape's files give as a batch of their own
        idx = [i for i in range(6) if shape[i] == s]
        out, st = plan.run_jpeg_jpeg([files[i] for i in idx], QUALITY)
        assert st == [OK, OK]
        for j, i in enumerate(idx):
            want[i] = {k: out[k][j] for k in KEYS}
    # one call over all six: the first file's shape is the batch's, the others are handed back
    out, st = plan.run_jpeg_jpeg(files, QUALITY)
    assert st == [OK if s == 411 else UNSUPPORTED for s in shape]
    assert all({k: out[k][i] for k in KEYS} == want[i] for i in (0, 3))
    plan.close()
    gs.close()
    ops = dict(resize=RESIZE, thumbnail=THUMB, glyphs=GLYPHS, col=DEFAULT_COL)
    got, errs = {}, []
    with ipx.Pool(devices=(0,)) as pool:
        idx = [0, 3]
        pout, pst = pool.submit_files([files[i] for i in idx], W, H, "jpeg", QUALITY, **ops).wait()      # one pool job of 4:1:1 files
        assert pst == [OK, OK]
        assert all({k: pout[k][j] for k in KEYS} == want[i] for j, i in enumerate(idx))
        # groups go out when they hold two files (nothing waits for the timer): were the key blind to the luma factors, groups would
        # fill with files of two shapes and one of each pair would come back UNSUPPORTED
        with ipx.Batcher(pool, max_batch=2, max_wait_us=5000000, quality=QUALITY) as b:
            def work(part):
                try:
                    tickets = [(i, b.submit(files[i], W, H, **ops)) for i in part]
                    for i, t in tickets:
                        got[i] = b.wait(t)
                except Exception as e:  # noqa: BLE001
                    errs.append(repr(e)[:300])
            ts = [threading.Thread(target=work, args=(range(k, 6, 2),)) for k in range(2)]
            [t.start() for t in ts]
            [t.join() for t in ts]
            stats = b.stats()
    assert not errs, errs
    # three shapes of one size and one operator set: three groups of two files, none of them handed back for its neighbours' shape
    assert stats["files"] == 6 and stats["batches"] == 3 and stats["largest_batch"] == 2 and stats["flushed_by_size"] == 3, stats
    for i in range(6):
        assert got[i][0] == OK, i
        assert got[i][1] == want[i], "file %d" % i


@pytest.mark.parametrize("value", [None, "0"])
def test_switch_off(ipx, ctx, monkeypatch, value):
    monkeypatch.delenv("IPX_JPEG_411", raising=False) if value is None else monkeypatch.setenv("IPX_JPEG_411", value)
    monkeypatch.setenv("IPX_BATCHER_IDLE_FLUSH", "0")
    files = mixed()
    gs = ctx.glyphset(GLYPHS, DEFAULT_COL)
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    counts = ctx.jpeg_decode_counts()
    out, st = plan.run_jpeg_jpeg(files, QUALITY)
    assert st == [UNSUPPORTED, OK, UNSUPPORTED, UNSUPPORTED, OK, UNSUPPORTED]
    assert [a - b for a, b in zip(ctx.jpeg_decode_counts(), counts)] == [2, 0, 0, 0]
    alone, st2 = plan.run_jpeg_jpeg([files[1], files[4]], QUALITY)
    assert st2 == [OK, OK]
    for j, i in enumerate((1, 4)):
        assert all(out[k][i] == alone[k][j] for k in KEYS)
    assert all(out[k][i] is None for k in KEYS for i in (0, 2, 3, 5))
    plan.close()
    gs.close()
    ops = dict(resize=RESIZE, thumbnail=THUMB, glyphs=GLYPHS, col=DEFAULT_COL)
    with ipx.Pool(devices=(0,)) as pool:
        with ipx.Batcher(pool, max_batch=2, max_wait_us=5000000, quality=QUALITY) as b:
            tickets = [b.submit(files[i], W, H, **ops) for i in (0, 1, 3, 4)]       # two groups of two, as with the switch
            got = [b.wait(t) for t in tickets]
            stats = b.stats()
    assert stats["batches"] == 2 and stats["flushed_by_size"] == 2, stats
    assert [g[0] for g in got] == [UNSUPPORTED, OK, UNSUPPORTED, OK]           # the 4:1:1 files are refused alone: the 4:2:0 files are served
    assert got[1][1] == {k: alone[k][0] for k in KEYS} and got[3][1] == {k: alone[k][1] for k in KEYS}
