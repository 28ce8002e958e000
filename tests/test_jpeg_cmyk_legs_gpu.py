"""Four-component JPEGs through the compressed-in / compressed-out leg (ipx_plan_run_jpeg_jpeg and _texts), the pool's JPEG job and
the micro-batcher, under IPX_JPEG_CMYK=1.

A four-component file's three streams equal a chain that does not go through the leg: tests/jpeg_cmyk_model.py -> the oracle's
operators on an *image.CMYK frame (tests/test_deep_gpu.py's route) -> oracle.jpeg_encode_rgba.  The three-component files of the same
call get what the call returns without the four-component files.  Without the switch the four-component files are
IPX_ERR_UNSUPPORTED and nothing else changes.  Without the feature the four-component files are UNSUPPORTED under the switch too, so
every test here but the switch-off one fails."""
import io
import threading

import numpy as np
import pytest

import jpeg_cmyk_model as model
import jpeg_cmyk_writer as cw
import oracle
from helpers import DEFAULT_COL, rgba_frames, text_glyphs
from oracle import DEEP_CMYK
from test_deep_gpu import _expect
from test_texts_gpu import file_texts

pytestmark = pytest.mark.gpu
PIL = pytest.importorskip("PIL.Image")

W, H = 48, 40
RESIZE, THUMB, QUALITY = (24, 20, False), (16, True), 85
OK, UNSUPPORTED = 0, -4
KEYS = ("resize", "thumbnail", "watermark")


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
    monkeypatch.setenv("IPX_JPEG_CMYK", "1")


def _jpeg(a, **kw):
    buf = io.BytesIO()
    PIL.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def four(v, transform, seed, progressive=False, dri=0):
    """-> (file, the model's *image.CMYK pixels)"""
    f = cw.frame4(W, H, v)
    b = cw.blocks4(f, 900 + seed, amp=300, ac=60)
    return cw.cmyk_file(f, b, transform=transform, progressive=progressive, dri=dri), model.from_blocks(f, b, cw.quants(), transform, progressive)["pix"]


@pytest.fixture(scope="module")
def corpus():
    """eight interleaved files: -> (files, {index: CMYK pixels})"""
    three = [_jpeg(rgba_frames(1, W, H, seed=700 + i)[0][..., :3], quality=80 + i, subsampling=2) for i in range(3)]
    gray = _jpeg(rgba_frames(1, 32, 32, seed=710)[0][..., 0], quality=80)         # another size: handed back, as ever
    cmyk = {1: four(1, 0, 1), 3: four(2, 2, 2), 5: four(1, 0, 3, progressive=True), 6: four(2, 1, 4, dri=2)}
    files = [three[0], cmyk[1][0], gray, cmyk[3][0], three[1], cmyk[5][0], cmyk[6][0], three[2]]
    return files, {i: c[1] for i, c in cmyk.items()}


GLYPHS = text_glyphs(W, H, n=4, width_px=30, height_px=12)


# the default (one part, one chunk), and the cut at its smallest: "the rest" of the corpus as two parts of two files, every part and
# every four-component sub-batch in one-file chunks (both variables are read on every call)
CUTS = [pytest.param({}, id="default"), pytest.param({"IPX_JPEG_JPEG_PART": "2", "IPX_JPEG_JPEG_CHUNK": "1"}, id="part2-chunk1")]


@pytest.fixture(params=CUTS)
def cut(request, monkeypatch):
    for k, v in request.param.items():
        monkeypatch.setenv(k, v)


def cmyk_chain(pix, glyphs, col):
    """model pixels -> the three streams"""
    frames = _expect(oracle.deep_pix(pix, DEEP_CMYK), DEEP_CMYK, W, H, RESIZE, THUMB, glyphs, col)
    return {k: oracle.jpeg_encode_rgba(f, QUALITY) for k, f in zip(KEYS, frames)}


def test_leg(ctx, on, cut, corpus):
    files, pixels = corpus
    gs = ctx.glyphset(GLYPHS, DEFAULT_COL)
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    before = ctx.jpeg_cmyk_files()
    got, st = plan.run_jpeg_jpeg(files, QUALITY)
    assert st == [OK, OK, UNSUPPORTED, OK, OK, OK, OK, OK]
    assert ctx.jpeg_cmyk_files() - before == len(pixels)
    for i, pix in pixels.items():
        want = cmyk_chain(pix, GLYPHS, DEFAULT_COL)
        for k in KEYS:
            assert got[k][i] == want[k], "file %d %s" % (i, k)
    rest = [i for i in range(len(files)) if i not in pixels]
    alone, st2 = plan.run_jpeg_jpeg([files[i] for i in rest], QUALITY)
    assert st2 == [st[i] for i in rest]
    for j, i in enumerate(rest):
        for k in KEYS:
            assert got[k][i] == alone[k][j], "file %d %s" % (i, k)
    assert all(got[k][2] is None for k in KEYS)
    # four-component files only, of both vectors: nothing is left for the three-component path
    only = sorted(pixels)
    got2, st3 = plan.run_jpeg_jpeg([files[i] for i in only], QUALITY)
    assert st3 == [OK] * len(only)
    for j, i in enumerate(only):
        assert {k: got2[k][j] for k in KEYS} == {k: got[k][i] for k in KEYS}
    plan.close()
    gs.close()


def test_leg_texts(ctx, on, cut, corpus):
    files, pixels = corpus
    texts = file_texts(len(files), W, H, 53)
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=THUMB, watermark=True)
    got, st = plan.run_jpeg_jpeg(files, QUALITY, texts=texts)
    assert st == [OK, OK, UNSUPPORTED, OK, OK, OK, OK, OK]
    assert len(texts[3][0]) != len(texts[5][0]) and texts[3][1] != texts[5][1]
    for i, pix in pixels.items():                       # every four-component file carries its own text (two would do)
        want = cmyk_chain(pix, texts[i][0], texts[i][1])
        for k in KEYS:
            assert got[k][i] == want[k], "file %d %s" % (i, k)
    rest = [i for i in range(len(files)) if i not in pixels]
    alone, _ = plan.run_jpeg_jpeg([files[i] for i in rest], QUALITY, texts=[texts[i] for i in rest])
    for j, i in enumerate(rest):
        for k in KEYS:
            assert got[k][i] == alone[k][j], "file %d %s" % (i, k)
    plan.close()


@pytest.mark.parametrize("value", [None, "0"])
def test_leg_switch_off(ctx, corpus, monkeypatch, value):
    monkeypatch.delenv("IPX_JPEG_CMYK", raising=False) if value is None else monkeypatch.setenv("IPX_JPEG_CMYK", value)
    files, pixels = corpus
    gs = ctx.glyphset(GLYPHS, DEFAULT_COL)
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    cmyk, counts = ctx.jpeg_cmyk_files(), ctx.jpeg_decode_counts()
    got, st = plan.run_jpeg_jpeg(files, QUALITY)
    assert st == [UNSUPPORTED if i in pixels or i == 2 else OK for i in range(len(files))]
    assert ctx.jpeg_cmyk_files() == cmyk
    assert [a - b for a, b in zip(ctx.jpeg_decode_counts(), counts)] == [3, 0, 0, 0]      # Pillow's three baseline files, nothing else
    rest = [i for i in range(len(files)) if i not in pixels]
    alone, _ = plan.run_jpeg_jpeg([files[i] for i in rest], QUALITY)
    for j, i in enumerate(rest):
        for k in KEYS:
            assert got[k][i] == alone[k][j]
    for i in pixels:
        assert all(got[k][i] is None for k in KEYS)
    plan.close()
    gs.close()


def test_pool_job_and_micro_batcher(ipx, ctx, on):
    """40 single files, half of them four-component, from 4 threads.  Both halves have the luma sampling 2 x 2, so only the component
    count keeps them apart in the batcher's grouping key: with max_batch above either half's 20 files no group can fill up unless the
    two kinds share one."""
    cm = [four(2, (2, 0, 1, 2)[i], 20 + i, progressive=i == 3) for i in range(4)]
    three = [_jpeg(rgba_frames(1, W, H, seed=800 + i)[0][..., :3], quality=78 + i, subsampling=2) for i in range(4)]
    files = [(cm[i % 4][0] if i & 1 else three[i % 4]) for i in range(40)]
    gs = ctx.glyphset(GLYPHS, DEFAULT_COL)
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    want, st = plan.run_jpeg_jpeg(files, QUALITY)
    plan.close()
    gs.close()
    assert st == [OK] * 40
    ops = dict(resize=RESIZE, thumbnail=THUMB, glyphs=GLYPHS, col=DEFAULT_COL)
    got, errs = {}, []
    with ipx.Pool(devices=(0,)) as pool:
        out, pst = pool.submit_files(files, W, H, "jpeg", QUALITY, **ops).wait()
        assert pst == [OK] * 40 and out == want
        with ipx.Batcher(pool, max_batch=32, max_wait_us=3000, quality=QUALITY) as b:
            def work(part):
                try:
                    tickets = [(i, b.submit(files[i], W, H, **ops)) for i in part]
                    for i, t in tickets:
                        got[i] = b.wait(t)
                except Exception as e:  # noqa: BLE001
                    errs.append(repr(e)[:300])
            ts = [threading.Thread(target=work, args=(range(k, 40, 4),)) for k in range(4)]
            [t.start() for t in ts]
            [t.join() for t in ts]
            stats = b.stats()
    assert not errs, errs
    assert stats["files"] == 40 and stats["batches"] >= 2
    assert stats["flushed_by_size"] == 0 and stats["largest_batch"] <= 20, stats
    for i in range(40):
        assert got[i][0] == OK, i
        assert got[i][1] == {k: want[k][i] for k in KEYS}, "file %d" % i
