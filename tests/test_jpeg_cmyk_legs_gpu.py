"""Four-component JPEGs through the compressed-in / compressed-out leg (ipx_plan_run_jpeg_jpeg and _texts), the pool's JPEG job and
the micro-batcher, under IPX_JPEG_CMYK=1.

A four-component file's three streams equal a chain that does not go through the leg: tests/jpeg_cmyk_model.py -> the oracle's
operators on an *image.CMYK frame (tests/test_deep_gpu.py's route) -> oracle.jpeg_encode_rgba.  The three-component files of the same
call get what the call returns without the four-component files.  Without the switch the four-component files are
IPX_ERR_UNSUPPORTED and nothing else changes.  Without the feature the four-component files are UNSUPPORTED under the switch too, so
every test here but the switch-off one fails.

The legs run at three sizes.  48 x 40: a frame of 7680 bytes, a multiple of 256, so the decoder's frame stride (align256 of the frame)
IS the frame.  52 x 38: 7904 bytes at a frame stride of 7936 -- a leg that handed the deep source rows * height for the frame stride
would read every frame but the first from the wrong place -- on the one-pass kernel.  50 x 38: 7600 bytes at 7680 and rows of
w % 4 = 2, which the one-pass kernel leaves to the per-output kernels behind the decode."""
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
SIZES = [(48, 40), (52, 38), (50, 38)]
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


def four(v, transform, seed, progressive=False, dri=0, size=(W, H)):
    """-> (file, the model's *image.CMYK pixels)"""
    f = cw.frame4(*size, v)
    b = cw.blocks4(f, 900 + seed, amp=300, ac=60)
    return cw.cmyk_file(f, b, transform=transform, progressive=progressive, dri=dri), model.from_blocks(f, b, cw.quants(), transform, progressive)["pix"]


_corpora = {}


def corpus_of(size):
    """eight interleaved files of one size: -> (files, {index: CMYK pixels}); made once per size and never changed"""
    if size not in _corpora:
        w, h = size
        three = [_jpeg(rgba_frames(1, w, h, seed=700 + i)[0][..., :3], quality=80 + i, subsampling=2) for i in range(3)]
        gray = _jpeg(rgba_frames(1, 32, 32, seed=710)[0][..., 0], quality=80)         # another size: handed back, as ever
        cmyk = {1: four(1, 0, 1, size=size), 3: four(2, 2, 2, size=size), 5: four(1, 0, 3, progressive=True, size=size),
                6: four(2, 1, 4, dri=2, size=size)}
        files = [three[0], cmyk[1][0], gray, cmyk[3][0], three[1], cmyk[5][0], cmyk[6][0], three[2]]
        _corpora[size] = (files, {i: c[1] for i, c in cmyk.items()})
    return _corpora[size]


@pytest.fixture(scope="module")
def corpus():
    return corpus_of((W, H))


def glyphs_of(size):
    return text_glyphs(*size, n=4, width_px=30, height_px=12)


GLYPHS = glyphs_of((W, H))


# the default (one part, one chunk), and the cut at its smallest: "the rest" of the corpus as two parts of two files, every part and
# every four-component sub-batch in one-file chunks (both variables are read on every call)
CUTS = [pytest.param({}, id="default"), pytest.param({"IPX_JPEG_JPEG_PART": "2", "IPX_JPEG_JPEG_CHUNK": "1"}, id="part2-chunk1")]


@pytest.fixture(params=CUTS)
def cut(request, monkeypatch):
    for k, v in request.param.items():
        monkeypatch.setenv(k, v)


def cmyk_chain(pix, glyphs, col):
    """model pixels (h x w x 4) -> the three streams"""
    frames = _expect(oracle.deep_pix(pix, DEEP_CMYK), DEEP_CMYK, pix.shape[1], pix.shape[0], RESIZE, THUMB, glyphs, col)
    return {k: oracle.jpeg_encode_rgba(f, QUALITY) for k, f in zip(KEYS, frames)}


def _one_pass_ran(capfd):
    return any(l.startswith("[ipx ks] src") for l in capfd.readouterr().err.splitlines())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_leg(ctx, on, cut, size, monkeypatch, capfd):
    w, h = size
    files, pixels = corpus_of(size)
    glyphs = glyphs_of(size)
    assert all(p.shape == (h, w, 4) for p in pixels.values())
    assert ((4 * w * h) % 256 == 0) == (size == (W, H))         # the other sizes: the frame stride is not the frame
    monkeypatch.setenv("IPX_KS_DEBUG", "1")
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(w, h, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    before = ctx.jpeg_cmyk_files()
    capfd.readouterr()
    got, st = plan.run_jpeg_jpeg(files, QUALITY)
    # launch_ks_fused (csrc/ipx_ks_fused.hip): ragged rows only where a pixel is a dword -- the expanded CMYK frames of 50 x 38 leave it.
    # (The three-component files of the call are 4:2:0 planes: the same rule.)
    assert _one_pass_ran(capfd) == (w % 4 == 0), "%dx%d: the one-pass kernel %s" % (w, h, "should have run" if w % 4 == 0 else "should not have run")
    monkeypatch.delenv("IPX_KS_DEBUG")
    assert st == [OK, OK, UNSUPPORTED, OK, OK, OK, OK, OK]
    assert ctx.jpeg_cmyk_files() - before == len(pixels)
    for i, pix in pixels.items():
        want = cmyk_chain(pix, glyphs, DEFAULT_COL)
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


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_leg_texts(ctx, on, cut, size):
    w, h = size
    files, pixels = corpus_of(size)
    texts = file_texts(len(files), w, h, 53)
    plan = ctx.plan(w, h, resize=RESIZE, thumbnail=THUMB, watermark=True)
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
    files = [(cm[(i >> 1) % 4][0] if i & 1 else three[i % 4]) for i in range(40)]      # each of the four files five times
    gs = ctx.glyphset(GLYPHS, DEFAULT_COL)
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=THUMB, watermark=gs)
    want, st = plan.run_jpeg_jpeg(files, QUALITY)
    plan.close()
    gs.close()
    assert st == [OK] * 40
    # the leg's 20 four-component files go up in two groups of the decode driver (16 + 4): the call is held to the model, not only to
    # the pool and the batcher, which run the same leg
    for j in range(4):
        chain = cmyk_chain(cm[j][1], GLYPHS, DEFAULT_COL)
        for i in range(2 * j + 1, 40, 8):
            assert {k: want[k][i] for k in KEYS} == chain, "file %d (four-component file %d)" % (i, j)
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
