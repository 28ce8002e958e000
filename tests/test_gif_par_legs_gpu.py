"""The parallel GIF code walk (IPX_GIF_PAR=1) behind the other entries that decode GIF files: ipx_plan_run_gif_gif and its _texts twin,
IPX_JOB_GIF through a one-device pool, one file through the micro-batcher.  The streams and statuses are those of the same call without
the switch, and ipx_gif_decode_counts shows that the files went through the parallel kernel."""
import pytest

import gif_corpus
import gif_decode_model as dm
import gif_edge_corpus as ge
import gif_par_model as pm
from helpers import DEFAULT_COL, text_glyphs
from test_gif_par_gpu import env

pytestmark = pytest.mark.gpu

SW, SH = 64, 48
RESIZE, THUMB = (32, 24, False), (16, True)


def _glyphs(seed=0xA8):
    return text_glyphs(SW, SH, n=3, seed=seed, width_px=40, height_px=12, margin=4)


def _files():
    """Pillow's files and the writer's at 64 x 48, one cut in its data (the serial walk's), one cut in its header (never walked) and one
    of another size; -> (files, statuses, how many reach the walk, how many of those it leaves, the records of the others)"""
    files = [gif_corpus.make(SW, SH, 20 + k, ("photo", "flat")[k % 2], ncol=(256, 16, 5)[k % 3], interlace=k % 2 == 1) for k in range(4)]
    files += [ge.make("leg #%d" % k, SW, SH, bits, lit, 30 + k, kind, interlace=k % 2 == 0, **pol)[1]
              for k, (lit, bits, kind, pol) in enumerate(((8, 8, "noise", dict(clear="never")), (3, 2, "runs", dict(clear="every", every=64)),
                                                          (5, 5, "photo", dict(clear="full", lead=False, double=True))))]
    files.insert(2, files[4][:len(files[4]) * 3 // 4])
    files.insert(5, files[0][:11])
    files.insert(7, gif_corpus.make(SW + 1, SH, 3, "photo", ncol=256))
    res = [dm.decode(f) for f in files]
    st = [dm.entry_status(r, (SW, SH)) for r in res]
    walked = [f for f, r, s in zip(files, res, st) if r["stage"] != "container" and s != dm.UNSUPPORTED]
    pars = [pm.par_walk(pm.stream_of(f)) for f in walked]
    return files, st, len(walked), sum(1 for p in pars if p.redo), sum(len(p.records) for p in pars if not p.redo)


@pytest.fixture(scope="module")
def ipx():
    import imageprocessor_amd as m
    return m


def _leg(ipx, texts):
    files, want_st, walked, left, records = _files()
    assert (walked, left) == (len(files) - 2, 1) and want_st.count(dm.OK) == len(files) - 3
    tx = None if texts is None else [texts[i % len(texts)] for i in range(len(files))]
    with ipx.Context(device=0) as ctx:
        gs = ctx.glyphset(_glyphs(), DEFAULT_COL) if texts is None else None
        plan = ctx.plan(SW, SH, resize=RESIZE, thumbnail=THUMB, watermark=gs if gs is not None else True)
        with env():
            ref, ref_st = plan.run_gif_gif(files, quality=80, texts=tx)
        assert ctx.gif_decode_counts() == [0] * 4
        with env(IPX_GIF_PAR=1):
            got, st = plan.run_gif_gif(files, quality=80, texts=tx)
        c = ctx.gif_decode_counts()
        plan.close()
        if gs is not None:
            gs.close()
    assert st == ref_st == want_st
    assert got == ref and all(v is not None for k in got for v, s in zip(got[k], st) if s == dm.OK)
    assert c == [walked, walked - left, left, records]


def test_run_gif_gif(ipx):
    _leg(ipx, None)


def test_run_gif_gif_texts(ipx):
    _leg(ipx, [(_glyphs(1), DEFAULT_COL), (_glyphs(2), (10, 200, 30, 255))])


def test_job_gif_through_a_pool(ipx):
    files, want_st, walked, left, records = _files()
    with ipx.Pool(devices=(0,)) as pool:
        kw = dict(resize=RESIZE, thumbnail=THUMB, glyphs=_glyphs(), col=DEFAULT_COL)
        with env():
            ref, ref_st = pool.submit_files(files, SW, SH, "gif", **kw).wait()
        assert pool.gif_decode_counts() == [0] * 4
        with env(IPX_GIF_PAR=1):
            got, st = pool.submit_files(files, SW, SH, "gif", **kw).wait()
        c = pool.gif_decode_counts()
    assert st == ref_st == want_st and got == ref
    assert c == [walked, walked - left, left, records]


def test_one_file_through_the_micro_batcher(ipx):
    f = ge.make("single", SW, SH, 8, 8, 77, "photo", clear="full")[1]
    records = len(pm.par_walk(pm.stream_of(f)).records)
    with ipx.Pool(devices=(0,)) as pool, ipx.Batcher(pool, max_batch=8, max_wait_us=2000, quality=85) as b:
        with env():
            ref_st, ref = b.wait(b.submit(f, SW, SH, resize=RESIZE))
        assert pool.gif_decode_counts() == [0] * 4
        with env(IPX_GIF_PAR=1):
            st, got = b.wait(b.submit(f, SW, SH, resize=RESIZE))
        c = pool.gif_decode_counts()
    assert st == ref_st == dm.OK and got == ref and got["resize"].startswith(b"GIF8")
    assert c == [1, 1, 0, records]
