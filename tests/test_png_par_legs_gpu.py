"""The parallel inflate (IPX_PNG_PAR=1) behind the other entries that decode PNG files: ipx_plan_run_png_png and its _texts twin on a
mixed-kind batch, IPX_JOB_PNG through a one-device pool, one file through the micro-batcher.  The streams and statuses are those of the
same call without the switch, and ipx_png_decode_counts shows that the files went through the parallel kernel."""
import pytest

import png_corpus as pc
import png_decode_model as dm
from helpers import DEFAULT_COL, text_glyphs
from test_png_par_gpu import env

pytestmark = pytest.mark.gpu

SW, SH = 64, 48
RESIZE, THUMB = (32, 24, False), (16, True)


def _glyphs(seed=0xA8):
    return text_glyphs(SW, SH, n=3, seed=seed, width_px=40, height_px=12, margin=4)


def _files():
    """every row of the type table at 64 x 48, a truncated file and one of another size; -> (files, how many reach the decoder)"""
    files = [pc.of_type(ctype, depth, trns, SH, SW, seed=300 + k, kind=("photo", "flat")[k % 2], filters=(k % 5, 4))
             for k, (_, ctype, depth, trns) in enumerate(pc.TYPES)]
    files.insert(5, files[8][:-40])                                      # cut inside the IDAT chunk: the container does not parse
    files.insert(9, pc.of_type(2, 8, False, SH + 1, SW, seed=1))
    damaged = bytearray(files[12])
    damaged[len(damaged) // 2] ^= 0x10                                   # a chunk CRC fails: parsed, decoded by neither kernel
    files.insert(13, bytes(damaged))
    res = [dm.decode(f) for f in files]
    return files, sum(1 for r in res if r["stage"] == "data" and (r["w"], r["h"]) == (SW, SH)), [dm.entry_status(r, (SW, SH)) for r in res]


@pytest.fixture(scope="module")
def ipx():
    import imageprocessor_amd as m
    return m


def _leg(ipx, texts):
    files, parsed, want_st = _files()
    assert parsed == len(files) - 2 and want_st.count(dm.OK) == len(files) - 3
    tx = None if texts is None else [texts[i % len(texts)] for i in range(len(files))]
    with ipx.Context(device=0) as ctx:
        gs = ctx.glyphset(_glyphs(), DEFAULT_COL) if texts is None else None
        plan = ctx.plan(SW, SH, resize=RESIZE, thumbnail=THUMB, watermark=gs if gs is not None else True)
        with env():
            ref, ref_st = plan.run_png_png(files, texts=tx)
        assert ctx.png_decode_counts() == [0] * 5
        with env(IPX_PNG_PAR=1):
            got, st = plan.run_png_png(files, texts=tx)
        c = ctx.png_decode_counts()
        plan.close()
        if gs is not None:
            gs.close()
    assert st == ref_st == want_st
    assert got == ref and all(v is not None for k in got for v, s in zip(got[k], st) if s == dm.OK)
    assert c[0] == parsed and c[0] == c[1] + c[2] and c[2] == 1 and c[3] > 0


def test_run_png_png(ipx):
    _leg(ipx, None)


def test_run_png_png_texts(ipx):
    _leg(ipx, [(_glyphs(1), DEFAULT_COL), (_glyphs(2), (10, 200, 30, 255))])


def test_job_png_through_a_pool(ipx):
    files, parsed, want_st = _files()
    with ipx.Pool(devices=(0,)) as pool:
        kw = dict(resize=RESIZE, thumbnail=THUMB, glyphs=_glyphs(), col=DEFAULT_COL)
        with env():
            ref, ref_st = pool.submit_files(files, SW, SH, "png", **kw).wait()
        assert pool.png_decode_counts() == [0] * 5
        with env(IPX_PNG_PAR=1):
            got, st = pool.submit_files(files, SW, SH, "png", **kw).wait()
        c = pool.png_decode_counts()
    assert st == ref_st == want_st and got == ref
    assert c[0] == parsed and c[0] == c[1] + c[2] and c[2] == 1 and c[3] > 0


def test_one_file_through_the_micro_batcher(ipx):
    f = pc.of_type(6, 8, False, SH, SW, seed=77, filters=(4,))
    with ipx.Pool(devices=(0,)) as pool, ipx.Batcher(pool, max_batch=8, max_wait_us=2000, quality=85) as b:
        with env():
            ref_st, ref = b.wait(b.submit(f, SW, SH, resize=RESIZE))
        assert pool.png_decode_counts() == [0] * 5
        with env(IPX_PNG_PAR=1):
            st, got = b.wait(b.submit(f, SW, SH, resize=RESIZE))
        c = pool.png_decode_counts()
    assert st == ref_st == dm.OK and got == ref and got["resize"].startswith(dm.SIG)
    assert c[:3] == [1, 1, 0] and c[3] > 0
