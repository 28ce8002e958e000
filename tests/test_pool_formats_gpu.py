"""IPX_JOB_PNG and IPX_JOB_GIF through the device pool (csrc/ipx_pool.hip): file jobs of several chunks, every status as the CPU models
say (tests/png_decode_model.py, tests/gif_decode_model.py), every stream equal to the one-context legs (ipx_plan_run_png_png /
ipx_plan_run_gif_gif, which tests/test_png_decode_gpu.py and tests/test_gif_decode_gpu.py hold to the models), and sampled files
along the chain those tests use: the model's frames -> the matching run_host_* -> the encoder.  The only non-OK files are the ones
broken here on purpose."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import gif_corpus
import gif_decode_model as gdm
import png_corpus as pc
import png_decode_model as pdm
from helpers import DEFAULT_COL, text_glyphs

pytestmark = pytest.mark.gpu

SW, SH, N = 96, 64, 300
RESIZE, THUMB = (64, 48, False), (32, True)


def _glyphs(sw=SW, sh=SH):
    return text_glyphs(sw, sh, n=4, width_px=60, height_px=16)


@pytest.fixture(scope="module")
def ipx():
    import imageprocessor_amd as m
    return m


@pytest.fixture(scope="module")
def pool(ipx):
    p = ipx.Pool(devices=(0,))
    yield p
    p.close()


def png_files(sw, sh, n):
    """every row of the type table (the seeds, photo / flat alternation and filter choice of tests/test_png_decode_gpu.py's leg test),
    repeated up to n - 3 files, then one truncated file, one of another size and one Adam7-flagged one; -> (files, indices broken)"""
    from test_png_decode_gpu import _recrc
    distinct = [pc.of_type(ctype, depth, trns, sh, sw, seed=900 + k, kind=("photo", "flat")[k % 2], filters=(k % 5,))
                for k, (_, ctype, depth, trns) in enumerate(pc.TYPES)]
    files = [distinct[i % len(distinct)] for i in range(n - 3)]
    il = bytearray(distinct[3])
    il[8 + 8 + 12] = 1                           # Adam7
    broken = {n // 3: distinct[3][:-20], n // 2: pc.of_type(2, 8, False, sh + 1, sw, seed=1), n - 5: _recrc(bytes(il))}
    for at in sorted(broken):
        files.insert(at, broken[at])
    return files, sorted(broken)


def gif_files(sw, sh, n):
    """photo and flat, interlaced or not, with and without transparency, repeated up to n - 2 files, then one truncated file and one
    of another size; -> (files, indices broken)"""
    distinct = [gif_corpus.make(sw, sh, 700 + k, ("photo", "flat")[k % 2], interlace=bool(k // 2 % 2), transparency=bool(k // 4 % 2))
                for k in range(12)]
    files = [distinct[i % len(distinct)] for i in range(n - 2)]
    broken = {n // 3: distinct[0][:len(distinct[0]) // 2], n // 2: gif_corpus.make(sw - 1, sh, 9)}
    for at in sorted(broken):
        files.insert(at, broken[at])
    return files, sorted(broken)


def model_statuses(files, decode, entry_status, size):
    memo = {}
    for f in files:
        if f not in memo:
            memo[f] = decode(f)
    return [entry_status(memo[f], size) for f in files], memo


def png_chain(ctx, plan, files, memo, idx):
    """{operator: {i: stream}} for the files idx along the CPU chain: the model's frames, the matching run_host_*, png_encode"""
    from test_png_decode_gpu import _host_outputs
    by_kind, out = {}, {}
    for i in idx:
        by_kind.setdefault(memo[files[i]]["kind"], []).append(i)
    for kind, ii in by_kind.items():
        host = _host_outputs(plan, kind, [memo[files[i]] for i in ii])
        for k, frames in host.items():
            for j, i in enumerate(ii):
                out.setdefault(k, {})[i] = ctx.png_encode(frames[j])
    return out


def gif_chain(plan, files, memo, idx, quality, want=("resize", "thumbnail", "watermark")):
    ref = plan.run_host_paletted_gif(np.stack([memo[files[i]]["index"] for i in idx]), np.stack([memo[files[i]]["palette"] for i in idx]),
                                     quality=quality, want=want)
    return {k: {i: v[j] for j, i in enumerate(idx)} for k, v in ref.items()}


def _done(pool):
    return sum(pool.frames_done(s) for s in range(pool.slots()))


def test_png_job_of_several_chunks(ipx, pool):
    files, broken = png_files(SW, SH, N)
    want_st, memo = model_statuses(files, pdm.decode, pdm.entry_status, (SW, SH))
    assert [i for i, s in enumerate(want_st) if s != pdm.OK] == broken      # exactly the files broken on purpose
    glyphs = _glyphs()
    before = _done(pool)
    got, st = pool.submit_files(files, SW, SH, "png", resize=RESIZE, thumbnail=THUMB, glyphs=glyphs, col=DEFAULT_COL).wait()
    assert _done(pool) - before == N
    assert st == want_st
    with ipx.Context(device=0) as ctx:
        gs = ctx.glyphset(glyphs, DEFAULT_COL)
        plan = ctx.plan(SW, SH, resize=RESIZE, thumbnail=THUMB, watermark=gs)
        want, leg_st = plan.run_png_png(files)
        assert leg_st == want_st
        assert sorted(got) == ["resize", "thumbnail", "watermark"]
        for k in got:
            assert got[k] == want[k], k
            assert all((v is None) == (s != pdm.OK) for v, s in zip(got[k], st)) and all(v is None or v[:8] == pdm.SIG for v in got[k])
        ok = [i for i, s in enumerate(st) if s == pdm.OK]
        sample = [ok[j] for j in np.random.default_rng(3).choice(len(ok), 10, replace=False)]
        chain = png_chain(ctx, plan, files, memo, sample)
        for k in got:
            for i in sample:
                assert got[k][i] == chain[k][i], (k, i)
        # a NULL output array leaves that operator out
        part, st2 = pool.submit_files(files[:40], SW, SH, "png", resize=RESIZE, thumbnail=THUMB, glyphs=glyphs, col=DEFAULT_COL,
                                      want=("thumbnail",)).wait()
        assert st2 == want_st[:40] and list(part) == ["thumbnail"] and part["thumbnail"] == want["thumbnail"][:40]
        plan.close()
        gs.close()


def test_gif_job_of_several_chunks(ipx, pool):
    files, broken = gif_files(SW, SH, N)
    want_st, memo = model_statuses(files, gdm.decode, gdm.entry_status, (SW, SH))
    assert [i for i, s in enumerate(want_st) if s != gdm.OK] == broken
    glyphs = _glyphs()
    before = _done(pool)
    got, st = pool.submit_files(files, SW, SH, "gif", 80, resize=RESIZE, thumbnail=THUMB, glyphs=glyphs, col=DEFAULT_COL).wait()
    assert _done(pool) - before == N
    assert st == want_st
    with ipx.Context(device=0) as ctx:
        gs = ctx.glyphset(glyphs, DEFAULT_COL)
        plan = ctx.plan(SW, SH, resize=RESIZE, thumbnail=THUMB, watermark=gs)
        want, leg_st = plan.run_gif_gif(files, quality=80)
        assert leg_st == want_st
        assert sorted(got) == ["resize", "thumbnail", "watermark"]
        for k, head in (("resize", b"GIF8"), ("thumbnail", b"GIF8"), ("watermark", b"\xff\xd8")):
            assert got[k] == want[k], k
            assert all((v is None) == (s != gdm.OK) for v, s in zip(got[k], st)) and all(v is None or v.startswith(head) for v in got[k])
        ok = [i for i, s in enumerate(st) if s == gdm.OK]
        sample = [ok[j] for j in np.random.default_rng(4).choice(len(ok), 10, replace=False)]
        chain = gif_chain(plan, files, memo, sample, 80)
        for k in got:
            for i in sample:
                assert got[k][i] == chain[k][i], (k, i)
        part, st2 = pool.submit_files(files[:40], SW, SH, "gif", 80, resize=RESIZE, thumbnail=THUMB, glyphs=glyphs, col=DEFAULT_COL,
                                      want=("resize", "watermark")).wait()
        assert st2 == want_st[:40] and sorted(part) == ["resize", "watermark"]
        assert part["resize"] == want["resize"][:40] and part["watermark"] == want["watermark"][:40]
        plan.close()
        gs.close()


def test_unknown_kind_and_missing_status_are_invalid(ipx, pool):
    from imageprocessor_amd import _lib
    files, _ = png_files(SW, SH, 8)
    job = pool.submit_files(files, SW, SH, "png", resize=RESIZE, thumbnail=None)
    job.wait()
    j, t = job.job, C.c_uint64()
    j.kind = 10
    assert ipx.lib().ipx_job_submit(pool.handle, C.byref(j), C.byref(t)) == -1
    assert b"unknown job kind" in ipx.lib().ipx_last_error()
    j.kind = 8
    j.status = None
    assert ipx.lib().ipx_job_submit(pool.handle, C.byref(j), C.byref(t)) == -1
    assert b"PNG job needs files and a status array" in ipx.lib().ipx_last_error()
    assert isinstance(j, _lib.Job)


_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import imageprocessor_amd as ipx
from test_pool_formats_gpu import png_files, gif_files, SW, SH, RESIZE, THUMB
pngs, _ = png_files(SW, SH, 300)
gifs, _ = gif_files(SW, SH, 300)
pool = ipx.Pool(devices=(0,))
a = pool.submit_files(pngs, SW, SH, "png", resize=RESIZE, thumbnail=THUMB)
a.release()                      # nobody waited: release waits for the job itself
b = pool.submit_files(gifs, SW, SH, "gif", resize=RESIZE, thumbnail=THUMB)
c = pool.submit_files(pngs, SW, SH, "png", resize=RESIZE, thumbnail=THUMB)
pool.close()                     # b and c still queued or running: the pool finishes them and frees their blocks
b.released = c.released = True   # (their tickets went with the pool)
print("released and destroyed")
"""


def test_release_unwaited_and_destroy_with_work_queued():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(here), here)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "released and destroyed" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
