"""JPEG, PNG and GIF uploads mixed through the micro-batcher (ipx_batcher_*) on the GPU: single files from many threads; every file's
status and three streams equal the batch entry of its format (ipx_plan_run_jpeg_jpeg / _png_png / _gif_gif) on the same group of files,
and per format sampled files are checked along a chain that does not go through the file legs at all: the CPU decoder (the oracle for
JPEG, the models for PNG and GIF), then the operators and the encoder.  The only non-OK files are the ones broken here on purpose."""
import io
import threading
import time

import numpy as np
import pytest

import gif_decode_model as gdm
import oracle
import png_decode_model as pdm
from helpers import DEFAULT_COL, rgba_frames, text_glyphs
from test_pool_formats_gpu import gif_chain, gif_files, model_statuses, png_chain, png_files

pytestmark = pytest.mark.gpu
PIL = pytest.importorskip("PIL.Image")

SIZES = [(96, 64), (64, 48), (40, 30)]
QUALITY = 85


def _ops(s):
    return dict(resize=(48, 32, False), thumbnail=(24, True), glyphs=text_glyphs(s[0], s[1], n=4, width_px=30, height_px=12), col=DEFAULT_COL)


def _jpeg(rgb, **kw):
    buf = io.BytesIO()
    PIL.fromarray(rgb).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _corpus():
    """-> (files: [(format, (w, h), bytes)], broken: indices); about 200 files per format over the three sizes"""
    files, broken = [], []
    rng = np.random.default_rng(21)
    for s in SIZES:
        w, h = s
        for i in range(66):
            kw = {"quality": int(rng.integers(60, 95))}
            if i % 17 == 0:
                kw["progressive"] = True
            files.append(("jpeg", s, _jpeg(rgba_frames(1, w, h, seed=2000 + 100 * w + i)[0][..., :3], **kw)))
        for fmt, (fs, br) in (("png", png_files(w, h, 69)), ("gif", gif_files(w, h, 68))):
            files += [(fmt, s, f) for i, f in enumerate(fs) if i not in br]
    first = {fmt: next(i for i, f in enumerate(files) if f[0] == fmt) for fmt in ("jpeg", "png", "gif")}
    for fmt, cut in (("jpeg", 200), ("png", -20), ("gif", None)):     # one truncated upload per format
        i = first[fmt] + 5
        data = files[i][2]
        files[i] = (fmt, files[i][1], data[:cut] if cut else data[:len(data) // 2])
        broken.append(i)
    noise = np.random.default_rng(5).integers(0, 256, 777, dtype=np.uint8).tobytes()
    assert noise[:2] != b"\xff\xd8" and noise[:2] != b"\x89P" and noise[:3] != b"GIF"
    files.append(("noise", SIZES[0], noise))                           # goes the JPEG way
    broken.append(len(files) - 1)
    return files, sorted(broken)


def test_mixed_single_files_from_many_threads_equal_the_batch_entries():
    import imageprocessor_amd as ipx
    from test_sources_gpu import _expect_ycbcr_ops
    files, broken = _corpus()
    n = len(files)
    assert n >= 590
    want, sampled = {}, {}
    with ipx.Context(device=0) as ctx:
        for s in SIZES:
            o = _ops(s)
            gs = ctx.glyphset(o["glyphs"], DEFAULT_COL)
            plan = ctx.plan(s[0], s[1], resize=o["resize"], thumbnail=o["thumbnail"], watermark=gs)
            for fmt in ("jpeg", "png", "gif", "noise"):
                idx = [i for i, f in enumerate(files) if f[0] == fmt and f[1] == s]
                if not idx:
                    continue
                group = [files[i][2] for i in idx]
                out, st = {"jpeg": lambda g: plan.run_jpeg_jpeg(g, QUALITY), "noise": lambda g: plan.run_jpeg_jpeg(g, QUALITY),
                           "png": plan.run_png_png, "gif": lambda g: plan.run_gif_gif(g, quality=QUALITY)}[fmt](group)
                for j, i in enumerate(idx):
                    want[i] = (st[j], {k: out[k][j] for k in ("resize", "thumbnail", "watermark")})
                # the CPU chain for a few OK files of this group
                ok = [i for j, i in enumerate(idx) if st[j] == 0][:4]
                if fmt == "jpeg":
                    for i in ok:
                        d = oracle.jpeg_decode(files[i][2])
                        w, h = s
                        ch, cw = (h + 1) // 2, (w + 1) // 2
                        e = _expect_ycbcr_ops(np.ascontiguousarray(d["y"][:h, :w]), np.ascontiguousarray(d["cb"][:ch, :cw]),
                                              np.ascontiguousarray(d["cr"][:ch, :cw]), d["ratio"], o["resize"], o["thumbnail"], o["glyphs"], DEFAULT_COL)
                        sampled[i] = {k: oracle.jpeg_encode_rgba(e[k], QUALITY) for k in e}
                elif fmt == "png":
                    blobs = [f[2] for f in files]
                    _, memo = model_statuses([blobs[i] for i in ok], pdm.decode, pdm.entry_status, s)
                    chain = png_chain(ctx, plan, blobs, memo, ok)
                    for i in ok:
                        sampled[i] = {k: chain[k][i] for k in chain}
                elif fmt == "gif":
                    blobs = [f[2] for f in files]
                    _, memo = model_statuses([blobs[i] for i in ok], gdm.decode, gdm.entry_status, s)
                    chain = gif_chain(plan, blobs, memo, ok, QUALITY)
                    for i in ok:
                        sampled[i] = {k: chain[k][i] for k in chain}
            plan.close()
            gs.close()
    assert [i for i in range(n) if want[i][0] != 0] == broken          # exactly the files broken on purpose
    for fmt in ("jpeg", "png", "gif"):
        assert sum(1 for i in sampled if files[i][0] == fmt) >= 10, fmt
    got, errs = {}, []
    with ipx.Pool(devices=(0,)) as pool, ipx.Batcher(pool, max_batch=48, max_wait_us=3000, quality=QUALITY) as b:
        order = np.random.default_rng(22).permutation(n)

        def work(part):
            try:
                tickets = []
                for i in part:
                    _, (w, h), data = files[i]
                    tickets.append((i, b.submit(data, w, h, **_ops((w, h)))))
                    if len(tickets) >= 6:
                        i0, t0 = tickets.pop(0)
                        got[i0] = b.wait(t0)
                for i0, t0 in tickets:
                    got[i0] = b.wait(t0)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e)[:300])
        ts = [threading.Thread(target=work, args=(order[k::8],)) for k in range(8)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        st = b.stats()
    assert not errs, errs
    assert st["files"] == n and st["largest_batch"] <= 48
    assert len(got) == n
    heads = {"jpeg": (b"\xff\xd8",) * 3, "png": (pdm.SIG,) * 3, "gif": (b"GIF8", b"GIF8", b"\xff\xd8")}
    for i in range(n):
        assert got[i][0] == want[i][0], (i, files[i][0], got[i][0], want[i][0])
        if want[i][0] == 0:
            assert got[i][1] == want[i][1], "file %d (%s): streams differ from the batch entry's" % (i, files[i][0])
            for k, head in zip(("resize", "thumbnail", "watermark"), heads[files[i][0]]):
                assert got[i][1][k].startswith(head), (i, k)
        else:
            assert got[i][1] == {"resize": None, "thumbnail": None, "watermark": None}
    for i, streams in sampled.items():
        for k, v in streams.items():
            assert got[i][1][k] == v, "file %d (%s) %s: differs from the CPU chain" % (i, files[i][0], k)


def test_a_lone_png_does_not_wait_for_the_timer():
    import imageprocessor_amd as ipx
    f = png_files(40, 30, 8)[0][0]
    with ipx.Pool(devices=(0,)) as pool, ipx.Batcher(pool, max_batch=48, max_wait_us=30_000_000, quality=QUALITY) as b:
        t0 = time.perf_counter()
        status, out = b.wait(b.submit(f, 40, 30, resize=(20, 15, False)))
        dt = time.perf_counter() - t0
        st = b.stats()
    assert status == 0 and out["resize"].startswith(pdm.SIG) and out["thumbnail"] is None
    assert st["flushed_when_idle"] >= 1 and st["flushed_by_timer"] == 0 and dt < 30
