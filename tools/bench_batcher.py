#!/usr/bin/env python3
"""The micro-batcher under load (ipx_batcher_*): S submitter threads, each with ONE file in flight at a time as a goroutine of the
reference has (internal/worker/worker.go:112-149), 1080p 4:2:0 q85 uploads, resize 1024x576 + thumbnail 200 + watermark, three JPEG
streams back.  Prints images/s and the p50 / p99 latency of a file (submit -> its objects), and how the batcher grouped the files.
--format png | gif: photo-like 1024x768 uploads of that format instead (the corpora of tools/bench_png_decode.py and
tools/bench_gif_decode.py: Pillow-written RGB PNGs, 256-colour GIFs), resize 512x384 + thumbnail 64 as those tools ask for; mixed: the
JPEG, PNG and GIF uploads in turn, each with its own size and operators.
--texts: every submitter watermarks with a text of its own (watermark_text of the upload form: 16 glyphs, its own seed), on every format.
Without IPX_BATCH_TEXTS=1 in the environment such files never share a batch; with it they do (ipx_job.texts).
usage: tools/bench_batcher.py [--format jpeg|png|gif|mixed] [--texts] [files per submitter] [max_batch] [max_wait_us] [submitters ...]"""
import io
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

import imageprocessor_amd as ipx  # noqa: E402
from helpers import DEFAULT_COL, text_glyphs  # noqa: E402

argv = sys.argv[1:]
fmt = "jpeg"
if "--format" in argv:
    i = argv.index("--format")
    fmt = argv[i + 1]
    del argv[i:i + 2]
own_texts = "--texts" in argv
if own_texts:
    argv.remove("--texts")
if fmt not in ("jpeg", "png", "gif", "mixed"):
    raise SystemExit("bench_batcher: --format jpeg|png|gif|mixed")
per = int(argv[0]) if len(argv) > 0 else 64
max_batch = int(argv[1]) if len(argv) > 1 else 256
max_wait = int(argv[2]) if len(argv) > 2 else 2000
subs = [int(v) for v in argv[3:]] or [3, 16, 64]


def jpeg_uploads():
    sw, sh = 1920, 1080
    yy, xx = np.mgrid[0:sh, 0:sw]
    out = []
    for k in range(4):
        base = np.stack([np.sin(xx / (40.0 + 7 * k)) * 90 + 128, np.cos(yy / (31.0 + 5 * k)) * 90 + 128, ((xx + 2 * yy) / 6.0 + 40 * k) % 256], -1)
        img = (base + np.random.default_rng(k).normal(0, 6, (sh, sw, 3))).clip(0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=85)
        out.append(buf.getvalue())
    return [(f, sw, sh, dict(resize=(1024, 768, True), thumbnail=(200, True), glyphs=text_glyphs(sw, sh), col=DEFAULT_COL)) for f in out]


def png_uploads(sw=1024, sh=768):
    import png_corpus
    out = []
    for k in range(4):
        buf = io.BytesIO()
        Image.fromarray(png_corpus.photo(sh, sw, 3, 9000 + k).astype(np.uint8), "RGB").save(buf, "PNG")
        out.append(buf.getvalue())
    return [(f, sw, sh, dict(resize=(sw // 2, sh // 2, False), thumbnail=(64, True))) for f in out]


def gif_uploads(sw=1024, sh=768):
    import gif_corpus
    return [(gif_corpus.make(sw, sh, 9000 + k, "photo", ncol=256, interlace=False), sw, sh, dict(resize=(sw // 2, sh // 2, False), thumbnail=(64, True)))
            for k in range(4)]


makers = {"jpeg": jpeg_uploads, "png": png_uploads, "gif": gif_uploads}
if fmt == "mixed":
    files = [u for trio in zip(jpeg_uploads(), png_uploads(), gif_uploads()) for u in trio]
else:
    files = makers[fmt]()
nf = len(files)
_texts = {}


def ops_of(f, k):
    """the operators of upload f for submitter k: as they are, or with submitter k's own text on the watermark"""
    if not own_texts:
        return f[3]
    if (k, f[1], f[2]) not in _texts:
        _texts[(k, f[1], f[2])] = text_glyphs(f[1], f[2], seed=0xA8 + 1 + k)
    return dict(f[3], glyphs=_texts[(k, f[1], f[2])], col=DEFAULT_COL)


with ipx.Pool(devices=(0,)) as pool, ipx.Batcher(pool, max_batch=max_batch, max_wait_us=max_wait, quality=85) as b:
    for t in [b.submit(files[i % nf][0], *files[i % nf][1:3], **ops_of(files[i % nf], i % max(subs))) for i in range(32)]:      # plans, glyph set, lanes warm
        b.wait(t)
    for S in subs:
        lat = []
        mu = threading.Lock()
        before = b.stats()

        def work(k):
            mine = []
            for i in range(per):
                t0 = time.perf_counter()
                f = files[(k + i) % nf]
                st, out = b.wait(b.submit(f[0], f[1], f[2], **ops_of(f, k)))
                mine.append(time.perf_counter() - t0)
                assert st == 0 and out["resize"]
            with mu:
                lat.extend(mine)
        ts = [threading.Thread(target=work, args=(k,)) for k in range(S)]
        t0 = time.perf_counter()
        [t.start() for t in ts]
        [t.join() for t in ts]
        dt = time.perf_counter() - t0
        lat.sort()
        st = b.stats()
        nb = st["batches"] - before["batches"]
        print("%s%s %3d submitters x %d files: %7.0f images/s; latency p50 %.2f ms, p99 %.2f ms; %d batches (mean %.1f files; %d by size, %d by timer, %d when idle)"
              % (fmt, (" own texts, IPX_BATCH_TEXTS=%s" % os.environ.get("IPX_BATCH_TEXTS", "unset")) if own_texts else "", S, per, S * per / dt, lat[len(lat) // 2] * 1e3, lat[min(len(lat) - 1, int(len(lat) * 0.99))] * 1e3, nb, S * per / max(1, nb),
                 st["flushed_by_size"] - before["flushed_by_size"], st["flushed_by_timer"] - before["flushed_by_timer"],
                 st["flushed_when_idle"] - before["flushed_when_idle"]), flush=True)
