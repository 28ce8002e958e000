#!/usr/bin/env python3
"""image.Decode throughput for baseline JPEG batches on the GPU (ipx_jpeg_decode_batch: compressed bytes in host memory ->
*image.YCbCr planes in HBM), next to the CPU oracle and libjpeg (Pillow) on one host thread.
usage: tools/bench_jpeg_dec.py [frames ...]
       tools/bench_jpeg_dec.py --progressive [--j2j] [--profile] [frames ...]
           the same pictures as progressive files: the host scan route (IPX_JPEG_PROG_GPU unset) and the GPU scan walk (=1) in one
           process, alternated, a warm-up first, three repetitions each; one JSON line per batch size with files/s (median, min, max),
           host CPU seconds per file (time.process_time over the timed window), bytes uploaded per file (from the shapes) and one
           file alone.  --j2j: JPEG files -> three JPEG streams (ipx_plan_run_jpeg_jpeg) instead of the decode alone.  --profile: one
           batch of 256 each way and nothing else, for a rocprofv3 --kernel-trace --stats run."""
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

import imageprocessor_amd as ipx  # noqa: E402
import oracle  # noqa: E402

w, h = 1920, 1080
yy, xx = np.mgrid[0:h, 0:w]


def progressive_bench(args):
    flags = {x for x in args if x.startswith("--")}
    sizes = [int(x) for x in args if not x.startswith("--")] or [256, 1024, 4096]
    prog = []
    for k in range(4):
        base = np.stack([np.sin(xx / (40.0 + 7 * k)) * 90 + 128, np.cos(yy / (31.0 + 5 * k)) * 90 + 128, ((xx + 2 * yy) / 6.0 + 40 * k) % 256], -1)
        img = (base + np.random.default_rng(k).normal(0, 6, (h, w, 3))).clip(0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=85, progressive=True)
        prog.append(buf.getvalue())
    nblk = ((w + 15) // 16) * ((h + 15) // 16) * 6
    up = {"host": nblk * 130, "gpu": sum(len(p) for p in prog) // 4}      # int16 coefficients + DC terms, against the file's bytes
    j2j = "--j2j" in flags
    if j2j:
        from helpers import DEFAULT_COL, text_glyphs
        ctx = ipx.Context(lanes=int(os.environ.get("IPX_BENCH_LANES", "5")), lane_bytes=1 << 30)
        gs = ctx.glyphset(text_glyphs(w, h), DEFAULT_COL)
        plan = ctx.plan(w, h, resize=(1024, 768, True), thumbnail=(200, True), watermark=gs)
    else:
        ctx = ipx.Context()

    def run(files, route):
        if route == "gpu":
            os.environ["IPX_JPEG_PROG_GPU"] = "1"
        else:
            os.environ.pop("IPX_JPEG_PROG_GPU", None)
        before = ctx.jpeg_decode_counts()
        c0, t0 = time.process_time(), time.perf_counter()
        if j2j:
            _, st = plan.run_jpeg_jpeg(files, copy=False)
            dt, dc = time.perf_counter() - t0, time.process_time() - c0
        else:
            info, st = ctx.jpeg_decode_batch(files, download=False)
            dt, dc = time.perf_counter() - t0, time.process_time() - c0
            info["free"]()
        rose = [x - y for x, y in zip(ctx.jpeg_decode_counts(), before)]
        assert not any(st) and rose[2 if route == "gpu" else 1] == len(files) and rose[3] == 0, (route, rose)
        return dt, dc

    if "--profile" in flags:
        for route in ("host", "gpu", "host", "gpu"):
            run([prog[i % 4] for i in range(256)], route)
        return
    print("progressive files: %dx%d 4:2:0 q85, %.0f KB each; %s" % (w, h, up["gpu"] / 1e3, "files -> three JPEG streams" if j2j else "ipx_jpeg_decode_batch, planes left in HBM"))
    for route in ("host", "gpu"):
        run(prog * 16, route)                                               # warm-up: allocations, the kernels' code objects
    for n in sizes + [1]:
        files = [prog[i % 4] for i in range(n)]
        t = {"host": [], "gpu": []}
        for rep in range(3 if n > 1 else 5):
            for route in ("host", "gpu"):
                t[route].append(run(files, route))
        row = {"bench": "jpeg_prog_j2j" if j2j else "jpeg_prog_decode", "batch": n}
        for route in ("host", "gpu"):
            dts = sorted(x[0] for x in t[route])
            med = dts[len(dts) // 2]
            row[route] = {"files_per_s": [round(n / med, 1), round(n / dts[-1], 1), round(n / dts[0], 1)], "ms": round(med * 1e3, 2),
                          "host_cpu_s_per_file": round(sorted(x[1] for x in t[route])[len(dts) // 2] / n, 6), "upload_bytes_per_file": up[route]}
        print(json.dumps(row), flush=True)


if "--progressive" in sys.argv[1:]:
    progressive_bench([x for x in sys.argv[1:] if x != "--progressive"])
    sys.exit(0)
pool, pool_rst = [], []
for k in range(4):
    base = np.stack([np.sin(xx / (40.0 + 7 * k)) * 90 + 128, np.cos(yy / (31.0 + 5 * k)) * 90 + 128, ((xx + 2 * yy) / 6.0 + 40 * k) % 256], -1)
    img = (base + np.random.default_rng(k).normal(0, 6, (h, w, 3))).clip(0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=85)
    pool.append(buf.getvalue())
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=85, restart_marker_rows=1)
    pool_rst.append(buf.getvalue())
print("files: %dx%d 4:2:0 q85, %.0f KB each" % (w, h, sum(len(p) for p in pool) / 4 / 1e3))
ctx = ipx.Context()
for n, src, label in [(int(a), pool, "no restart markers") for a in sys.argv[1:] or [256, 1024, 4096]] + [(int(a), pool_rst, "one restart interval per MCU row") for a in sys.argv[1:] or [256, 1024]]:
    files = [src[i % 4] for i in range(n)]
    ctx.jpeg_decode_batch(files[:64], download=False)[0]["free"]()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        info, st = ctx.jpeg_decode_batch(files, download=False)
        dt = time.perf_counter() - t0
        info["free"]()
        best = min(best, dt)
    assert not any(st)
    print("GPU decode, %s, batch of %5d: %.1f ms = %.0f frames/s (parse + pack + upload + Huffman + IDCT, planes left in HBM)" % (label, n, best * 1e3, n / best))
t0 = time.perf_counter()
for i in range(4):
    ref = oracle.jpeg_decode(pool[i])
dt = (time.perf_counter() - t0) / 4
t0 = time.perf_counter()
for i in range(8):
    im = Image.open(io.BytesIO(pool[i % 4]))
    im.draft("YCbCr", (w, h))
    im.load()
dp = (time.perf_counter() - t0) / 8
print("one host thread: oracle (Go's decoder restated) %.1f ms per frame = %.0f frames/s; libjpeg-turbo (Pillow) %.1f ms = %.0f frames/s" % (dt * 1e3, 1 / dt, dp * 1e3, 1 / dp))
