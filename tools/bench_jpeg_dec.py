#!/usr/bin/env python3
"""image.Decode throughput for baseline JPEG batches on the GPU (ipx_jpeg_decode_batch: compressed bytes in host memory ->
*image.YCbCr planes in HBM), next to the CPU oracle and libjpeg (Pillow) on one host thread.
usage: tools/bench_jpeg_dec.py [frames ...]
       tools/bench_jpeg_dec.py --progressive [--j2j] [--profile] [frames ...]
           the same pictures as progressive files: the host scan route (IPX_JPEG_PROG_GPU unset) and the GPU scan walk (=1) in one
           process, alternated, a warm-up first, three repetitions each; one JSON line per batch size with files/s (median, min, max),
           host CPU seconds per file (time.process_time over the timed window), bytes uploaded per file (from the shapes) and one
           file alone.  --j2j: JPEG files -> three JPEG streams (ipx_plan_run_jpeg_jpeg) instead of the decode alone.  --profile: one
           batch of 256 each way and nothing else, for a rocprofv3 --kernel-trace --stats run.
       tools/bench_jpeg_dec.py --cmyk [--j2j] [--profile] [--corpus DIR] [frames ...]
           four-component files under IPX_JPEG_CMYK=1 (ipx_jpeg_decode_batch_cmyk, or with --j2j the files -> three JPEG streams):
           1080p YCCK files of the vector 22 11 11 22, baseline, written by tests/jpeg_cmyk_writer.py from the quantised DCT of the
           pictures above (Pillow writes transform-0 files of the vector 11 11 11 11 only); a warm-up, three repetitions, one JSON
           line per batch size.  --corpus DIR keeps the files there (writing one takes the Python writer a while) and reads them back
           when they exist.  --profile: two batches of 256 and nothing else.
       tools/bench_jpeg_dec.py --411 [--corpus DIR] [frames ...]
           4:1:1 files (Y 4x1 over 1x1 chroma) under IPX_JPEG_411=1 beside 4:2:0 files of the same pictures, same quantisers and same
           Huffman tables in the same process: 1080p baseline files written by tests/jpeg_writer.py from the quantised DCT of the
           pictures above (libjpeg-turbo's Python front end writes no 4:1:1); a warm-up, three repetitions alternated, one JSON line per
           batch size (default 1, 256, 1024) with files/s (median, min, max) of both.  --corpus DIR as for --cmyk."""
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


def cmyk_corpus(folder, count=2):
    """count 1080p YCCK files (22 11 11 22, transform 2) from the quantised DCT of synthetic pictures"""
    import jpeg_cmyk_writer as cw
    import jpeg_writer as jw
    files = []
    k8 = np.arange(8)
    dct = np.sqrt(2.0 / 8) * np.cos((2 * k8[None, :] + 1) * k8[:, None] * np.pi / 16)
    dct[0] /= np.sqrt(2.0)
    q85 = oracle.jpeg_quant(85)
    q = {0: [int(v) for v in q85[0]], 1: [int(v) for v in q85[1]], 2: [int(v) for v in q85[0]]}
    for k in range(count):
        path = os.path.join(folder, "ycck_1080p_%d.jpg" % k) if folder else None
        if path and os.path.exists(path):
            files.append(open(path, "rb").read())
            continue
        frame = cw.frame4(w, h, 2)
        planes = [np.sin(xx / (40.0 + 7 * k)) * 90 + 128, np.cos(yy / (31.0 + 5 * k)) * 40 + 128, ((xx + 2 * yy) / 6.0 + 40 * k) % 64 + 96,
                  np.cos((xx - yy) / (53.0 + 3 * k)) * 100 + 128]
        noise = np.random.default_rng(k)
        blocks = []
        for c in range(4):
            rows, cols = frame.grid(c)
            p = (planes[c] + noise.normal(0, 6, (h, w))).clip(0, 255)
            if c in (1, 2):
                p = p[::2, ::2]
            full = np.zeros((rows * 8, cols * 8))
            full[:p.shape[0], :p.shape[1]] = p
            full[p.shape[0]:, :] = full[p.shape[0] - 1:p.shape[0], :]           # edge replication, as an encoder pads
            full[:, p.shape[1]:] = full[:, p.shape[1] - 1:p.shape[1]]
            b = (full - 128).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)
            coef = np.einsum("ij,rcjk,lk->rcil", dct, b, dct).reshape(rows, cols, 64)[..., jw.ZIG]
            blocks.append(np.rint(coef / np.asarray(q[frame.comps[c][3]], float)).astype(np.int64))
        data = cw.cmyk_file(frame, blocks, transform=2, q=q)
        if path:
            os.makedirs(folder, exist_ok=True)
            with open(path, "wb") as fh:
                fh.write(data)
        files.append(data)
    return files


def cmyk_bench(args):
    os.environ["IPX_JPEG_CMYK"] = "1"
    flags = {x for x in args if x.startswith("--")}
    folder = args[args.index("--corpus") + 1] if "--corpus" in args else None
    sizes = [int(x) for x in args if x.isdigit()] or [256, 1024]
    src = cmyk_corpus(folder)
    if "--write-only" in flags:
        return
    j2j = "--j2j" in flags
    if j2j:
        from helpers import DEFAULT_COL, text_glyphs
        ctx = ipx.Context(lanes=int(os.environ.get("IPX_BENCH_LANES", "5")), lane_bytes=1 << 30)
        gs = ctx.glyphset(text_glyphs(w, h), DEFAULT_COL)
        plan = ctx.plan(w, h, resize=(1024, 768, True), thumbnail=(200, True), watermark=gs)
    else:
        ctx = ipx.Context()

    def run(files):
        before = ctx.jpeg_cmyk_files()
        c0, t0 = time.process_time(), time.perf_counter()
        if j2j:
            _, st = plan.run_jpeg_jpeg(files, copy=False)
            dt, dc = time.perf_counter() - t0, time.process_time() - c0
        else:
            info, st = ctx.jpeg_decode_batch_cmyk(files, download=False)
            dt, dc = time.perf_counter() - t0, time.process_time() - c0
            info["free"]()
        assert not any(st) and ctx.jpeg_cmyk_files() - before == len(files), st[:8]
        return dt, dc

    if "--profile" in flags:
        for _ in range(2):
            run([src[i % len(src)] for i in range(256)])
        return
    print("YCCK files: %dx%d 22 11 11 22 q85 baseline, %.0f KB each; %s" % (w, h, sum(len(p) for p in src) / len(src) / 1e3,
                                                                           "files -> three JPEG streams" if j2j else "ipx_jpeg_decode_batch_cmyk, frames left in HBM"))
    run(src * 32)                                                           # warm-up
    for n in sizes:
        files = [src[i % len(src)] for i in range(n)]
        t = [run(files) for _ in range(3)]
        dts = sorted(x[0] for x in t)
        print(json.dumps({"bench": "jpeg_cmyk_j2j" if j2j else "jpeg_cmyk_decode", "batch": n,
                          "files_per_s": [round(n / dts[1], 1), round(n / dts[-1], 1), round(n / dts[0], 1)], "ms": round(dts[1] * 1e3, 2),
                          "host_cpu_s_per_file": round(sorted(x[1] for x in t)[1] / n, 6)}), flush=True)


def sampled_corpus(folder, h0, v0, count=2):
    """count 1080p baseline files with luma factors (h0, v0) over 1x1 chroma, from the quantised DCT of synthetic pictures"""
    import jpeg_edge_corpus as ec
    import jpeg_writer as jw
    files = []
    k8 = np.arange(8)
    dct = np.sqrt(2.0 / 8) * np.cos((2 * k8[None, :] + 1) * k8[:, None] * np.pi / 16)
    dct[0] /= np.sqrt(2.0)
    q85 = oracle.jpeg_quant(85)
    q = {0: [int(v) for v in q85[0]], 1: [int(v) for v in q85[1]]}
    dc, ac, _ = ec.tables_short()
    for k in range(count):
        path = os.path.join(folder, "y%dx%d_1080p_%d.jpg" % (h0, v0, k)) if folder else None
        if path and os.path.exists(path):
            files.append(open(path, "rb").read())
            continue
        frame = jw.Frame(w, h, [(1, h0, v0, 0), (2, 1, 1, 1), (3, 1, 1, 1)])
        planes = [np.sin(xx / (40.0 + 7 * k)) * 90 + 128, np.cos(yy / (31.0 + 5 * k)) * 40 + 128, ((xx + 2 * yy) / 6.0 + 40 * k) % 64 + 96]
        noise = np.random.default_rng(k)
        blocks = []
        for c in range(3):
            rows, cols = frame.grid(c)
            p = (planes[c] + noise.normal(0, 6, (h, w))).clip(0, 255)
            if c:
                p = p[::v0, ::h0]
            full = np.zeros((rows * 8, cols * 8))
            full[:p.shape[0], :p.shape[1]] = p
            full[p.shape[0]:, :] = full[p.shape[0] - 1:p.shape[0], :]           # edge replication, as an encoder pads
            full[:, p.shape[1]:] = full[:, p.shape[1] - 1:p.shape[1]]
            b = (full - 128).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)
            coef = np.einsum("ij,rcjk,lk->rcil", dct, b, dct).reshape(rows, cols, 64)[..., jw.ZIG]
            blocks.append(np.rint(coef / np.asarray(q[frame.comps[c][3]], float)).astype(np.int64))
        data = ec.file(w, h, frame.comps, blocks, {(0, 0): dc, (1, 0): ac, (0, 1): dc, (1, 1): ac}, {0: (q[0], 0), 1: (q[1], 0)})
        if path:
            os.makedirs(folder, exist_ok=True)
            with open(path, "wb") as fh:
                fh.write(data)
        files.append(data)
    return files


def s411_bench(args):
    os.environ["IPX_JPEG_411"] = "1"
    flags = {x for x in args if x.startswith("--")}
    folder = args[args.index("--corpus") + 1] if "--corpus" in args else None
    sizes = [int(x) for x in args if x.isdigit()] or [1, 256, 1024]
    src = {"411": sampled_corpus(folder, 4, 1), "420": sampled_corpus(folder, 2, 2)}
    if "--write-only" in flags:
        return
    ctx = ipx.Context()

    def run(files):
        t0 = time.perf_counter()
        info, st = ctx.jpeg_decode_batch(files, download=False)
        dt = time.perf_counter() - t0
        info["free"]()
        assert not any(st), st[:8]
        return dt

    print("files: %dx%d q85 baseline, one scan, the writer's Huffman tables; 4:1:1 %.0f KB each, 4:2:0 %.0f KB each; ipx_jpeg_decode_batch, planes left in HBM"
          % (w, h, sum(len(p) for p in src["411"]) / len(src["411"]) / 1e3, sum(len(p) for p in src["420"]) / len(src["420"]) / 1e3))
    for kind in src:
        run(src[kind] * 32)                                                 # warm-up
    for n in sizes:
        t = {kind: [] for kind in src}
        for rep in range(3 if n > 1 else 5):
            for kind in src:
                t[kind].append(run([src[kind][i % len(src[kind])] for i in range(n)]))
        row = {"bench": "jpeg_411_decode", "batch": n}
        for kind in src:
            dts = sorted(t[kind])
            med = dts[len(dts) // 2]
            row[kind] = {"files_per_s": [round(n / med, 1), round(n / dts[-1], 1), round(n / dts[0], 1)], "ms": round(med * 1e3, 2)}
        print(json.dumps(row), flush=True)


if "--411" in sys.argv[1:]:
    s411_bench([x for x in sys.argv[1:] if x != "--411"])
    sys.exit(0)
if "--cmyk" in sys.argv[1:]:
    cmyk_bench([x for x in sys.argv[1:] if x != "--cmyk"])
    sys.exit(0)
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
