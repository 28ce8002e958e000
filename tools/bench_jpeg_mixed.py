"""JPEG uploads of mixed sizes: files/s for N photo-like 4:2:0 quality-85 files whose sizes are drawn from K seeded sizes around
1920x1080, K in {1, 4, 16, 64}, by two routes, for the whole JPEG-to-JPEG task (uploads in, three JPEG streams per file out) and for
the decode entry alone:

  (a) one uniform call per size, in sequence -- ipx_plan_run_jpeg_jpeg with a plan of that size; ipx_jpeg_decode_batch -- which is what
      a caller can do with these files without the mixed entries.  It uses no new entry, so this script gives the same route's number
      on a commit that has none.
  (b) one mixed call over all files -- ipx_run_jpeg_jpeg_mixed; ipx_jpeg_decode_mixed (skipped, with a note, where the library has
      neither).

Both routes on the same files in the same process.  At K = 1 route (a) is the uniform entry itself: the row shows what the per-image
records cost when there is nothing to gain.  Median of --reps timed calls after one warm-up call, as the sibling tools do.

  python tools/bench_jpeg_mixed.py                       # the table, one JSON line per K and entry
  python tools/bench_jpeg_mixed.py --n 64 --ks 1,16      # narrower
  python tools/bench_jpeg_mixed.py --memory              # one K = 64 call per route with IPX_DEBUG_J2J=1: the decode lines on stderr
                                                         # carry the bytes of planes and scratch of every decode pass
  python tools/bench_jpeg_mixed.py --profile             # one K = 16 call of route (b), meant for rocprofv3 --kernel-trace --stats

Files: four seeded photo-like pictures, cut to each size and written by Pillow (4:2:0, quality 85, Annex K tables, no restart markers)."""
import argparse
import concurrent.futures as cf
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RESIZE, THUMB, QUALITY = (1024, 768, True), (200, True), 85
W0, H0 = 1920, 1080


def sizes_for(k, seed):
    """k distinct seeded sizes around 1920 x 1080 (k = 1: that size itself)"""
    if k == 1:
        return [(W0, H0)]
    rng = np.random.default_rng(seed + k)
    out = []
    while len(out) < k:
        s = (W0 + int(rng.integers(-128, 129)), H0 + int(rng.integers(-96, 97)))
        if s not in out:
            out.append(s)
    return out


def pictures():
    w, h = W0 + 128, H0 + 96
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(4):
        base = np.stack([np.sin(xx / (40.0 + 7 * k)) * 90 + 128, np.cos(yy / (31.0 + 5 * k)) * 90 + 128, ((xx + 2 * yy) / 6.0 + 40 * k) % 256], -1)
        out.append((base + np.random.default_rng(k).normal(0, 6, (h, w, 3))).clip(0, 255).astype(np.uint8))
    return out


def make_files(n, sizes, pics):
    """file i: size i mod K, picture (i div K) mod 4 -> (files, the size of each)"""
    from PIL import Image
    want = [(sizes[i % len(sizes)], (i // len(sizes)) % 4) for i in range(n)]
    distinct = sorted(set(want))

    def one(sc):
        (w, h), c = sc
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(pics[c][:h, :w])).save(buf, "JPEG", quality=QUALITY)
        return buf.getvalue()
    with cf.ThreadPoolExecutor(16) as pool:
        made = list(pool.map(one, distinct))
    by = dict(zip(distinct, made))
    return [by[x] for x in want], [x[0] for x in want]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--routes", default="a,b")
    ap.add_argument("--entries", default="leg,decode")
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import imageprocessor_amd as ipx
    if ipx.device_count() < 1:
        raise SystemExit("bench_jpeg_mixed: no GPU (this tool measures the device; there is no CPU fallback)")
    has_mixed = hasattr(ipx.Context, "run_jpeg_jpeg_mixed")
    routes = [r for r in a.routes.split(",") if r == "a" or has_mixed]
    if not has_mixed:
        print(json.dumps({"bench": "jpeg_mixed", "note": "this library has no ipx_run_jpeg_jpeg_mixed: route (a) only"}), flush=True)
    ks = [int(k) for k in a.ks.split(",")]
    entries = a.entries.split(",")
    if a.profile:
        ks, a.reps, routes, entries = [16], 1, ["b"], ["leg"]
    if a.memory:
        ks, a.reps = [64], 1
        os.environ["IPX_DEBUG_J2J"] = "1"
    ops = {"resize": RESIZE, "thumbnail": THUMB, "watermark": True}
    pics = pictures()
    with ipx.Context(device=0, lanes=int(os.environ.get("IPX_BENCH_LANES", "5")), lane_bytes=1 << 30) as ctx:
        for k in ks:
            sizes = sizes_for(k, a.seed)
            files, size_of = make_files(a.n, sizes, pics)
            groups = [(s, [f for f, fs in zip(files, size_of) if fs == s]) for s in sizes]
            groups = [(s, g) for s, g in groups if g]
            plans = {s: ctx.plan(s[0], s[1], resize=RESIZE, thumbnail=THUMB, watermark=True) for s, _ in groups}

            def leg_a():
                for s, g in groups:
                    _, st = plans[s].run_jpeg_jpeg(g, quality=QUALITY, copy=False)
                    assert st.count(0) == len(g), st[:8]

            def leg_b():
                _, st = ctx.run_jpeg_jpeg_mixed(ops, files, quality=QUALITY, copy=False)
                assert st.count(0) == len(files), st[:8]

            def decode_a():
                for s, g in groups:
                    info, st = ctx.jpeg_decode_batch(g, download=False)
                    info["free"]()
                    assert st.count(0) == len(g), st[:8]

            def decode_b():
                _, st, free = ctx.jpeg_decode_mixed(files, download=False)
                free()
                assert st.count(0) == len(files), st[:8]

            for entry, fa, fb in (("leg", leg_a, leg_b), ("decode", decode_a, decode_b)):
                if entry not in entries:
                    continue
                row = {"bench": "jpeg_mixed", "entry": entry, "k": k, "n": a.n, "bytes_per_file": sum(len(f) for f in files) // len(files)}
                if "a" in routes:
                    if a.memory:
                        print("[bench_jpeg_mixed] %s, K = %d, route (a): one uniform call per size" % (entry, k), file=sys.stderr, flush=True)
                    t, lo, hi = timed(fa, a.reps)
                    row.update(route_a_s=round(t, 4), route_a_files_per_s=round(a.n / t, 1), route_a_min_max_s=[round(lo, 4), round(hi, 4)])
                if "b" in routes:
                    if a.memory:
                        print("[bench_jpeg_mixed] %s, K = %d, route (b): one mixed call" % (entry, k), file=sys.stderr, flush=True)
                    t, lo, hi = timed(fb, a.reps)
                    row.update(route_b_s=round(t, 4), route_b_files_per_s=round(a.n / t, 1), route_b_min_max_s=[round(lo, 4), round(hi, 4)])
                if "route_a_s" in row and "route_b_s" in row:
                    row["b_over_a"] = round(row["route_a_s"] / row["route_b_s"], 3)
                print(json.dumps(row), flush=True)
            for p in plans.values():
                p.close()


if __name__ == "__main__":
    main()
