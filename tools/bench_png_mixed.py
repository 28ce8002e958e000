"""PNG uploads of mixed sizes: files/s of the whole PNG-to-PNG task (uploads in, three PNG streams per file out) for N photo-like files
whose sizes are drawn from K seeded sizes around 1024x768, K in {1, 4, 16, 64}, by two routes:

  (a) one ipx_plan_run_png_png call per size, in sequence, each with a plan of that size -- what a caller can do with these files
      without the mixed entries.  It uses no new entry, so this script gives the same route's number on a commit that has none.
  (b) one ipx_run_png_png_mixed call over all files (skipped, with a note, where the library does not have it).

Both with IPX_PNG_PAR unset and set.  At K = 1 route (a) is the uniform leg itself: the row shows what the table-driven encoder costs
when there is nothing to gain.  Median of --reps timed calls after one warm-up call, as the sibling tools do.

  python tools/bench_png_mixed.py                       # the table, one JSON line per (K, IPX_PNG_PAR)
  python tools/bench_png_mixed.py --n 64 --ks 1,16      # narrower
  python tools/bench_png_mixed.py --profile             # one K = 16 call of route (b), meant for rocprofv3 --kernel-trace --stats

Files: tests/png_corpus.py's photo-like RGB 8 generator, 16 distinct seeded contents per size, repeated through the batch."""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RESIZE, THUMB = (512, 384, True), (64, True)


def sizes_for(k, seed):
    """k distinct seeded sizes around 1024 x 768 (k = 1: that size itself)"""
    if k == 1:
        return [(1024, 768)]
    rng = np.random.default_rng(seed + k)
    out = []
    while len(out) < k:
        s = (1024 + int(rng.integers(-128, 129)), 768 + int(rng.integers(-96, 97)))
        if s not in out:
            out.append(s)
    return out


def make_files(n, sizes, seed):
    """file i: size i mod K, content (i div K) mod 16 -> (files, the size of each)"""
    import png_corpus as pc
    want = [(sizes[i % len(sizes)], (i // len(sizes)) % 16) for i in range(n)]
    distinct = sorted(set(want))
    with cf.ThreadPoolExecutor(16) as pool:
        made = list(pool.map(lambda sc: pc.of_type(2, 8, False, sc[0][1], sc[0][0], seed=seed + 977 * sc[1] + sc[0][0], kind="photo"), distinct))
    by = dict(zip(distinct, made))
    return [by[w] for w in want], [w[0] for w in want]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20240611)
    ap.add_argument("--routes", default="a,b")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import imageprocessor_amd as ipx
    if ipx.device_count() < 1:
        raise SystemExit("bench_png_mixed: no GPU (this tool measures the device; there is no CPU fallback)")
    has_mixed = hasattr(ipx.Context, "run_png_png_mixed")
    routes = [r for r in a.routes.split(",") if r == "a" or has_mixed]
    if not has_mixed:
        print(json.dumps({"bench": "png_mixed", "note": "this library has no ipx_run_png_png_mixed: route (a) only"}), flush=True)
    ks = [int(k) for k in a.ks.split(",")]
    pars = ["", "1"]
    if a.profile:
        ks, pars, a.reps, routes = [16], [""], 1, ["b"]
    ops = {"resize": RESIZE, "thumbnail": THUMB, "watermark": True}
    with ipx.Context(device=0) as ctx:
        for k in ks:
            sizes = sizes_for(k, a.seed)
            files, size_of = make_files(a.n, sizes, a.seed)
            groups = [(s, [f for f, fs in zip(files, size_of) if fs == s]) for s in sizes]
            groups = [(s, g) for s, g in groups if g]
            plans = {s: ctx.plan(s[0], s[1], resize=RESIZE, thumbnail=THUMB, watermark=True) for s, _ in groups}

            def route_a():
                for s, g in groups:
                    _, st = plans[s].run_png_png(g, copy=False)
                    assert st.count(0) == len(g), st[:8]

            def route_b():
                _, st = ctx.run_png_png_mixed(ops, files, copy=False)
                assert st.count(0) == len(files), st[:8]

            for par in pars:
                if par:
                    os.environ["IPX_PNG_PAR"] = par
                else:
                    os.environ.pop("IPX_PNG_PAR", None)
                row = {"bench": "png_mixed", "k": k, "n": a.n, "par": int(bool(par)), "bytes_per_file": sum(len(f) for f in files) // len(files)}
                if "a" in routes:
                    t = timed(route_a, a.reps)
                    row.update(route_a_s=round(t, 4), route_a_files_per_s=round(a.n / t, 1))
                if "b" in routes:
                    t = timed(route_b, a.reps)
                    row.update(route_b_s=round(t, 4), route_b_files_per_s=round(a.n / t, 1))
                if "route_a_s" in row and "route_b_s" in row:
                    row["b_over_a"] = round(row["route_a_s"] / row["route_b_s"], 3)
                print(json.dumps(row), flush=True)
            for p in plans.values():
                p.close()
    os.environ.pop("IPX_PNG_PAR", None)


if __name__ == "__main__":
    main()
