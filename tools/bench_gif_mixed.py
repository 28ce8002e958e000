"""GIF uploads of mixed sizes: N photo-like files whose sizes are drawn from K seeded sizes around 1024x768, K in {1, 4, 16, 64}, through
the three mixed entries, each against the only route a caller has without them -- one uniform call per size, in sequence:

  decode   ipx_gif_decode_mixed                     against ipx_gif_decode_batch per size
  encode   ipx_gif_encode_mixed_dev                 against ipx_gif_encode_batch_dev per size (RGBA frames of half the files' sizes in HBM)
  leg      ipx_run_gif_gif_mixed                    against ipx_plan_run_gif_gif per size with a plan of that size

The per-size routes use no new entry, so this script gives their numbers on a commit that has none (the mixed columns are then
skipped, with a note).  Decode and leg with IPX_GIF_PAR unset and set.  At K = 1 the per-size route is the uniform entry itself: the
row shows what the per-frame records cost when there is nothing to gain.  Median of --reps timed calls after one warm-up call.

  python tools/bench_gif_mixed.py                       # the table, one JSON line per (stage, K, IPX_GIF_PAR)
  python tools/bench_gif_mixed.py --n 64 --ks 1,16      # narrower
  python tools/bench_gif_mixed.py --stages encode       # one stage
  python tools/bench_gif_mixed.py --profile             # one K = 16 call of the mixed leg, meant for rocprofv3 --kernel-trace --stats

Files: tests/gif_corpus.py's photo-like generator (256 colours), 4 distinct seeded contents per size, repeated through the batch."""
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
    """file i: size i mod K, content (i div K) mod 4 -> (files, the size of each)"""
    import gif_corpus as gc
    want = [(sizes[i % len(sizes)], (i // len(sizes)) % 4) for i in range(n)]
    distinct = sorted(set(want))
    with cf.ThreadPoolExecutor(16) as pool:
        made = list(pool.map(lambda sc: gc.make(sc[0][0], sc[0][1], seed % 1000 + 977 * sc[1] + sc[0][0], "photo", ncol=256, interlace=False), distinct))
    by = dict(zip(distinct, made))
    return [by[w] for w in want], [w[0] for w in want]


def rgba(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 4), np.int64)
    f[..., 0] = xx * 255 // max(w - 1, 1)
    f[..., 1] = yy * 255 // max(h - 1, 1)
    f[..., 2] = (xx + yy) * 3 % 256
    f[..., :3] += rng.integers(-40, 41, (h, w, 3))
    f[..., 3] = 255
    return f.clip(0, 255).astype(np.uint8)


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
    ap.add_argument("--stages", default="decode,encode,leg")
    ap.add_argument("--routes", default="a,b", help="a: one uniform call per size; b: the mixed entry")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import imageprocessor_amd as ipx
    if ipx.device_count() < 1:
        raise SystemExit("bench_gif_mixed: no GPU (this tool measures the device; there is no CPU fallback)")
    has_mixed = hasattr(ipx.Context, "run_gif_gif_mixed")
    routes = [r for r in a.routes.split(",") if r == "a" or has_mixed]
    if not has_mixed:
        print(json.dumps({"bench": "gif_mixed", "note": "this library has no mixed-size GIF entries: the per-size routes only"}), flush=True)
    ks = [int(k) for k in a.ks.split(",")]
    stages = a.stages.split(",")
    if a.profile:
        ks, stages, a.reps, routes = [16], ["leg"], 1, ["b"]
    ops = {"resize": RESIZE, "thumbnail": THUMB, "watermark": True}

    def row_of(stage, k, par, files, fn_a, fn_b):
        row = {"bench": "gif_mixed", "stage": stage, "k": k, "n": a.n, "par": par}
        if files is not None:
            row["bytes_per_file"] = sum(len(f) for f in files) // len(files)
        if "a" in routes:
            t = timed(fn_a, a.reps)
            row.update(per_size_s=round(t, 4), per_size_per_s=round(a.n / t, 1))
        if "b" in routes:
            t = timed(fn_b, a.reps)
            row.update(mixed_s=round(t, 4), mixed_per_s=round(a.n / t, 1))
        if "per_size_s" in row and "mixed_s" in row:
            row["mixed_over_per_size"] = round(row["per_size_s"] / row["mixed_s"], 3)
        print(json.dumps(row), flush=True)

    with ipx.Context(device=0) as ctx:
        for k in ks:
            sizes = sizes_for(k, a.seed)
            files, size_of = make_files(a.n, sizes, a.seed)
            groups = [(s, [f for f, fs in zip(files, size_of) if fs == s]) for s in sizes]
            groups = [(s, g) for s, g in groups if g]
            if "encode" in stages:
                # frames of half the files' sizes: what the leg's resize output is
                bufs, descs = [], []
                for s, g in groups:
                    w, h = s[0] // 2, s[1] // 2
                    buf = ipx.DevBuffer(ctx, w * h * 4 * len(g))
                    distinct = [rgba(w, h, a.seed % 1000 + c) for c in range(min(len(g), 4))]
                    for i in range(len(g)):
                        buf.upload(distinct[i % len(distinct)], i * w * h * 4)
                    bufs.append((buf, w, h, len(g)))
                    descs += [(buf.ptr + i * w * h * 4, w, h, w * 4) for i in range(len(g))]

                def enc_a():
                    for buf, w, h, m in bufs:
                        _, release = ctx.gif_encode_batch_dev(buf.ptr, w, h, m, copy=False)
                        release()

                def enc_b():
                    _, release = ctx.gif_encode_mixed_dev(descs, copy=False)
                    release()

                row_of("encode", k, 0, None, enc_a, enc_b)
                for buf, _, _, _ in bufs:
                    buf.free()
            plans = {s: ctx.plan(s[0], s[1], resize=RESIZE, thumbnail=THUMB, watermark=True) for s, _ in groups} if "leg" in stages else {}

            def dec_a():
                for s, g in groups:
                    info, st = ctx.gif_decode_batch(g, download=False)
                    assert st.count(0) == len(g), st[:8]
                    info["free"]()

            def dec_b():
                _, st, free = ctx.gif_decode_mixed(files, download=False)
                assert st.count(0) == len(files), st[:8]
                free()

            def leg_a():
                for s, g in groups:
                    _, st = plans[s].run_gif_gif(g, copy=False)
                    assert st.count(0) == len(g), st[:8]

            def leg_b():
                _, st = ctx.run_gif_gif_mixed(ops, files, copy=False)
                assert st.count(0) == len(files), st[:8]

            for par in ("", "1"):
                if a.profile and par:
                    continue
                if par:
                    os.environ["IPX_GIF_PAR"] = par
                else:
                    os.environ.pop("IPX_GIF_PAR", None)
                if "decode" in stages:
                    row_of("decode", k, int(bool(par)), files, dec_a, dec_b)
                if "leg" in stages:
                    row_of("leg", k, int(bool(par)), files, leg_a, leg_b)
            os.environ.pop("IPX_GIF_PAR", None)
            for p in plans.values():
                p.close()


if __name__ == "__main__":
    main()
