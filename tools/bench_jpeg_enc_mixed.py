"""jpeg.Encode of frames of mixed sizes, the entry alone: frames/s for N photo-like RGBA frames resident in HBM whose sizes are drawn from
K seeded sizes around 1024x768, K in {1, 4, 16, 64}, quality 85, by two routes:

  (a) one ipx_jpeg_encode_batch_dev call per size, in sequence (the frames of a size lie one frame stride apart) -- what a caller can
      do with these frames without the mixed entry: three waits for the device per size;
  (b) one ipx_jpeg_encode_mixed_dev call over all frames: three waits in all (skipped, with a note, where the library has none).

Both routes on the same frames in the same process; the streams of the two routes are compared once, byte for byte, before anything is
timed.  At K = 1 route (a) is the uniform entry itself: the row shows what the per-frame records cost when there is nothing to gain.
Median of --reps timed calls after one warm-up call, as the sibling tools do.

  python tools/bench_jpeg_enc_mixed.py                       # the table, one JSON line per K
  python tools/bench_jpeg_enc_mixed.py --n 64 --ks 1,16      # narrower
  python tools/bench_jpeg_enc_mixed.py --profile             # one K = 16 call of route (b), meant for rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUALITY = 85
W0, H0 = 1024, 768


def sizes_for(k, seed):
    """k distinct seeded sizes around 1024 x 768 (k = 1: that size itself)"""
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
        base = np.stack([np.sin(xx / (40.0 + 7 * k)) * 90 + 128, np.cos(yy / (31.0 + 5 * k)) * 90 + 128, ((xx + 2 * yy) / 6.0 + 40 * k) % 256,
                         np.full((h, w), 255.0)], -1)
        base[..., :3] += np.random.default_rng(k).normal(0, 6, (h, w, 3))
        out.append(base.clip(0, 255).astype(np.uint8))
    return out


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
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import imageprocessor_amd as ipx
    if ipx.device_count() < 1:
        raise SystemExit("bench_jpeg_enc_mixed: no GPU (this tool measures the device; there is no CPU fallback)")
    has_mixed = hasattr(ipx.Context, "jpeg_encode_mixed_dev")
    if not has_mixed:
        print(json.dumps({"bench": "jpeg_enc_mixed", "note": "this library has no ipx_jpeg_encode_mixed_dev: route (a) only"}), flush=True)
    ks = [int(k) for k in a.ks.split(",")]
    if a.profile:
        ks, a.reps = [16], 1
    pics = pictures()
    with ipx.Context(device=0, lane_bytes=1 << 30) as ctx:
        for k in ks:
            sizes = sizes_for(k, a.seed)
            # the frames of a size lie together, tightly packed, one 256-aligned frame stride apart
            groups, recs = [], []
            for j, (w, h) in enumerate(sizes):
                m = len(range(j, a.n, k))
                if m == 0:
                    continue
                fs = (4 * w * h + 255) & ~255
                buf = ctx.alloc(fs * m)
                for q in range(m):
                    buf.upload(np.ascontiguousarray(pics[q % 4][:h, :w]), offset=q * fs)
                    recs.append((buf.ptr + q * fs, w, h, 4 * w))
                groups.append((buf, w, h, fs, m))

            def route_a(copy=False):
                out = []
                for buf, w, h, fs, m in groups:
                    r = ctx.jpeg_encode_batch_dev(buf.ptr, w, h, m, QUALITY, frame_stride=fs, copy=copy)
                    if copy:
                        out += r
                    else:
                        r[1]()
                return out

            def route_b(copy=False):
                r = ctx.jpeg_encode_mixed_dev(recs, QUALITY, copy=copy)
                if copy:
                    return r
                r[1]()

            row = {"bench": "jpeg_enc_mixed", "k": k, "n": a.n, "quality": QUALITY}
            if has_mixed and not a.profile:
                want = route_a(copy=True)
                assert route_b(copy=True) == want, "the two routes disagree"
                row["bytes_per_frame"] = sum(len(s) for s in want) // len(want)
            if not a.profile:
                t, lo, hi = timed(route_a, a.reps)
                row.update(route_a_s=round(t, 4), route_a_frames_per_s=round(a.n / t, 1), route_a_min_max_s=[round(lo, 4), round(hi, 4)])
            if has_mixed:
                t, lo, hi = timed(route_b, a.reps)
                row.update(route_b_s=round(t, 4), route_b_frames_per_s=round(a.n / t, 1), route_b_min_max_s=[round(lo, 4), round(hi, 4)])
            if "route_a_s" in row and "route_b_s" in row:
                row["b_over_a"] = round(row["route_a_s"] / row["route_b_s"], 3)
            print(json.dumps(row), flush=True)
            for g in groups:
                g[0].free()


if __name__ == "__main__":
    main()
