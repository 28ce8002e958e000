"""gif.Encode on the GPU: frames/s from frames resident in HBM to finished GIF streams in host memory (ipx_gif_encode_batch_dev),
at 1024x768 and 200x200 for batches of 1, 64 and 1024, next to one host thread of the numpy model (tests/gif_model.py) on the same
frames -- a CPU reference rate of this repository's model, NOT Go's image/gif.

  python tools/bench_gif.py                      # the table, one JSON line per case
  python tools/bench_gif.py --profile            # a short run meant for rocprofv3 --kernel-trace --stats (kernel times per launch)
  python tools/bench_gif.py --quick              # 200x200 only, batches 1 and 64

Frames: 16 distinct seeded frames (noise over gradients, flat patches) repeated through the batch on the device."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frame(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 4), np.int64)
    f[..., 0] = xx * 255 // max(w - 1, 1)
    f[..., 1] = yy * 255 // max(h - 1, 1)
    f[..., 2] = (xx + yy) * 3 % 256
    f[..., :3] += rng.integers(-40, 41, (h, w, 3))
    f[h // 3:h // 2, w // 4:w // 2, :3] = 90
    f[..., 3] = 255
    return f.clip(0, 255).astype(np.uint8)


def device_batch(ctx, w, h, n):
    fb = w * h * 4
    buf = ctx.alloc(fb * n)
    distinct = [frame(w, h, s) for s in range(min(n, 16))]
    for i in range(n):
        if i < len(distinct):
            buf.upload(distinct[i], offset=i * fb)
        else:
            ctx.copy_d2d(buf.ptr + i * fb, buf.ptr + (i % len(distinct)) * fb, fb)
    ctx.device_sync()
    return buf, distinct


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=1, help="frames the numpy model codes per shape (0: skip)")
    a = ap.parse_args()
    import imageprocessor_amd as ipx
    if ipx.device_count() < 1:
        raise SystemExit("bench_gif: no GPU (this tool measures the device; there is no CPU fallback)")
    shapes = [(200, 200)] if a.quick else [(1024, 768), (200, 200)]
    batches = [1, 64] if a.quick else [1, 64, 1024]
    if a.profile:
        shapes, batches, a.reps, a.cpu_frames = [(1024, 768), (200, 200)], [1, 64], 2, 0
    with ipx.Context(device=0) as ctx:
        for w, h in shapes:
            cpu = None
            for n in batches:
                buf, distinct = device_batch(ctx, w, h, n)
                views, release = ctx.gif_encode_batch_dev(buf.ptr, w, h, n, copy=False)    # warm-up (code objects, pinned cache)
                total = sum(len(v) for v in views)
                release()
                times = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    views, release = ctx.gif_encode_batch_dev(buf.ptr, w, h, n, copy=False)   # returns once the streams are in host memory
                    times.append(time.perf_counter() - t0)
                    release()
                buf.free()
                t = float(np.median(times))
                if cpu is None and a.cpu_frames > 0:
                    import gif_model as gm
                    t0 = time.perf_counter()
                    for k in range(a.cpu_frames):
                        gm.encode(distinct[k % len(distinct)])
                    cpu = (time.perf_counter() - t0) / a.cpu_frames
                print(json.dumps({"bench": "gif_encode_batch_dev", "w": w, "h": h, "batch": n, "median_s": round(t, 5),
                                  "min_s": round(min(times), 5), "frames_per_s": round(n / t, 1), "ms_per_call": round(t * 1e3, 2),
                                  "stream_bytes_per_frame": total // n,
                                  "cpu_numpy_model_one_thread_s_per_frame_not_go": None if cpu is None else round(cpu, 3)}), flush=True)


if __name__ == "__main__":
    main()
