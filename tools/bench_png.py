"""png.Encode on the GPU: frames/s from frames resident in HBM to finished PNG streams in host memory (ipx_png_encode_batch_dev) at
1024x768 and 200x200 for batches of 1 and 1024, photo-like and flat content; then the PNG task's leg (ipx_plan_run_host_png) next to
ipx_plan_run_host (pixels back).  Beside each GPU rate: one host thread of libpng (Pillow, compress_level 6, the encoder
tools/bench_png_host.py times) on the same frame, and the stream's size next to zlib levels 1 and 6 on the same filtered rows.

  python tools/bench_png.py              # the table, one JSON line per case
  python tools/bench_png.py --quick      # 200x200 only, batch 1 and 64
  python tools/bench_png.py --profile    # a short run meant for rocprofv3 --kernel-trace --stats

Frames: 16 distinct seeded frames per content kind, repeated through the batch on the device."""
import argparse
import io
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frame(w, h, seed, kind):
    """the two contents of tools/bench_png_host.py (photograph-like: smooth fields plus sensor noise; flat graphics: 5-level tiles),
    phase-shifted by the seed"""
    yy, xx = np.mgrid[0:h, 0:w]
    xx = xx + 37 * seed
    if kind == "photo":
        img = np.stack([np.sin(xx / 40.0) * 90 + 128, np.cos(yy / 31.0) * 90 + 128, ((xx + 2 * yy) / 6.0) % 256], -1)
        img = (img + np.random.default_rng(seed).normal(0, 6, (h, w, 3))).clip(0, 255).astype(np.uint8)
    else:
        img = ((xx // 64 + yy // 64) % 5 * 50).astype(np.uint8)[..., None].repeat(3, -1)
    return np.concatenate([img, np.full((h, w, 1), 255, np.uint8)], -1)


def device_batch(ctx, w, h, n, kind):
    fb = w * h * 4
    buf = ctx.alloc(fb * n)
    distinct = [frame(w, h, s, kind) for s in range(min(n, 16))]
    for i in range(n):
        if i < len(distinct):
            buf.upload(distinct[i], offset=i * fb)
        else:
            ctx.copy_d2d(buf.ptr + i * fb, buf.ptr + (i % len(distinct)) * fb, fb)
    ctx.device_sync()
    return buf, distinct


def host_reference(f):
    """one thread: libpng (Pillow, level 6) seconds per frame; zlib 1 / 6 sizes of png.Encode's filtered rows"""
    from PIL import Image
    import png_model as pm
    img = Image.fromarray(np.ascontiguousarray(f[..., :3]))
    t0, k = time.perf_counter(), 0
    while time.perf_counter() - t0 < 1.0:
        img.save(io.BytesIO(), "PNG", compress_level=6)
        k += 1
    t = (time.perf_counter() - t0) / k
    data = pm.filtered_stream(f)[3].tobytes()
    return t, len(zlib.compress(data, 1)), len(zlib.compress(data, 6))


def timed(fn, reps):
    fn()   # warm-up: code objects, the pinned cache, stream-ordered pools
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import imageprocessor_amd as ipx
    if ipx.device_count() < 1:
        raise SystemExit("bench_png: no GPU (this tool measures the device; there is no CPU fallback)")
    shapes = [(200, 200)] if a.quick else [(1024, 768), (200, 200)]
    batches = [1, 64] if a.quick else [1, 1024]
    if a.profile:
        shapes, batches, a.reps = [(1024, 768)], [1, 64], 2
    with ipx.Context(device=0) as ctx:
        for w, h in shapes:
            for kind in ("photo", "flat"):
                ref = None if a.profile else host_reference(frame(w, h, 0, kind))
                for n in batches:
                    buf, _ = device_batch(ctx, w, h, n, kind)
                    sizes = []

                    def run():
                        views, release = ctx.png_encode_batch_dev(buf.ptr, w, h, n, copy=False)
                        sizes[:] = [len(views[0])]
                        release()
                    t, tmin = timed(run, a.reps)
                    buf.free()
                    print(json.dumps({"bench": "png_encode_batch_dev", "content": kind, "w": w, "h": h, "batch": n, "median_s": round(t, 5),
                                      "min_s": round(tmin, 5), "frames_per_s": round(n / t, 1),
                                      "host_libpng_l6_one_thread_frames_per_s": None if ref is None else round(1 / ref[0], 1),
                                      "stream_bytes": sizes[0], "zlib1_bytes": None if ref is None else ref[1],
                                      "zlib6_bytes": None if ref is None else ref[2]}), flush=True)
        # the PNG task's leg: 1280x720 uploads, resize 1024x768 + thumbnail 200 + watermark, batches of 64
        from helpers import DEFAULT_COL, text_glyphs
        sw, sh, n = 1280, 720, 8 if a.profile else 64
        frames = np.stack([frame(sw, sh, s, "photo") for s in range(n)])
        gs = ctx.glyphset(text_glyphs(sw, sh), DEFAULT_COL)
        plan = ctx.plan(sw, sh, resize=(1024, 768, True), thumbnail=(200, True), watermark=gs)
        t_png, _ = timed(lambda: plan.run_host_png(frames, copy=False), a.reps)
        t_pix, _ = timed(lambda: plan.run_host(frames), a.reps)
        print(json.dumps({"bench": "plan_run_host_png", "src": [sw, sh], "batch": n, "median_s": round(t_png, 4),
                          "frames_per_s": round(n / t_png, 1), "run_host_pixels_back_frames_per_s": round(n / t_pix, 1)}), flush=True)
        plan.close()
        gs.close()


if __name__ == "__main__":
    main()
