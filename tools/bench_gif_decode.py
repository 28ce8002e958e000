"""gif.Decode on the GPU: files/s of ipx_gif_decode_batch (uploads in, paletted frames in HBM) and of the whole GIF-to-GIF leg
(ipx_plan_run_gif_gif: uploads in, resize / thumbnail GIF streams and the watermark JPEG stream out), at 200x200 and 1024x768 for
batches of 1, 64 and 1024, on seeded photo-like and flat-graphics GIFs written by Pillow.  Beside each:
  * Pillow's decode of the same files on ONE host thread -- a host rate, NOT Go's image/gif;
  * the merged leg fed with host-decoded frames: Pillow decode + ipx_plan_run_host_paletted_gif.

  python tools/bench_gif_decode.py               # the table, one JSON line per case
  python tools/bench_gif_decode.py --profile     # a short run meant for rocprofv3 --kernel-trace --stats (kernel times per launch)
  python tools/bench_gif_decode.py --quick       # 200x200 only, batches 1 and 64
  python tools/bench_gif_decode.py --par         # the parallel code walk (IPX_GIF_PAR=1 is set for the run); each row then carries the
                                                 # rise of ipx_gif_decode_counts over its decode-only calls
  python tools/bench_gif_decode.py --no-host     # without the host-decoded leg beside each row

Files: 16 distinct seeded files per kind, repeated through the batch."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pillow_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    idx = np.array(im)
    pal = np.zeros((256, 4), np.uint8)
    p = np.array(im.getpalette()[:768], np.uint8).reshape(-1, 3)
    pal[:len(p), :3] = p
    pal[:len(p), 3] = 255
    if "transparency" in im.info:
        pal[im.info["transparency"]] = 0
    return idx, pal


def timed(fn, reps):
    fn()                                         # warm-up (code objects, pinned cache)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--par", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if a.par:
        os.environ["IPX_GIF_PAR"] = "1"
    else:
        os.environ.pop("IPX_GIF_PAR", None)
    import gif_corpus
    import imageprocessor_amd as ipx
    if ipx.device_count() < 1:
        raise SystemExit("bench_gif_decode: no GPU (this tool measures the device; there is no CPU fallback)")
    shapes = [(200, 200)] if a.quick else [(200, 200), (1024, 768)]
    batches = [1, 64] if a.quick else [1, 64, 1024]
    kinds = ["photo", "flat"]
    if a.profile:
        shapes, batches, a.reps, kinds = [(200, 200), (1024, 768)], [1, 64], 2, ["photo"]
    with ipx.Context(device=0) as ctx:
        for w, h in shapes:
            plan = ctx.plan(w, h, resize=(w // 2, h // 2, False), thumbnail=(64, True))
            for kind in kinds:
                distinct = [gif_corpus.make(w, h, 9000 + s, kind, ncol=256, interlace=False) for s in range(16)]
                t0 = time.perf_counter()
                decoded = [pillow_decode(f) for f in distinct]
                host_dec = (time.perf_counter() - t0) / len(distinct)
                for n in batches:
                    files = [distinct[i % len(distinct)] for i in range(n)]

                    def decode_only():
                        info, st = ctx.gif_decode_batch(files, download=False)
                        info["free"]()
                        assert st.count(0) == n

                    def gif_gif():
                        _, st = plan.run_gif_gif(files, copy=False)
                        assert st.count(0) == n

                    idx = np.stack([decoded[i % len(distinct)][0] for i in range(n)])
                    pal = np.stack([decoded[i % len(distinct)][1] for i in range(n)])

                    def host_leg():
                        for f in files:            # the host decode this leg needs, one thread
                            pillow_decode(f)
                        plan.run_host_paletted_gif(idx, pal, copy=False)

                    before = ctx.gif_decode_counts()
                    td, tdm, tdx = timed(decode_only, a.reps)
                    rose = [x - y for x, y in zip(ctx.gif_decode_counts(), before)]
                    tg, tgm, tgx = timed(gif_gif, a.reps)
                    th = None if a.no_host else timed(host_leg, 1 if n >= 1024 else a.reps)[0]
                    print(json.dumps({"bench": "gif_decode", "par": a.par, "par_counts_rose": rose, "kind": kind, "w": w, "h": h, "batch": n,
                                      "bytes_per_file": sum(len(f) for f in distinct) // len(distinct),
                                      "decode_ms": round(td * 1e3, 3), "decode_ms_min_max": [round(tdm * 1e3, 3), round(tdx * 1e3, 3)],
                                      "decode_files_per_s": round(n / td, 1),
                                      "gif_gif_ms": round(tg * 1e3, 3), "gif_gif_ms_min_max": [round(tgm * 1e3, 3), round(tgx * 1e3, 3)],
                                      "gif_gif_files_per_s": round(n / tg, 1),
                                      "host_decoded_leg_files_per_s": None if th is None else round(n / th, 1),
                                      "pillow_one_thread_decode_ms_per_file_not_go": round(host_dec * 1e3, 3)}), flush=True)
            plan.close()


if __name__ == "__main__":
    main()
