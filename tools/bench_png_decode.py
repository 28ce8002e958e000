"""png.Decode on the GPU: files/s of ipx_png_decode_batch (uploads in, frames of Go's type in HBM) at batches of 1, 64 and 1024, and of
the whole PNG-to-PNG leg (ipx_plan_run_png_png: uploads in, three PNG streams out) at batch 1024, at 200x200 and 1024x768 on seeded
corpora written by Pillow at its defaults (photo-like RGB, photo-like RGBA, flat 8-bit palette) and on the project's own encoder output
(ipx_png_encode_rgba8 of the photo-like RGB frames).  Beside each:
  * the host-decoded leg: Pillow decode (one thread) + the merged leg on its frames (ipx_plan_run_host_png, or run_host_nrgba /
    run_host_paletted + png.Encode of the outputs for the other kinds);
  * Pillow's decode of the same files in ms per file on ONE host thread, and in files/s on 16 threads -- a host rate, NOT Go's image/png.

  python tools/bench_png_decode.py               # the table, one JSON line per case
  python tools/bench_png_decode.py --profile     # a short run meant for rocprofv3 --kernel-trace --stats (kernel times per launch)
  python tools/bench_png_decode.py --quick       # 200x200 only, batches 1 and 64
  python tools/bench_png_decode.py --adam7       # the same corpora as Adam7 files (IPX_PNG_ADAM7=1 is set for the run): each file's
                                                 # samples re-wrapped by tests/png_adam7_corpus.py (Paeth rows, zlib level 6)
  python tools/bench_png_decode.py --par         # the parallel inflate (IPX_PNG_PAR=1 is set for the run); each row then carries the
                                                 # rise of ipx_png_decode_counts over its decode-only calls
  --shapes 1024x768 --corpora rgb,rgba --decode-only     # narrow a run: these sizes, these corpora, no PNG-to-PNG or host leg

Files: 16 distinct seeded files per corpus, repeated through the batch."""
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


def frames(w, h, corpus, seed):
    import png_corpus
    if corpus == "palette":
        return png_corpus.flat(h, w, 1, seed, 255).astype(np.uint8)[..., 0]
    c = 4 if corpus == "rgba" else 3
    f = png_corpus.photo(h, w, c, seed).astype(np.uint8)
    if c == 4:
        f[..., 3] = (f[..., 3] // 2 + 128).astype(np.uint8)
    return f


def pillow_png(a, corpus):
    from PIL import Image
    if corpus == "palette":
        im = Image.fromarray(a, "L").convert("P")
    else:
        im = Image.fromarray(a, "RGBA" if a.shape[2] == 4 else "RGB")
    b = io.BytesIO()
    im.save(b, "PNG")
    return b.getvalue()


def adam7_of(data):
    """the Adam7 file of a file's samples (Pillow cannot write one)"""
    import png_adam7_corpus
    im = pillow_decode(data)
    a = np.asarray(im)
    if im.mode == "P":
        return png_adam7_corpus.write(a[..., None], 3, 8, plte=np.asarray(im.getpalette(), np.uint8).reshape(-1, 3), filters=(4,))
    return png_adam7_corpus.write(a, {"RGB": 2, "RGBA": 6}[im.mode], 8, filters=(4,))


def pillow_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


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
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--adam7", action="store_true")
    ap.add_argument("--par", action="store_true")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--corpora", default="")
    ap.add_argument("--decode-only", action="store_true")
    a = ap.parse_args()
    if a.adam7:
        os.environ["IPX_PNG_ADAM7"] = "1"
    if a.par:
        os.environ["IPX_PNG_PAR"] = "1"
    import imageprocessor_amd as ipx
    import png_decode_model as dm
    if ipx.device_count() < 1:
        raise SystemExit("bench_png_decode: no GPU (this tool measures the device; there is no CPU fallback)")
    shapes = [(200, 200)] if a.quick else [(200, 200), (1024, 768)]
    batches = [1, 64] if a.quick else [1, 64, 1024]
    corpora = ["rgb", "rgba", "palette", "own"]
    if a.shapes:
        shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    if a.corpora:
        corpora = a.corpora.split(",")
    if a.profile:
        shapes, batches, a.reps, corpora = [(1024, 768)], [64], 1, ["rgb"]
    pool = cf.ThreadPoolExecutor(16)
    with ipx.Context(device=0) as ctx:
        for w, h in shapes:
            plan = ctx.plan(w, h, resize=(w // 2, h // 2, False), thumbnail=(64, True))
            for corpus in corpora:
                if corpus == "own":
                    distinct = [ctx.png_encode(np.concatenate([frames(w, h, "rgb", 9000 + s), np.full((h, w, 1), 255, np.uint8)], -1))
                                for s in range(16)]
                else:
                    distinct = [pillow_png(frames(w, h, corpus, 9000 + s), corpus) for s in range(16)]
                if a.adam7:
                    distinct = [adam7_of(f) for f in distinct]
                t0 = time.perf_counter()
                for f in distinct:
                    pillow_decode(f)
                pil_one = (time.perf_counter() - t0) / len(distinct)
                ref, st = ctx.png_decode_batch(distinct)    # the frames of the host-decoded leg (the decoder's own, tested elsewhere)
                assert st == [0] * len(distinct)
                kind = ref["kind"]
                for n in batches:
                    files = [distinct[i % len(distinct)] for i in range(n)]

                    def decode_only():
                        info, st = ctx.png_decode_batch(files, download=False)
                        info["free"]()
                        assert st.count(0) == n, st[:8]

                    before = ctx.png_decode_counts()
                    td = timed(decode_only, a.reps)
                    row = {"bench": "png_decode", "adam7": a.adam7, "par": a.par,
                           "par_counts_rose": [x - y for x, y in zip(ctx.png_decode_counts(), before)], "corpus": corpus, "kind": kind, "w": w, "h": h, "batch": n,
                           "bytes_per_file": sum(len(f) for f in distinct) // len(distinct),
                           "decode_ms": round(td * 1e3, 3), "decode_files_per_s": round(n / td, 1),
                           "pillow_one_thread_decode_ms_per_file_not_go": round(pil_one * 1e3, 3)}
                    if n == max(batches) and not a.decode_only:
                        t16 = timed(lambda: list(pool.map(pillow_decode, files)), 1)
                        row["pillow_16_threads_files_per_s_not_go"] = round(n / t16, 1)

                        def png_png():
                            _, st = plan.run_png_png(files, copy=False)
                            assert st.count(0) == n

                        pix = ref["pix"][[i % len(distinct) for i in range(n)]]
                        pal = ref["palettes"][[i % len(distinct) for i in range(n)]] if kind == dm.PALETTED else None

                        def host_leg():
                            for f in files:        # the host decode this leg needs, one thread
                                pillow_decode(f)
                            if kind == dm.RGBA:
                                plan.run_host_png(pix.reshape(n, h, w, 4), copy=False)
                                return
                            out = plan.run_host_nrgba(pix.reshape(n, h, w, 4)) if kind == dm.NRGBA else plan.run_host_paletted(pix, pal)
                            for v in out.values():
                                for fr in v:
                                    ctx.png_encode(fr)

                        tg = timed(png_png, a.reps)
                        th = timed(host_leg, 1)
                        row.update(png_png_ms=round(tg * 1e3, 3), png_png_files_per_s=round(n / tg, 1),
                                   host_decoded_leg_files_per_s=round(n / th, 1))
                    print(json.dumps(row), flush=True)
            plan.close()
    pool.shutdown()


if __name__ == "__main__":
    main()
