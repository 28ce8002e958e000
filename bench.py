#!/usr/bin/env python3
"""bench.py -- images/sec through resize + thumbnail + watermark on a batch of 1920x1080 RGBA
frames resident in HBM (BASELINE.json configs[2]; --workload resize gives configs[1]).

One process per GPU.  For N > 1 the driver launches this file under torch.distributed.run; the
frames are independent, so every rank runs the same batch size on its own GPU with no data-path
collective (weak scaling) and torch.distributed (gloo, CPU tensors) only carries the barrier and
the max-over-ranks of the timed region.

A "step" is one pass of the hot path over the whole batch (one fused launch).  Prints ONE JSON
line on rank 0: `value` is the HBM-resident rate; `roofline` comes from HIP events on the stream
the kernel runs on.  A plain run does no more than that line needs: set up, warm up, time the steps.

--full adds everything else the benchmark measures or checks, after the timed steps: the check of
what was timed against the CPU oracle (`checked`), the plain-copy ceiling beside the roofline
(`roofline.copy_ceiling`), `cpu_baseline` (the CPU oracle on a time-bounded sample) and `e2e` (the
PCIe-inclusive legs: pinned host memory in and out, JPEG in and out -- reported, never `value`).
Without it `checked` is false and the other three are absent or null.

--mixed N runs BASELINE config 5 instead (mixed 480p-8K sizes, pull scheduling).

--dump-outputs DIR writes what the last timed step computed (rank 0) as float32 .npy files, one per output (resize.npy,
thumbnail.npy, watermark.npy), so that two builds can be compared output for output: see dump_outputs().
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is achievable


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1024, help="frames per GPU per step")
    ap.add_argument("--workload", choices=["full", "resize", "full-keepaspect", "wm", "thumb", "resize-wm"], default="full")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pool", type=int, default=32, help="distinct seeded frames tiled over the batch")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run what the headline figure does not need: the check against the CPU oracle, "
                         "the plain-copy ceiling, the CPU baseline and the PCIe-inclusive legs (--cpu-seconds, --copy-gib, --e2e-frames "
                         "and --e2e-reps size them)")
    ap.add_argument("--cpu-seconds", type=float, default=6.0, help="with --full: seconds per row of the CPU baseline (0 = skip)")
    ap.add_argument("--sets", type=int, default=3, help="buffer sets the steps rotate over (the run time depends on where buffers land: DESIGN.md 4)")
    ap.add_argument("--copy-gib", type=int, default=4, help="with --full: size of the plain-copy ceiling measurement beside the roofline (0 = skip; N = 1 only)")
    ap.add_argument("--e2e-frames", type=int, default=256, help="with --full: frames per call of the PCIe-inclusive legs (0 = skip; N = 1 only)")
    ap.add_argument("--e2e-reps", type=int, default=4, help="with --full: timed calls per PCIe-inclusive leg")
    ap.add_argument("--check", action="store_true", help="check what was timed against the CPU oracle as --full does, on --pool more slots (also without --full)")
    ap.add_argument("--mixed", type=int, default=0, metavar="N",
                    help="BASELINE config 5 instead: N frames per GPU of mixed sizes (480p-8K, seed 0x51), full "
                         "pipeline, pull scheduling over a shared largest-first queue (work stealing across ranks)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last step to DIR/<output>.npy (float32, a fixed seeded "
                         "sample of the batch, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.mixed:
        ap.error("--dump-outputs covers the default path, not --mixed")
    return args


def dump_outputs(dirname, F, outputs, seed=0xD0, max_slots=8, max_pixels=1 << 17):
    """outputs: [(name, device buffer, frame stride in bytes, (h, w, 4))] of the last timed step -> dirname/<name>.npy, float32.

    A fixed seeded sample, the same for the same arguments: slots 0 and F - 1 and up to max_slots - 2 others (all F when F <=
    max_slots); of each frame, every pixel when it has at most max_pixels, else the same max_pixels positions (row-major order) in
    every slot.  Arrays are slots x h x w x 4 (whole frames) or slots x max_pixels x 4 (sampled); at most 50.3 MB in all."""
    import numpy as np
    rng = np.random.default_rng(seed)
    if F <= max_slots:
        slots = np.arange(F)
    else:
        slots = np.sort(np.concatenate(([0, F - 1], rng.choice(np.arange(1, F - 1), max_slots - 2, replace=False))))
    os.makedirs(dirname, exist_ok=True)
    for name, buf, stride, shape in outputs:
        npx = shape[0] * shape[1]
        pick = None if npx <= max_pixels else np.sort(rng.choice(npx, max_pixels, replace=False))
        frames = []
        for slot in slots:
            f = buf.download(shape, offset=int(slot) * stride)
            frames.append(f if pick is None else f.reshape(npx, 4)[pick])
        np.save(os.path.join(dirname, name + ".npy"), np.stack(frames).astype(np.float32))


def copy_ceiling(ctx, gib=4, pairs=3, reps=4):
    """What a plain streaming copy reaches on THIS box, in this process: the practical ceiling the band kernels are held against next to
    the 8 TB/s of the data sheet.  It differs from box to box (4.9 .. 5.9 TB/s seen) and by some 8% with where the two buffers happen to
    land (profiles/r02_ubench_place.txt), so a few pairs of buffers are tried and the best and the worst are reported."""
    nbytes = gib << 30
    rates, keep = [], []
    for _ in range(pairs):
        a, b = ctx.alloc(nbytes), ctx.alloc(nbytes)
        keep += [a, b]
        ctx.stream_copy(b.ptr, a.ptr, nbytes)
        ctx.device_sync()
        ms = min(ctx.timed(lambda: ctx.stream_copy(b.ptr, a.ptr, nbytes)) for _ in range(reps))
        rates.append(2.0 * nbytes / (ms * 1e-3) / 1e9)
    for b in keep:
        b.free()
    return {"best": round(max(rates), 1), "worst": round(min(rates), 1), "unit": "GB/s",
            "what": "ipx_stream_copy (uint4 copy kernel, 2048 contiguous streams) of %d GiB, read + written bytes / best of %d runs, %d buffer pairs" % (gib, reps, pairs)}


def host_info():
    """What the CPU rows ran on: model string, logical CPUs of the node, CPUs this process may use."""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    usable = len(os.sched_getaffinity(0))
    try:   # a cgroup CPU quota bounds what the threads can really get
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()
            if q != "max":
                usable = max(1, min(usable, int(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    return {"cpu_model": model, "nproc": os.cpu_count(), "usable_cpus": usable}


def timed_pool(fn, threads, seconds, limit=None):
    """threads workers call fn(i) for i = 0, 1, 2, ... until `seconds` have passed (or `limit` calls were started); every started call
    is finished and counted.  -> (calls, wall seconds)"""
    import itertools
    import threading
    counter = itertools.count()
    lock = threading.Lock()
    done = [0]
    t0 = time.perf_counter()
    deadline = t0 + seconds

    def work():
        while time.perf_counter() < deadline:
            with lock:
                i = next(counter)
            if limit is not None and i >= limit:
                return
            fn(i)
            with lock:
                done[0] += 1
    ts = [threading.Thread(target=work) for _ in range(threads)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    return done[0], time.perf_counter() - t0


def cpu_rows(one, seconds, what):
    """The CPU oracle (scalar C restatement of the reference's loops; one frame per thread, as Go's loops are single-threaded per
    image) on a time-bounded sample of the same workload: once on every usable CPU, once at the reference's deployed concurrency of 3
    goroutines (.env.example:38, worker.go:90)."""
    hi = host_info()
    threads = max(1, min(hi["usable_cpus"], 64))
    one(0)  # warm: page in the library
    n_all, dt_all = timed_pool(one, threads, seconds)
    n3, dt3 = timed_pool(one, 3, seconds)
    return {"value": round(n_all / dt_all, 2), "unit": "images/sec", "cores": threads, "kind": "port",
            "sample": "%d frames of %s through oracle/ipx_oracle.c (C restatement of the Go loops, gcc -O2, no FMA) in %.1f s on %d "
                      "threads, one frame per thread; then %d frames in %.1f s on 3 threads" % (n_all, what, dt_all, threads, n3, dt3),
            "threads": threads, "nproc": hi["nproc"], "usable_cpus": hi["usable_cpus"], "cpu_model": hi["cpu_model"],
            "at_reference_concurrency_3": round(n3 / dt3, 2), "seconds_per_row": [round(dt_all, 2), round(dt3, 2)]}


def cpu_baseline(pool, glyphs, col, resize, thumb, want, seconds):
    import oracle

    def one(i):
        oracle.process(pool[i % len(pool)], resize=resize or (1, 1, False), thumb=thumb or (1, False),
                       glyphs=glyphs, col=col, want=want)
    return cpu_rows(one, seconds, "the same workload (seeded %dx%d frames)" % (pool.shape[2], pool.shape[1]))


def run_mixed(args, ipx, shard, rank, local_rank, world):
    """Config 5: args.mixed frames per GPU, sizes drawn uniformly from six (854x480 ... 7680x4320, seed 0x51), full pipeline with the
    product-default keep_aspect=true.  Every rank holds one plan, one pool of source frames and two sets of outputs per size in HBM
    (shard.MixedBatch); work items are chunks of equal-size frames (~1 GiB of source, at most 128 frames: an 8K chunk of 2 frames fills half
    the chip, one of 8 all of it -- 42 k images/s with 256 MB chunks, 51 k with 1 GiB), ordered largest first and claimed with an
    atomic counter in the rendezvous store, so a rank that finishes early claims more (work stealing).  A rank keeps two chunks in
    flight on two streams: the next chunk is claimed and launched while the previous one runs.  A step = one pass over the batch."""
    import ctypes
    import numpy as np
    import torch.distributed as dist
    from helpers import DEFAULT_COL, rgba_frames, text_glyphs
    sizes = shard.MIXED_SIZES
    rng = np.random.default_rng(0x51)
    total = args.mixed * world
    draw = [int(v) for v in rng.integers(0, len(sizes), total)]
    ctx = ipx.Context(device=local_rank % max(1, ipx.device_count()))
    L = ipx.lib()

    def make_frames(si, w, h, k):
        return rgba_frames(k, w, h, seed=0x1F00D + si)
    mb = shard.MixedBatch(ctx, make_frames, text_glyphs, DEFAULT_COL, resize=(1024, 768, True), thumbnail=(200, True),
                          chunk_bytes=int(os.environ.get("IPX_MIXED_CHUNK_MB", "1024")) << 20, max_chunk=int(os.environ.get("IPX_MIXED_MAX_CHUNK", "128")))
    items = mb.items_for(draw)
    store = shard.default_store()

    def ev():
        return L.ipx_event_create(ctx.handle)

    def elapsed(e0, e1):
        ms = ctypes.c_float()
        L.ipx_event_elapsed_ms(ctx.handle, e0, e1, ctypes.byref(ms))
        return ms.value

    # every plan once on every stream (first-launch costs), then each size alone: full chunks back to back on one stream give the
    # uniform rate of that size, from which the byte-weighted expectation for this mix follows
    for si in range(len(sizes)):
        for k in range(len(mb.streams)):
            mb.launch(si, 1, k)
    ctx.device_sync()
    uniform_ms = []
    for si in range(len(sizes)):
        reps = 3
        e0, e1 = ev(), ev()
        mb.launch(si, mb.chunk_of[si], 0)
        L.ipx_event_record(ctx.handle, e0, mb.streams[0])
        for _ in range(reps):
            mb.launch(si, mb.chunk_of[si], 0)
        L.ipx_event_record(ctx.handle, e1, mb.streams[0])
        uniform_ms.append(elapsed(e0, e1) / reps / mb.chunk_of[si])        # ms per frame of this size, uniform batch
        L.ipx_event_destroy(ctx.handle, e0)
        L.ipx_event_destroy(ctx.handle, e1)
    for w_ in range(args.warmup):
        mb.run(items, shard.WorkQueue(len(items), chunk=1, key="ipx_mixed_w%d" % w_, store=store))
    ctx.device_sync()
    if world > 1:
        dist.barrier()
    K = args.steps
    e_start = ev()
    e_end = [ev() for _ in mb.streams]
    t0 = time.perf_counter()
    L.ipx_event_record(ctx.handle, e_start, mb.streams[0])
    mine = alg = 0
    for k in range(K):
        f_, a_ = mb.run(items, shard.WorkQueue(len(items), chunk=1, key="ipx_mixed_%d" % k, store=store))
        mine += f_
        alg += a_
    for st, e in zip(mb.streams, e_end):
        L.ipx_event_record(ctx.handle, e, st)
    ctx.device_sync()
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    dev_ms = max(elapsed(e_start, e) for e in e_end)      # device timeline of this rank: first launch -> last completion
    frames_done, wall_max = shard.aggregate(mine, wall)
    counts = [mine]
    if world > 1:
        import torch
        t = torch.zeros(world, dtype=torch.int64)
        t[rank] = mine
        dist.all_reduce(t)
        counts = t.tolist()
    if rank == 0:
        achieved = alg / (dev_ms * 1e-3) / 1e9
        expect_ms = sum(uniform_ms[si] for si in draw) * K / world      # the same frames as uniform batches, one size after the other
        out = {
            "metric": "images/sec (resize+thumb+watermark) on mixed-size batch (480p-8K), work stealing",
            "value": round(frames_done / wall_max, 1), "unit": "images/sec", "n_gpus": world, "steps": K, "warmup": args.warmup,
            "ms_per_step": round(wall_max / K * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32+f64",
            "data": "synthetic: one seeded opaque RGBA8 frame per size tiled over each chunk, resident in HBM",
            "config": {"workload": "%d frames per step of sizes %s drawn uniformly (seed 0x51), full pipeline keep_aspect=true (BASELINE config 5)"
                                   % (total, sizes), "items_per_step": len(items), "frames_per_rank": counts,
                       "sharding": "pull scheduling, largest first, atomic counter in the store; two chunks in flight per rank"},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
                         "kernel": "ks_fused_kernel (float pass + exact pass), one launch group per chunk of equal-size frames",
                         "algorithmic_bytes": alg,
                         "basis": "sum of algorithmic bytes of the frames rank 0 processed / rank 0's device timeline from the first launch "
                                  "to the last completion (HIP events on the two streams the kernels run on): %.3f ms" % dev_ms,
                         "uniform_ms_per_frame": {"%dx%d" % sizes[si]: round(uniform_ms[si], 5) for si in range(len(sizes))},
                         "vs_byte_weighted_uniform": round(expect_ms / (wall_max * 1e3), 4)},
        }
        if args.full and world == 1 and args.cpu_seconds > 0:
            import oracle
            pools = [mb.pool[si][0] for si in range(len(sizes))]
            glyphs = mb.glyphs

            def one(i):
                si = draw[i % len(draw)]
                oracle.process(pools[si], resize=(1024, 768, True), thumb=(200, True), glyphs=glyphs[si], col=DEFAULT_COL)
            out["cpu_baseline"] = cpu_rows(one, args.cpu_seconds, "the same mix (sizes in the order of the seeded draw)")
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    mb.close()
    ctx.close()


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the ranks as children (no exec after
    GPU init: nothing here has touched the GPU yet)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", os.environ.get("MASTER_PORT", "29533"),
           os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


def photo_like(n, sw, sh):
    """n x sh x sw x 4 opaque frames with photograph-like content (smooth gradients + mild texture): noise frames would make the JPEG
    streams of the codec legs unrealistically large"""
    import numpy as np
    yy, xx = np.mgrid[0:sh, 0:sw]
    out = np.empty((n, sh, sw, 4), np.uint8)
    for k in range(n):
        base = np.stack([np.sin(xx / (40.0 + 7 * k)) * 90 + 128, np.cos(yy / (31.0 + 5 * k)) * 90 + 128, ((xx + 2 * yy) / 6.0 + 40 * k) % 256], -1)
        out[k, ..., :3] = (base + np.random.default_rng(k).normal(0, 6, (sh, sw, 3))).clip(0, 255)
        out[k, ..., 3] = 255
    return out


def e2e_legs(ipx, device, n, sw, sh, resize, reps, lanes=5):
    """The PCIe-inclusive legs of the north star's pipeline (decode -> H2D -> kernel -> D2H -> encode) on the same workload, through the
    synchronous host entries of the ABI: n frames in pinned host memory per call, chunks pipelined over `lanes` streams.  Never
    `value`: these are bound by the link, not by HBM.  Every repetition is reported, not the best."""
    from helpers import DEFAULT_COL, text_glyphs
    pool = photo_like(4, sw, sh)
    # the pool first, while the process holds no other context (an idle second one costs it 12 %: DESIGN.md section 5)
    pool_result = pool_leg(ipx, n, sw, sh, resize, reps, pool)
    ctx = ipx.Context(device=device, lanes=lanes, lane_bytes=1 << 30)
    gs = ctx.glyphset(text_glyphs(sw, sh), DEFAULT_COL)
    plan = ctx.plan(sw, sh, resize=resize, thumbnail=(200, True), watermark=gs)
    i = plan.info
    src = ctx.host_alloc((n, sh, sw, 4))
    for k in range(n):
        src[k] = pool[k % 4]
    outs = {"resize": ctx.host_alloc((n, i.resize_h, i.resize_w, 4)), "thumbnail": ctx.host_alloc((n, i.thumb_h, i.thumb_w, 4)),
            "watermark": ctx.host_alloc((n, i.wm_h, i.wm_w, 4))}
    up = sw * sh * 4
    down = i.resize_bytes + i.thumb_bytes + i.wm_bytes
    legs = {}
    # what the link gives pinned copies on this box, with the byte mix of a pixels-to-pixels call (8.3 MB up : 11.6 MB down per frame)
    link = ctx.link_probe(64 * up, 64 * down, 3)

    def leg(name, call, up_b, down_b, note):
        call()     # warm: lane buffers, pinned blocks
        ms = []
        res = None
        for _ in range(reps):
            t0 = time.perf_counter()
            res = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        mean = sum(ms) / len(ms)
        d = down_b(res) if callable(down_b) else down_b
        h2d, d2h = n * up_b / (mean * 1e-3) / 1e9, n * d / (mean * 1e-3) / 1e9
        # the least time the link needs for the call's bytes (each direction alone at its rate, both together at their summed rate when
        # they run side by side) over the time the call took: 1.0 = the call costs what its copies alone cost on this box
        t_link = max(n * up_b / (link["up"] * 1e9), n * d / (link["down"] * 1e9),
                     n * (up_b + d) / ((link["up_while_down"] + link["down_while_up"]) * 1e9))
        frac = t_link / (mean * 1e-3)
        legs[name] = {"images_per_s": round(n / (mean * 1e-3), 1), "ms_per_call": [round(v, 2) for v in ms], "frames_per_call": n,
                      "h2d_GBps": round(h2d, 2), "d2h_GBps": round(d2h, 2), "frac_of_link": round(frac, 3),
                      "bytes_up_per_image": int(up_b), "bytes_down_per_image": int(d), "what": note}
        return res

    leg("pixels_to_pixels", lambda: plan.run_host(src, out=outs), up, down,
        "ipx_plan_run_host: RGBA8 frames in, the three RGBA8 outputs back")
    leg("pixels_to_jpeg", lambda: plan.run_host_jpeg(src, 85, copy=False), up,
        lambda r: sum(sum(v) for v in r.values()) / n,
        "ipx_plan_run_host_jpeg: RGBA8 frames in, operators + jpeg.Encode(q85) on the GPU, three streams back")
    files = [ctx.jpeg_encode(pool[k], 85) for k in range(4)]       # Go-layout baseline 4:2:0 streams, made by the GPU encoder
    batch = [files[k % 4] for k in range(n)]

    def j2j():
        r, st = plan.run_jpeg_jpeg(batch, 85, copy=False)
        assert not any(st), st
        return r
    leg("jpeg_to_jpeg", j2j, sum(len(f) for f in files) / 4.0, lambda r: sum(sum(v) for v in r.values()) / n,
        "ipx_plan_run_jpeg_jpeg: JPEG files in, image.Decode + operators + jpeg.Encode on the GPU, three streams back")
    ctx.host_free(src)
    for a in outs.values():
        ctx.host_free(a)
    plan.close()
    gs.close()
    ctx.close()
    legs["pool_pixels_to_pixels"] = pool_result
    return {"workload": "%d x %dx%d per call, photograph-like frames, %d lanes, pinned host memory" % (n, sw, sh, lanes),
            "link_GBps": dict(link, what="ipx_link_probe: 64 frames' worth of pinned memory up (8.3 MB each) and down (11.6 MB each), alone and at once, best of 3; copies in 32 MiB pieces, one stream per direction; at once = the better of copy engine / kernel stores for the way down"),
            "legs": legs}


def pool_leg(ipx, n, sw, sh, resize, reps, frames4):
    """The product's own multi-device path: ONE process, ipx_pool_create over every visible device, the batch as one pixel job per device
    through the job API (what a Go worker binds; on an 8-GPU node this leg is the 8-GPU run).  Frames and outputs in pinned memory next
    to each slot's GPU."""
    from helpers import DEFAULT_COL, text_glyphs
    ndev = max(1, ipx.device_count())
    glyphs = text_glyphs(sw, sh)
    tmp = ipx.Context(device=0)                           # (the output sizes; gone before the pool exists)
    info = tmp.plan(sw, sh, resize=resize, thumbnail=(200, True), watermark=True).info
    rb, tb = (info.resize_h, info.resize_w, 4), (info.thumb_h, info.thumb_w, 4)
    tmp.close()
    with ipx.Pool(devices=tuple(range(ndev))) as pool:
        per = (n + ndev - 1) // ndev
        jobs, keep = [], []
        for d in range(ndev):
            src = pool.host_alloc(d, (per, sh, sw, 4))
            for k in range(per):
                src[k] = frames4[k % 4]
            outs = (pool.host_alloc(d, (per,) + rb), pool.host_alloc(d, (per,) + tb), pool.host_alloc(d, (per, sh, sw, 4)))
            keep.append((src,) + outs)
            jobs.append(dict(frames=src, resize=resize, thumbnail=(200, True), glyphs=glyphs, col=DEFAULT_COL, out=dict(resize=outs[0], thumbnail=outs[1], watermark=outs[2])))
        def run():
            tickets = [pool.submit(j["frames"], resize=j["resize"], thumbnail=j["thumbnail"], glyphs=j["glyphs"], col=j["col"], out=j["out"]) for j in jobs]
            for t in tickets:
                t.wait()
        run()                                                 # warm: plans, glyph sets, lane buffers
        before = [pool.frames_done(sl) for sl in range(pool.slots())]
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            ms.append((time.perf_counter() - t0) * 1e3)
        done = [pool.frames_done(sl) - b for sl, b in zip(range(pool.slots()), before)]
        for arrs in keep:
            for a in arrs:
                pool.host_free(a)
    mean = sum(ms) / len(ms)
    return {"images_per_s": round(per * ndev / (mean * 1e-3), 1), "ms_per_call": [round(v, 2) for v in ms], "frames_per_call": per * ndev, "devices": ndev,
            "frames_done_per_slot": done, "what": "ipx_pool_* / ipx_job_submit + ipx_job_wait: one process, one context per visible device, one largest-first queue; RGBA8 frames in, the three RGBA8 outputs back"}


def main():
    args = parse()
    if args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        self_launch(args)

    import numpy as np
    import imageprocessor_amd as ipx
    from imageprocessor_amd import shard
    from helpers import DEFAULT_COL, rgba_frames, text_glyphs

    # one process per GPU; gloo carries the barrier and the max-over-ranks only (no data-path collective)
    rank, local_rank, world = shard.init_from_env()
    if args.mixed:
        return run_mixed(args, ipx, shard, rank, local_rank, world)
    dist = None
    if world > 1:
        import torch.distributed as dist

    sw, sh, F = args.width, args.height, args.frames
    resize = {"full": (1024, 768, False), "resize": (1024, 768, False), "full-keepaspect": (1024, 768, True),
              "wm": None, "thumb": None, "resize-wm": (1024, 768, False)}[args.workload]
    thumb = None if args.workload in ("resize", "wm", "resize-wm") else (200, True)
    do_wm = args.workload not in ("resize", "thumb")

    ctx = ipx.Context(device=local_rank % max(1, ipx.device_count()))
    glyphs = text_glyphs(sw, sh) if do_wm else []
    gs = ctx.glyphset(glyphs, DEFAULT_COL) if do_wm else None
    plan = ctx.plan(sw, sh, resize=resize, thumbnail=thumb, watermark=gs)
    info = plan.info

    # synthetic batch: `pool` seeded opaque frames (seed 0x1F00D + rank), tiled over F slots in HBM
    P = min(args.pool, F)
    pool = rgba_frames(P, sw, sh, seed=0x1F00D + rank)
    fbytes = sw * sh * 4
    # experiment switch: IPX_BENCH_PAD=bytes widens the OUTPUT frame strides (a 1024x768 frame is exactly 3 MiB)
    pad = int(os.environ.get("IPX_BENCH_PAD", "0"))
    # The batch lives in `--sets` buffer sets (same content) and the steps rotate over them: a launch runs 8 % faster or slower with where
    # its buffers happen to land (so does a plain copy: profiles/r02_ubench_place.txt), and one set per process made the line a draw
    # from that spread.  Every step is still one pass over one resident batch.
    nsets = max(1, min(args.sets, args.steps))
    sets = []
    for _ in range(nsets):
        src = ctx.alloc(F * fbytes)
        if sets:
            ctx.copy_d2d(src.ptr, sets[0][0].ptr, F * fbytes)
        else:
            src.upload(pool)
            for i in range(P, F, P):
                m = min(P, F - i)
                ctx.copy_d2d(src.ptr + i * fbytes, src.ptr, m * fbytes)
        res = ctx.alloc(F * (info.resize_bytes + pad)) if info.resize_bytes else None
        th = ctx.alloc(F * (info.thumb_bytes + pad)) if info.thumb_bytes else None
        wm = ctx.alloc(F * info.wm_bytes) if info.wm_bytes else None
        sets.append((src, res, th, wm))
    src, res, th, wm = sets[0]
    turn = [0]

    def step():
        s_, r_, t_, w_ = sets[turn[0] % nsets]
        turn[0] += 1
        plan.run_dev(F, s_.ptr, r_.ptr if r_ else None, t_.ptr if t_ else None, w_.ptr if w_ else None,
                     resize_frame_stride=info.resize_bytes + pad, thumb_frame_stride=info.thumb_bytes + pad)

    L = ipx.lib()
    for _ in range(max(args.warmup, nsets)):      # (every set at least once before the clock starts)
        step()
    ctx.device_sync()
    turn[0] = 0
    if dist:
        dist.barrier()
    K = args.steps
    evs = [(L.ipx_event_create(ctx.handle), L.ipx_event_create(ctx.handle)) for _ in range(K)]
    t0 = time.perf_counter()
    for k in range(K):
        L.ipx_event_record(ctx.handle, evs[k][0], None)   # HIP events on the stream the kernel runs on
        step()
        L.ipx_event_record(ctx.handle, evs[k][1], None)
    ctx.device_sync()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    import ctypes
    launch_ms = []
    for e0, e1 in evs:
        ms = ctypes.c_float()
        L.ipx_event_elapsed_ms(ctx.handle, e0, e1, ctypes.byref(ms))
        launch_ms.append(ms.value)
        L.ipx_event_destroy(ctx.handle, e0)
        L.ipx_event_destroy(ctx.handle, e1)
    frames_done, elapsed = shard.aggregate(F * K, elapsed)   # frames summed over ranks, time = max over ranks

    # --full (or --check) checks what was timed: frames 0, P - 1 and F - 1 of the last buffer set (slot i holds pool frame i % P) against
    # the CPU oracle, every byte of every output.  The oracle is the checker here, never the thing measured.  --check adds P more slots.
    checked = None
    if rank == 0:
        s_, r_, t_, w_ = sets[(turn[0] - 1) % nsets]
        rstride, tstride = info.resize_bytes + pad, info.thumb_bytes + pad
        outputs = [(key, buf, stride, shape) for key, buf, stride, shape in (
            ("resize", r_, rstride, (info.resize_h, info.resize_w, 4)), ("thumbnail", t_, tstride, (info.thumb_h, info.thumb_w, 4)),
            ("watermark", w_, info.wm_bytes, (sh, sw, 4))) if buf]
        checked = False
        if args.full or args.check:
            import oracle
            slots = sorted({0, min(P, F) - 1, F - 1} | (set(range(min(P, F), min(2 * P, F))) if args.check else set()))
            for slot in slots:
                want = oracle.process(pool[slot % P], resize=resize or (1, 1, False), thumb=thumb or (1, False), glyphs=glyphs, col=DEFAULT_COL,
                                      want=[key for key, _, _, _ in outputs])
                for key, buf, stride, shape in outputs:
                    if not np.array_equal(buf.download(shape, offset=slot * stride), want[key]):
                        raise SystemExit("bench.py: %s of slot %d differs from the oracle" % (key, slot))
            checked = True
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, F, outputs)

    if rank == 0 and os.environ.get("IPX_BENCH_TRACE"):
        print("launch_ms:", " ".join("%.3f" % m for m in launch_ms), file=sys.stderr)
    if rank == 0:
        avg_ms = sum(launch_ms) / len(launch_ms)
        alg = info.algorithmic_bytes * F  # source read once + each output written once
        achieved = alg / (avg_ms * 1e-3) / 1e9
        # HBM bytes per launch from the PMC counters cannot be collected inside this process: they come from the separate
        # rocprofv3 --pmc passes whose summaries are committed under profiles/ (another session, possibly another box)
        traffic, traffic_src = None, None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tpath):
            try:
                with open(tpath) as f:
                    tj = json.load(f)
                key = "%s_%dx%d_%d" % (args.workload, sw, sh, F)
                traffic = tj.get(key, {}).get("hbm_bytes_per_launch")
                if traffic is not None:
                    traffic_src = "profiles/pmc_traffic.json[%s]: rocprofv3 --pmc passes of %s, not measured in this run" % (
                        key, tj.get(key, {}).get("session", "an earlier session"))
            except Exception:
                traffic = None
        out = {
            "metric": "images/sec (resize+thumb+watermark) on 1080p batch at 1/2/4/8 MI355X",
            "value": round(frames_done / elapsed, 1),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": K,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / K * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32+f64",
            "data": "synthetic: %d seeded opaque RGBA8 frames per GPU tiled over %d slots resident in HBM" % (P, F),
            "config": {"workload": "%d x %dx%d RGBA8, %s" % (F, sw, sh, {
                "full": "full pipeline: resize 1024x768 (keep_aspect=false) + thumbnail 200 crop + watermark 16 glyphs",
                "resize": "resize to 1024x768 only",
                "full-keepaspect": "full pipeline, product-default keep_aspect=true (1024x576)",
                "wm": "watermark only (copy + 16 glyphs)", "thumb": "thumbnail 200 crop only",
                "resize-wm": "resize 1024x768 + watermark"}[args.workload]),
                "frames_per_gpu": F, "sharding": "independent frames, round-robin by rank, no collective",
                "arithmetic": "u8 pixels in, u8 pixels out, every byte the reference's: x/image's kernel scaler is evaluated in f32 with a proven error margin, and each value that margin cannot separate from a rounding boundary (about 0.1 % of the pixels) is recomputed in f64, every product rounded before it is added as in the reference's amd64 build (IPX_KS_FAST=0: f64 throughout, 5.7 ms per launch against 4.4); composite in u32"},
            "checked": checked,
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                         "kernel": "ks_fused_kernel<RGBA, 3 channels, float pass> (frames taken as opaque; ks_fix_kernel recomputes the listed pixels in float64, the 4-channel float64 kernel redoes items that meet alpha != 0xff or fill their list); avg_launch_ms covers all of a call's kernels",
                         "in_practice": "HBM streaming: the launch moves the algorithmic minimum at 0.84 - 0.88 of what ipx_stream_copy reaches on the same box (copy_ceiling); with float64 throughout it was float64 VALU issue (DESIGN.md 4.1)",
                         "algorithmic_bytes_per_launch": alg,
                         "avg_launch_ms": round(avg_ms, 4), "traffic_source": traffic_src,
                         "buffer_sets": nsets,
                         "avg_launch_ms_by_set": [round(sum(launch_ms[i::nsets]) / len(launch_ms[i::nsets]), 4) for i in range(nsets)],
                         "frac_best_set": round(alg / (min(sum(launch_ms[i::nsets]) / len(launch_ms[i::nsets]) for i in range(nsets)) * 1e-3) / 1e9
                                                / HBM_PEAK_GBS, 4)},
        }
        if args.full and world == 1 and args.copy_gib > 0:
            cc = copy_ceiling(ctx, args.copy_gib)
            out["roofline"]["copy_ceiling"] = cc
            out["roofline"]["frac_of_copy_ceiling"] = round(achieved / cc["best"], 4)
        if args.full and world == 1 and args.cpu_seconds > 0:
            out["cpu_baseline"] = cpu_baseline(pool, glyphs, DEFAULT_COL, resize, thumb,
                                               [k for k, b in (("resize", res), ("thumbnail", th), ("watermark", wm)) if b],
                                               args.cpu_seconds)
        else:
            out["cpu_baseline"] = None
        if args.full and world == 1 and args.e2e_frames > 0 and args.workload in ("full", "full-keepaspect"):
            for bs in sets:
                for b in bs:
                    if b:
                        b.free()
            # the timed region's context goes first: a process holds ONE context or pool per device in production, and a second idle
            # one costs the pool leg 12 % (its streams share the device's hardware queues)
            plan.close()
            ctx.close()
            plan = ctx = None
            out["e2e"] = e2e_legs(ipx, local_rank % max(1, ipx.device_count()), args.e2e_frames, sw, sh, resize, args.e2e_reps)
        else:
            out["e2e"] = None
        print(json.dumps(out), flush=True)

    if dist:
        dist.barrier()
        dist.destroy_process_group()
    if ctx is not None:
        plan.close()
        ctx.close()


if __name__ == "__main__":
    main()
