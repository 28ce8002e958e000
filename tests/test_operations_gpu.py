"""The reference's operator interface (Resizer / Thumbnailer / Watermarker .Process and
ImageProcessor.Process) on the HIP path, against expectations assembled from the CPU oracle and
the parameter / error rules of operations/*.go and image_processor.go."""
import numpy as np
import pytest

import oracle
from helpers import rgba_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipx():
    import imageprocessor_amd as m
    return m


@pytest.fixture(scope="module")
def ops(ipx):
    from imageprocessor_amd import operations
    return operations


@pytest.fixture(scope="module")
def ctx(ipx):
    c = ipx.Context(lanes=2)
    yield c
    c.close()


# a deterministic stand-in for golang/freetype + Go Regular (the glyph producer is outside the path)
def fake_measure(text, size):
    return int(len(text) * size * 0.52) + 1


def fake_glyphs(text, size, px, py, w=None, h=None):
    out = []
    x = px
    for i, ch in enumerate(text):
        rng = np.random.default_rng(ord(ch) * 131 + int(size * 8))
        mw, mh = max(2, int(size * 0.6)), max(2, int(size * (0.6 + 0.4 * rng.random())))
        m = rng.integers(0, 256, (mh, mw), dtype=np.uint8)
        m[rng.random((mh, mw)) < 0.4] = 0
        out.append({"mask": m, "dr": (x - 1, py - mh + (i % 3), x - 1 + mw, py + (i % 3)), "mp": (0, 0)})
        x += int(size * 0.52)
    return out


@pytest.fixture(scope="module")
def font(ops):
    return ops.Font(fake_measure, fake_glyphs)


def expect_watermark(src, text, position, opacity, size, color):
    h, w = src.shape[:2]
    col, _ = oracle.parse_color(color, opacity)
    px, py = oracle.watermark_anchor(position, w, h, fake_measure(text, size), oracle.text_height_px(size))
    out = src.copy()
    oracle.composite_glyphs(out, fake_glyphs(text, size, px, py), col)
    return out


SRC = rgba_frames(1, 640, 360, seed=77)[0]


def test_resizer_parameter_ladder_and_formats(ctx, ops):
    r = ops.Resizer()
    want_fit = oracle.scale_bilinear(SRC, *oracle.resize_dims(640, 360, 300, 300, True))
    for params in ({"width": 300.0, "height": 300.0, "keep_aspect": True},          # after the JSON round trip
                   {"width": 300, "height": 300, "keep_aspect": True},
                   {"width": ops.Int64(300), "height": ops.Int32(300), "keep_aspect": True},
                   {"width": 300.9, "height": 300.2, "keep_aspect": True}):           # int(w) truncates
        got, fmt = r.Process(ctx, SRC, "jpeg", params)
        np.testing.assert_array_equal(got, want_fit)
        assert fmt == "jpeg"
    got, _ = r.Process(ctx, SRC, "png", {"width": 300, "height": 300})               # keep_aspect absent = false
    np.testing.assert_array_equal(got, oracle.scale_bilinear(SRC, 300, 300))
    got, _ = r.Process(ctx, SRC, "png", {"width": 300, "height": 300, "keep_aspect": "true"})  # not a bool = false
    assert got.shape == (300, 300, 4)
    for f, want in (("JPG", "jpeg"), ("jpeg", "jpeg"), ("png", "png"), ("GIF", "gif"), ("webp", "jpeg"), ("", "jpeg")):
        assert r.Process(ctx, SRC, f, {"width": 8, "height": 8})[1] == want


def test_resizer_errors(ctx, ops, ipx):
    r = ops.Resizer()
    for params, text in (({"height": 5}, "width parameter is required and must be a number"),
                         ({"width": "5", "height": 5}, "width parameter is required and must be a number"),
                         ({"width": 5}, "height parameter is required and must be a number"),
                         ({"width": 5, "height": True}, "height parameter is required and must be a number"),
                         ({"width": 0, "height": 5}, "width and height must be positive numbers"),
                         ({"width": 5, "height": -1.0}, "width and height must be positive numbers")):
        with pytest.raises(ipx.IpxError) as e:
            r.Process(ctx, SRC, "jpeg", params)
        assert e.value.text == text


def test_thumbnailer(ctx, ops, ipx):
    t = ops.Thumbnailer()
    crop, nw, nh = oracle.thumb_geometry(640, 360, 200, True)
    want = oracle.scale_bilinear(SRC, nw, nh, sr=crop)
    for params in ({"crop_to_fit": True}, {"size": "big", "crop_to_fit": True}, {"size": 200.0, "crop_to_fit": True}):
        got, fmt = t.Process(ctx, SRC, "jpg", params)       # size absent / not a number -> 200 (task.go:56)
        np.testing.assert_array_equal(got, want)
        assert fmt == "jpeg"
    _, nw, nh = oracle.thumb_geometry(640, 360, 50, False)
    got, _ = t.Process(ctx, SRC, "png", {"size": 50})
    assert (nw, nh) == (88, 50)
    np.testing.assert_array_equal(got, oracle.scale_bilinear(SRC, nw, nh))
    tall = np.ascontiguousarray(SRC.transpose(1, 0, 2))
    got, _ = t.Process(ctx, tall, "png", {"size": 50, "crop_to_fit": False})
    np.testing.assert_array_equal(got, oracle.scale_bilinear(tall, 50, 88))
    for bad in (0, -3, -1.5):
        with pytest.raises(ipx.IpxError) as e:
            t.Process(ctx, SRC, "png", {"size": bad})
        assert e.value.text == "size must be a positive number"
    assert t.Process(ctx, SRC, "gif", {})[1] == "gif"


def test_watermarker(ctx, ops, ipx, font):
    w = ops.Watermarker(font)
    got, fmt = w.Process(ctx, SRC, "jpeg", {})               # every default of watermark.go:41-60
    np.testing.assert_array_equal(got, expect_watermark(SRC, "© ImageProcessor", "bottom-right", 0.5, 36, "255,255,255"))
    assert fmt == "jpeg"
    cases = [
        ({"text": "hello", "opacity": 0.8, "position": "top-left", "font_size": 20.0, "font_color": "10,200,30"},
         ("hello", "top-left", 0.8, 20.0, "10,200,30")),
        ({"text": "", "opacity": -1.0, "position": "center", "font_size": 0.0, "font_color": "1,2,3,200"},
         ("© ImageProcessor", "center", 0.5, 36, "1,2,3,200")),          # empty / non-positive -> defaults
        ({"text": "x y", "opacity": 1, "position": "nowhere", "font_size": 24, "font_color": "red"},
         ("x y", "nowhere", 0.5, 36, "red")),                                 # ints are not float64 -> defaults; bad colour -> black
        ({"position": 7}, ("© ImageProcessor", "bottom-right", 0.5, 36, "255,255,255")),
    ]
    for params, exp in cases:
        got, _ = w.Process(ctx, SRC, "png", params)
        np.testing.assert_array_equal(got, expect_watermark(SRC, *exp), err_msg=str(params))
    for f, want in (("png", "png"), ("gif", "jpeg"), ("jpg", "jpeg"), ("bmp", "jpeg")):   # watermark.go:66-79
        assert w.Process(ctx, SRC, f, {"text": "a"})[1] == want
    with pytest.raises(ipx.IpxError) as e:
        ops.Watermarker(None).Process(ctx, SRC, "png", {})
    assert e.value.text == "failed to add watermark: font not loaded"           # watermark.go:87-89,61-64


def test_watermarker_with_the_library_font(ctx, ops, ipx):
    """NewWatermarker's font slot filled by the library's own truetype / freetype restatement (ipx_font_*):
    text -> glyph masks on the host -> composite on the GPU, against the Python model of the glyph producer
    plus the oracle's composite."""
    from oracle import ft_model
    from helpers import DEJAVU as path
    f = ops.TrueTypeFont.from_file(path)
    model = ft_model.Font(path)
    w = ops.Watermarker(f)
    h_, w_ = SRC.shape[:2]
    for params, (text, pos, opacity, size, color) in (
            ({}, ("© ImageProcessor", "bottom-right", 0.5, 36, "255,255,255")),
            ({"text": "Grüße, Welt!", "position": "top-left", "font_size": 23.5, "font_color": "250,10,10", "opacity": 0.9},
             ("Grüße, Welt!", "top-left", 0.9, 23.5, "250,10,10")),
            ({"text": "a very long line of text that runs out of the frame on the right hand side", "position": "center",
              "font_size": 48.0}, ("a very long line of text that runs out of the frame on the right hand side", "center", 0.5, 48.0,
                                   "255,255,255"))):
        got, _ = w.Process(ctx, SRC, "png", params)
        col, _ = oracle.parse_color(color, opacity)
        _, width_px = ft_model.text_width(model, text, size)
        px, py = oracle.watermark_anchor(pos, w_, h_, width_px, oracle.text_height_px(size))
        glyphs, _ = ft_model.draw_string(model, text, size, px, py, w_, h_)
        want = SRC.copy()
        oracle.composite_glyphs(want, glyphs, col)
        np.testing.assert_array_equal(got, want, err_msg=str(params))
        assert (got != SRC).any()
    # the same font feeding a batch plan
    gl, _ = f.draw_string("© ImageProcessor", 36, 100, 300, w_, h_)
    gs = ctx.glyphset(gl, (255, 255, 255, 127))
    plan = ctx.plan(w_, h_, watermark=gs)
    out = plan.run_host(np.stack([SRC, SRC[::-1].copy()]))
    for i, src in enumerate((SRC, SRC[::-1])):
        want = src.copy()
        oracle.composite_glyphs(want, gl, (255, 255, 255, 127))
        np.testing.assert_array_equal(out["watermark"][i], want)
    plan.close()
    gs.close()
    f.close()


def _task(ops_list, fmt=""):
    return {"ID": "task-1", "ImageID": "img-42", "OriginalPath": "original/img-42.jpg", "Bucket": "original",
            "Operations": ops_list, "Format": fmt}


def test_image_processor_standard_task(ctx, ops, font):
    # parseOperationsFromForm (handler/image/image.go:222-256) after json.Marshal / Unmarshal
    task = _task([{"Type": "thumbnail", "Parameters": {"size": 200.0, "crop_to_fit": True}},
                  {"Type": "resize", "Parameters": {"width": 1024.0, "height": 768.0, "keep_aspect": True}},
                  {"Type": "watermark", "Parameters": {"text": "© ImageProcessor", "opacity": 0.5, "position": "bottom-right"}}])
    res, err = ops.ImageProcessor(ctx, font).Process(task, SRC, "jpeg")
    assert err is None and res["Status"] == "completed" and res["Error"] == ""
    assert res["ProcessedPaths"] == {"thumbnail": "processed/thumbnails/img-42/200.jpeg",
                                     "resize": "processed/resize/img-42/1024x768.jpeg",       # requested, not actual, size
                                     "watermark": "processed/watermarked/img-42/watermarked.jpeg"}
    crop, tw, th = oracle.thumb_geometry(640, 360, 200, True)
    np.testing.assert_array_equal(res["Outputs"]["thumbnail"][0], oracle.scale_bilinear(SRC, tw, th, sr=crop))
    np.testing.assert_array_equal(res["Outputs"]["resize"][0], oracle.scale_bilinear(SRC, *oracle.resize_dims(640, 360, 1024, 768, True)))
    np.testing.assert_array_equal(res["Outputs"]["watermark"][0],
                                  expect_watermark(SRC, "© ImageProcessor", "bottom-right", 0.5, 36, "255,255,255"))
    assert all(v[1] == "image/jpeg" for v in res["Outputs"].values())
    # task.Format overrides the decoded format (image_processor.go:55-58); a PNG task keeps PNG everywhere
    res, _ = ops.ImageProcessor(ctx, font).Process(_task(task["Operations"], "png"), SRC, "jpeg")
    assert res["ProcessedPaths"]["watermark"].endswith(".png") and res["Outputs"]["resize"][1] == "image/png"


def test_image_processor_failures_and_quirks(ctx, ops, font):
    ip = ops.ImageProcessor(ctx, font)
    res, err = ip.Process(_task([{"Type": "thumbnail", "Parameters": {}},
                                 {"Type": "resize", "Parameters": {"height": 10.0}},
                                 {"Type": "watermark", "Parameters": {}}]), SRC)
    assert err == "operation resize failed: failed to process operation resize: width parameter is required and must be a number"
    assert res["Status"] == "failed" and res["Error"].startswith("Operation resize failed: ")
    assert list(res["ProcessedPaths"]) == ["thumbnail"]          # stored before the failure (image_processor.go:76-92)
    res, err = ip.Process(_task([{"Type": "rotate", "Parameters": {"angle": 90.0}}]), SRC)
    assert err == "operation rotate failed: unsupported operation type: rotate" and not res["ProcessedPaths"]
    res, err = ops.ImageProcessor(ctx, None).Process(_task([{"Type": "watermark", "Parameters": {}}]), SRC)
    assert err == "operation watermark failed: failed to process operation watermark: failed to add watermark: font not loaded"
    # generatePath reads width / height with the short ladder only (float64, int): int64 prints as 0
    res, err = ip.Process(_task([{"Type": "resize", "Parameters": {"width": ops.Int64(64), "height": ops.Int64(48)}}], "gif"), SRC)
    assert err is None and res["ProcessedPaths"]["resize"] == "processed/resize/img-42/0x0.gif"
    assert res["Outputs"]["resize"][0].shape == (48, 64, 4) and res["Outputs"]["resize"][1] == "image/gif"
    # the same operator twice: last path wins in ProcessedPaths, both run on the ORIGINAL frame
    res, err = ip.Process(_task([{"Type": "resize", "Parameters": {"width": 32, "height": 32}},
                                 {"Type": "resize", "Parameters": {"width": 16, "height": 16}}]), SRC)
    assert err is None and res["ProcessedPaths"]["resize"] == "processed/resize/img-42/16x16.jpeg"
    np.testing.assert_array_equal(res["Outputs"]["resize"][0], oracle.scale_bilinear(SRC, 16, 16))
    # an empty operator list is a completed task with no outputs
    res, err = ip.Process(_task([]), SRC)
    assert err is None and res["Status"] == "completed" and not res["Outputs"]


def test_single_image_calls_are_served_while_a_batch_runs(ipx, ops, font):
    """image_processor.go:64-77 per message next to a batch of the same process: the per-operator seam takes its plan and glyph
    set from the context's cache (no hipMalloc / hipFree after the first call -- each of those waits for every stream of the
    device) and ONE staging lane, and a host batch leaves one lane free: single calls finish while the batch is still running,
    and both produce the oracle's bytes.

    Round 2 retried the latency bound on up to three contexts: about one context in ten had its single calls wait for the batch.  The
    cause was the order in which the context made its streams: ROCclr hands streams to hardware queues in creation order, and the
    high-priority lane, made last, came to share a queue with a batch lane.  It is made first now (and GPU_MAX_HW_QUEUES is raised to
    one queue per stream of a context before the runtime starts, ipx_create): 32 contexts of 32 served their single calls in 3 - 9 ms
    beside a 115 ms batch (tools/seam_hunt.py), so the bound is asserted on the first context.  The other cause this test found -- small
    pageable copies blocking the ENQUEUEING thread behind other streams' work -- went away with the pinned bounce buffer (run_host_packed)."""
    import threading
    import time
    task = _task([{"Type": "thumbnail", "Parameters": {"size": 200.0, "crop_to_fit": True}},
                  {"Type": "resize", "Parameters": {"width": 1024.0, "height": 768.0, "keep_aspect": True}},
                  {"Type": "watermark", "Parameters": {"text": "© ImageProcessor", "opacity": 0.5, "position": "bottom-right"}}])
    want_wm = expect_watermark(SRC, "© ImageProcessor", "bottom-right", 0.5, 36, "255,255,255")
    n, w, h = 384, 1920, 1080
    batch_frames = rgba_frames(4, w, h, seed=5)
    want = oracle.process(batch_frames[1], resize=(1024, 768, True), thumb=(200, True))
    tried = []
    for attempt in range(1):
        with ipx.Context(device=0) as c:        # default lanes: four for a batch's pipeline, one left for single calls
            ip = ops.ImageProcessor(c, font)
            for _ in range(3):                  # first call builds the plan; the later ones come from the cache
                res, err = ip.Process(task, SRC, "jpeg")
                assert err is None
            frames = c.host_alloc((n, h, w, 4))
            frames[:] = np.resize(batch_frames, frames.shape)
            plan = c.plan(w, h, resize=(1024, 768, True), thumbnail=(200, True), watermark=True)
            outs = {"resize": c.host_alloc((n, 576, 1024, 4)), "thumbnail": c.host_alloc((n, 200, 200, 4)), "watermark": c.host_alloc((n, h, w, 4))}
            plan.run_host(frames, out=outs)                                     # warm the lanes
            t0 = time.perf_counter()
            plan.run_host(frames, out=outs)
            batch_alone = time.perf_counter() - t0
            state = {"running": True, "batches": 0}

            def batches():
                while state["running"]:
                    plan.run_host(frames, out=outs)
                    state["batches"] += 1
            th = threading.Thread(target=batches)
            th.start()
            time.sleep(batch_alone * 0.3)
            lat = []
            try:
                for _ in range(12):
                    t0 = time.perf_counter()
                    res, err = ip.Process(task, SRC, "jpeg")
                    lat.append(time.perf_counter() - t0)
                    assert err is None
                    np.testing.assert_array_equal(res["Outputs"]["watermark"][0], want_wm)
            finally:
                state["running"] = False
                th.join()
            np.testing.assert_array_equal(outs["resize"][1], want["resize"])
            plan.close()
            for a in [frames] + list(outs.values()):
                c.host_free(a)
        # a call that had to wait for the device to drain would take about batch_alone (every chunk of a batch is queued at once);
        # what is left is queueing behind the copies that already sit on the link
        median = sorted(lat)[len(lat) // 2]
        tried.append((round(median * 1e3, 2), round(batch_alone * 1e3, 1)))
        if median < 0.5 * batch_alone:
            break
    assert tried[-1][0] < 0.5 * tried[-1][1], "median single-call latency (ms) / batch alone (ms) per attempt: %s" % tried


def test_fused_failure_falls_back_to_the_sequential_order(ctx, ops):
    """image_processor.go:64-92: when the watermark fails (here: the rasteriser), the resize before it has already been stored and
    the error names the watermark operator with its own prefix."""
    def bad_glyphs(text, size, px, py, w=None, h=None):
        raise RuntimeError("no outlines")
    broken = ops.Font(fake_measure, bad_glyphs)
    res, err = ops.ImageProcessor(ctx, broken).Process(_task([{"Type": "resize", "Parameters": {"width": 64.0, "height": 36.0}},
                                                              {"Type": "watermark", "Parameters": {}}]), SRC)
    assert err == ("operation watermark failed: failed to process operation watermark: failed to add watermark: "
                   "failed to draw watermark text: rasteriser failed")
    assert list(res["ProcessedPaths"]) == ["resize"] and res["Status"] == "failed"
    np.testing.assert_array_equal(res["Outputs"]["resize"][0], oracle.scale_bilinear(SRC, 64, 36))


def test_plan_cache_replaces_the_least_recently_used_plan(ipx, monkeypatch):
    """ipx_plan_acquire (what every per-operator call and the pool go through): a worker fed arbitrary upload sizes must not fill the
    cache with sizes it never sees again.  With room for 8 plans: 20 different sizes go in, a size used a moment ago is still there, the
    oldest is gone, and a plan some call still holds is never the victim."""
    import ctypes as C
    from imageprocessor_amd import _lib
    monkeypatch.setenv("IPX_PLAN_CACHE_MAX", "8")
    L = ipx.lib()
    with ipx.Context(device=0) as c:
        def acquire(w):
            ops_ = _lib.PoolOps(sw=w, sh=40, do_resize=1, resize_w=16, resize_h=16, keep_aspect=0, do_thumbnail=0, thumb_size=0, crop_to_fit=0,
                                do_watermark=0, glyphs=None, n_glyphs=0)
            plan, cached = C.c_void_p(), C.c_int()
            assert L.ipx_plan_acquire(c.handle, C.byref(ops_), C.byref(plan), C.byref(cached)) == 0
            return plan.value, cached.value
        held, _ = acquire(1000)                            # kept by "a call in flight" through everything below
        seen = {}
        for w in range(100, 120):
            p, cached = acquire(w)
            assert cached == 1
            seen[w] = p
            L.ipx_plan_release(c.handle, p, cached)
        p, cached = acquire(119)                           # the most recent one: a hit, the same plan
        assert cached == 1 and p == seen[119]
        L.ipx_plan_release(c.handle, p, cached)
        p, cached = acquire(1000)                          # never evicted while held
        assert cached == 1 and p == held
        L.ipx_plan_release(c.handle, p, cached)
        L.ipx_plan_release(c.handle, held, 1)
        # the oldest sizes were replaced: asking for one builds a new plan that works
        frames = rgba_frames(1, 100, 40, seed=3)
        p, cached = acquire(100)
        assert cached == 1
        out = np.zeros((1, 16, 16, 4), np.uint8)
        src_d, out_d = c.alloc(frames.nbytes).upload(frames), c.alloc(out.nbytes)
        assert L.ipx_plan_run_dev(c.handle, None, p, 1, src_d.ptr, 400, frames.nbytes, out_d.ptr, out.nbytes, None, 0, None, 0) == 0
        c.sync()
        np.testing.assert_array_equal(out_d.download((16, 16, 4)), oracle.scale_bilinear(frames[0], 16, 16))
        L.ipx_plan_release(c.handle, p, cached)


@pytest.mark.parametrize("shape", [(640, 360, 9, (1024, 768, True), (200, True)),      # every stride a multiple of 16: the kernels store into the pinned outputs
                                   (333, 251, 5, (201, 99, False), (63, False)),       # odd strides: through the lane's scratch and copy engines
                                   (1280, 720, 7, (500, 333, False), (64, True))],
                         ids=lambda c: "%dx%d" % (c[0], c[1]))
@pytest.mark.parametrize("direct", ["1", "0"], ids=["kernel-stored", "copied"])
def test_pinned_outputs_of_the_host_entries(ctx, shape, direct, monkeypatch):
    """ipx_plan_run_host with frames and outputs in pinned memory (ipx_host_alloc): the kernels store the outputs over the link
    themselves when every pointer and stride is 16-byte aligned (IPX_HOST_DIRECT=0: the copy path), several chunks per call, the text
    composite reading and writing the pinned watermark frames; the same bytes as the oracle, and nothing written beside the outputs."""
    from helpers import DEFAULT_COL, rgba_frames, text_glyphs
    monkeypatch.setenv("IPX_HOST_DIRECT", direct)
    monkeypatch.setenv("IPX_HOST_CHUNK", "2")
    sw, sh, n, resize, thumb = shape
    frames = rgba_frames(n, sw, sh, seed=sw + n)
    glyphs = text_glyphs(sw, sh, n=6, width_px=min(150, sw), height_px=min(30, sh))
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(sw, sh, resize=resize, thumbnail=thumb, watermark=gs)
    i = plan.info
    src = ctx.host_alloc((n, sh, sw, 4))
    src[:] = frames
    # one guard frame behind each output: it must stay untouched
    outs = {"resize": ctx.host_alloc((n + 1, i.resize_h, i.resize_w, 4)), "thumbnail": ctx.host_alloc((n + 1, i.thumb_h, i.thumb_w, 4)),
            "watermark": ctx.host_alloc((n + 1, i.wm_h, i.wm_w, 4))}
    for a in outs.values():
        a[:] = 0xA5
    got = plan.run_host(src, out={k: v[:n] for k, v in outs.items()})
    for k in range(n):
        want = oracle.process(frames[k], resize=resize, thumb=thumb, glyphs=glyphs, col=DEFAULT_COL)
        for key in ("resize", "thumbnail", "watermark"):
            np.testing.assert_array_equal(got[key][k], want[key], err_msg="%s frame %d" % (key, k))
    for key, a in outs.items():
        assert (a[n] == 0xA5).all(), key
    for a in [src] + list(outs.values()):
        ctx.host_free(a)
    plan.close()
    gs.close()
