"""A watermark text per file (watermark_text of the upload form, handler/image/image.go:249-251): the text set and its one launch
(composite_texts_kernel, csrc/ipx_kernels.hip) against oracle.composite_glyphs frame by frame, the layout rule of the ipx_dev_*
entries, the refusals the host makes before any launch, and the three compressed-in / compressed-out legs, the pool and the
micro-batcher with texts[i] on files[i] -- where the indexing can go wrong: parts and chunks of the JPEG leg, the PNG leg's sort by kind.
Expected values: the oracle as it stands -- its decoders (oracle.jpeg_decode; tests/png_decode_model.py, tests/gif_decode_model.py), the
watermark's draw.Draw of the decoded type, oracle.composite_glyphs with the file's own glyphs and colour, the oracle's encoder."""
import ctypes as C
import io
import threading

import numpy as np
import pytest

import gif_corpus
import gif_decode_model as gdm
import oracle
import png_corpus as pc
import png_decode_model as pdm
import png_model
from helpers import rgba_frames

pytestmark = pytest.mark.gpu
PIL = pytest.importorskip("PIL.Image")

W, H = 96, 64
RESIZE, THUMB = (32, 24, False), (16, True)


@pytest.fixture(scope="module")
def ipx():
    import imageprocessor_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(ipx):
    with ipx.Context(device=0) as c:
        yield c


def _mask(rng, mh, mw):
    m = rng.integers(0, 256, (mh, mw), dtype=np.uint8)
    sel = rng.random((mh, mw))
    m[sel < 0.3] = 0
    m[sel > 0.75] = 255
    return m


def _run(rng, n, x0, y0, gw, gh, step, windowed=False):
    """n glyphs of gw x gh walking right from (x0, y0) by `step` (< gw: neighbours overlap).  windowed: every mask is a window of a
    larger array (mstride > mw) and is entered at mp = (1, 2), its own rectangle two columns and three rows smaller"""
    out = []
    for i in range(n):
        x, y = x0 + i * step, y0 + int(rng.integers(0, 3))
        if windowed:
            big = _mask(rng, gh + 4, gw + 9)
            out.append({"mask": big[1:1 + gh, 3:3 + gw], "dr": (x, y, x + gw - 2, y + gh - 3), "mp": (1, 2)})
        else:
            out.append({"mask": _mask(rng, gh, gw), "dr": (x, y, x + gw, y + gh), "mp": (0, 0)})
    return out


def device_texts():
    """9 (glyphs, colour): counts 0, 1, 3, 4, 5, 8, 9, 17 (across the walk's step of four) and 256 glyphs of 2 x 2; anchored top-left,
    bottom-right, across each of the four edges, wholly outside; the wrap colour, opaque black, alpha 0"""
    rng = np.random.default_rng(20261019)
    small = []
    for i in range(256):                                     # 2 x 2 each, a pixel apart: every glyph overlaps its neighbour
        x, y = 8 + i % 64, 20 + 3 * (i // 64)
        small.append({"mask": _mask(rng, 2, 2), "dr": (x, y, x + 2, y + 2), "mp": (0, 0)})
    return [
        ([], (1, 2, 3, 4)),
        (_run(rng, 1, 200, 10, 9, 12, 7), (9, 9, 9, 200)),                      # wholly outside
        (_run(rng, 3, 0, 0, 11, 14, 8), (255, 255, 255, 127)),                  # top-left; not premultiplied: the uint32 wrap
        (_run(rng, 4, W - 38, H - 17, 11, 15, 9), (0, 0, 0, 255)),              # ends at the bottom-right corner
        (_run(rng, 5, -6, 20, 10, 13, 7), (10, 20, 30, 0)),                     # across the left edge; alpha 0
        (_run(rng, 8, 5, -7, 12, 16, 9), (200, 100, 50, 255)),                  # across the top edge
        (_run(rng, 9, 20, 30, 12, 14, 9, windowed=True), (30, 60, 90, 180)),    # across the right edge; mstride > mw, mp != (0, 0)
        (_run(rng, 17, 2, H - 6, 8, 12, 5), (255, 0, 255, 64)),                 # across the bottom edge
        (small, (17, 34, 51, 85)),
    ]


@pytest.fixture(scope="module")
def dev_case():
    """frames, texts and, computed once, want[z][t]: frame z with text t on it"""
    texts = device_texts()
    assert [len(g) for g, _ in texts] == [0, 1, 3, 4, 5, 8, 9, 17, 256]
    frames = rgba_frames(9, W, H, seed=77, opaque=False)
    frames[4] = rgba_frames(1, W, H, seed=78)[0]             # one opaque frame among them
    want = {}

    def expect(z, t):
        if (z, t) not in want:
            want[(z, t)] = oracle.composite_glyphs(frames[z].copy(), texts[t][0], texts[t][1])
        return want[(z, t)]
    for z in range(9):
        assert (z in (0, 1)) == np.array_equal(expect(z, z), frames[z]), z   # the empty text and the one outside draw nothing; alpha 0 with colour does
    return frames, texts, expect


def _composite(ctx, frames, ts, first=0, tmap=None):
    n = len(frames)
    buf = ctx.alloc(n * W * H * 4).upload(frames)
    ctx.dev_composite_texts(buf.ptr, W, H, W * 4, W * H * 4, n, ts, first=first, map=tmap)
    ctx.sync()
    got = buf.download((n, H, W, 4))
    buf.free()
    return got


def test_device_entry_every_frame_its_own_text(ipx, ctx, dev_case):
    frames, texts, expect = dev_case
    ts = ctx.textset(texts, W, H)
    got = _composite(ctx, frames, ts)
    for z in range(9):
        assert np.array_equal(got[z], expect(z, z)), "frame %d" % z
    # a sub-range: frames 0 .. 3 take texts 3 .. 6
    got = _composite(ctx, frames[:4], ts, first=3)
    for z in range(4):
        assert np.array_equal(got[z], expect(z, 3 + z)), "first = 3, frame %d" % z
    # a shuffled map, one text twice and one not at all
    tmap = [int(v) for v in np.random.default_rng(5).permutation(9)]
    tmap[0] = tmap[8]
    got = _composite(ctx, frames, ts, tmap=tmap)
    for z in range(9):
        assert np.array_equal(got[z], expect(z, tmap[z])), "map, frame %d takes text %d" % (z, tmap[z])
    # indices are checked on the host
    for kw in ({"first": 1}, {"first": -1}, {"tmap": [0] * 8 + [9]}, {"tmap": [0] * 8 + [-1]}):
        with pytest.raises(ipx.IpxError) as e:
            _composite(ctx, frames, ts, **kw)
        assert e.value.status == -1
    ts.close()


@pytest.mark.parametrize("off", [0, 4, 8, 12])
def test_layout_padded_strides_and_offsets(ipx, ctx, dev_case, off):
    frames, texts, expect = dev_case
    ts = ctx.textset(texts, W, H)
    dstride = W * 4 + 32
    fs = dstride * H + 48
    total = 16 + off + 9 * fs + 64
    host = np.full(total, 0xA5, np.uint8)
    inside = np.zeros(total, bool)
    for z in range(9):
        for y in range(H):
            a = 16 + off + z * fs + y * dstride
            host[a:a + W * 4] = frames[z][y].reshape(-1)
            inside[a:a + W * 4] = True
    buf = ctx.alloc(total).upload(host)
    ctx.dev_composite_texts(buf.ptr + 16 + off, W, H, dstride, fs, 9, ts)
    ctx.sync()
    got = buf.download((total,))
    assert (got[~inside] == 0xA5).all(), "bytes between or around the frames were written"
    for z in range(9):
        rows = np.stack([got[16 + off + z * fs + y * dstride:][:W * 4] for y in range(H)]).reshape(H, W, 4)
        assert np.array_equal(rows, expect(z, z)), "frame %d" % z
    # a misaligned destination, row stride or frame stride: refused on the host, nothing written
    buf.upload(host)
    for dp, ds, df in ((2, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 2), (0, 0, 1)):
        with pytest.raises(ipx.IpxError) as e:
            ctx.dev_composite_texts(buf.ptr + 16 + off + dp, W, H, dstride + ds, fs + df, 9, ts)
        assert e.value.status == -1 and "multiples of 4" in e.value.text
    ctx.sync()
    assert np.array_equal(buf.download((total,)), host)
    buf.free()
    ts.close()


def test_refusals_on_the_host(ipx, ctx):
    from imageprocessor_amd import _lib
    rng = np.random.default_rng(1)
    ok = _run(rng, 2, 4, 4, 6, 6, 4)
    one = {"mask": _mask(rng, 2, 2), "dr": (1, 1, 3, 3), "mp": (0, 0)}
    with pytest.raises(ipx.IpxError) as e:
        ctx.textset([(ok, (1, 1, 1, 1)), ([one] * 257, (1, 1, 1, 1))], W, H)
    assert e.value.status == -4 and "256" in e.value.text
    ctx.textset([([one] * 256, (1, 1, 1, 1)), ([], (0, 0, 0, 0))], W, H).close()          # 256 and an empty text are fine
    # bad masks, through the raw table: rows shorter than the mask is wide; no mask although it has an area
    m = np.zeros((4, 4), np.uint8)
    for g in (_lib.Glyph(m.ctypes.data, 4, 4, 2, _lib.Rect(0, 0, 4, 4), 0, 0), _lib.Glyph(None, 4, 4, 4, _lib.Rect(0, 0, 4, 4), 0, 0)):
        t = (_lib.Text * 1)()
        t[0].glyphs, t[0].n_glyphs = C.pointer(g), 1
        h = C.c_void_p()
        assert ipx.lib().ipx_textset_create(ctx.handle, None, t, 1, W, H, C.byref(h)) == -1 and not h.value
        assert b"bad mask" in ipx.lib().ipx_last_error()
    # a plan that carries a glyph set of its own is not a copy-only plan
    gs = ctx.glyphset(ok, (1, 2, 3, 4))
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=None, watermark=gs)
    f = _jpeg(rgba_frames(1, W, H, seed=3)[0][..., :3])
    for run in (plan.run_jpeg_jpeg, plan.run_png_png, plan.run_gif_gif):
        with pytest.raises(ipx.IpxError) as e:
            run([f], texts=[(ok, (1, 1, 1, 1))])
        assert e.value.status == -1 and "glyph set" in e.value.text
    plan.close()
    gs.close()
    # a text too long for a text set refuses the leg's call too, before anything runs
    plan = ctx.plan(W, H, resize=RESIZE, thumbnail=None, watermark=True)
    with pytest.raises(ipx.IpxError) as e:
        plan.run_jpeg_jpeg([f], texts=[([one] * 257, (1, 1, 1, 1))])
    assert e.value.status == -4
    plan.close()


# ---- the legs ------------------------------------------------------------------------------------------------------------------------

def _jpeg(rgb, **kw):
    buf = io.BytesIO()
    PIL.fromarray(rgb).save(buf, "JPEG", **kw)
    return buf.getvalue()


def file_texts(n, sw, sh, seed):
    """n different texts for sw x sh frames: 0 .. n - 1 glyphs growing from the left, at places and in colours of their own"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        x0, y0 = int(rng.integers(-4, sw // 3)), int(rng.integers(-4, sh - 10))
        col = (255, 255, 255, 127) if k == 1 else tuple(int(v) for v in rng.integers(0, 256, 4))
        out.append((_run(rng, k + (k > 0), x0, y0, 7, 11, 5), col))      # 0, 2, 3, ... glyphs
    return out


JW, JH = 64, 48


@pytest.fixture(scope="module")
def jpeg_case():
    files = [_jpeg(rgba_frames(1, JW, JH, seed=300 + i)[0][..., :3] // 2 + 40 * (i % 3), quality=75 + 2 * i, subsampling=2) for i in range(8)]
    f = files[5]
    sos = f.index(b"\xff\xda")
    files[5] = f[:sos + (len(f) - sos) // 2]                 # ends in the middle of its scan
    return files, file_texts(8, JW, JH, 41)


def jpeg_wm_chain(f, text, w, h, quality=85):
    d = oracle.jpeg_decode(f)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    wm = oracle.draw_ycbcr(np.zeros((h, w, 4), np.uint8), (0, 0, w, h), np.ascontiguousarray(d["y"][:h, :w]),
                           np.ascontiguousarray(d["cb"][:ch, :cw]), np.ascontiguousarray(d["cr"][:ch, :cw]), 2)
    return oracle.jpeg_encode_rgba(oracle.composite_glyphs(wm, text[0], text[1]), quality)


@pytest.mark.parametrize("part,chunk", [("2", "3"), ("384", "3")], ids=["four-parts", "one-part-three-chunks"])
def test_jpeg_leg(ctx, jpeg_case, monkeypatch, part, chunk):
    files, texts = jpeg_case
    plan = ctx.plan(JW, JH, resize=RESIZE, thumbnail=THUMB, watermark=True)
    plain, plain_st = plan.run_jpeg_jpeg(files)
    monkeypatch.setenv("IPX_JPEG_JPEG_PART", part)
    monkeypatch.setenv("IPX_JPEG_JPEG_CHUNK", chunk)
    got, st = plan.run_jpeg_jpeg(files, texts=texts)
    assert st == plain_st and st[5] != 0 and [s for i, s in enumerate(st) if i != 5] == [0] * 7
    assert got["resize"] == plain["resize"] and got["thumbnail"] == plain["thumbnail"]
    for i in range(8):
        if st[i]:
            assert got["watermark"][i] is None
            continue
        assert got["watermark"][i] == jpeg_wm_chain(files[i], texts[i], JW, JH), "file %d does not carry its own text" % i
    # no watermark wanted, or no watermark operator: the texts are checked and nothing is drawn
    part_out, st2 = plan.run_jpeg_jpeg(files, texts=texts, want=("resize",))
    assert st2 == st and list(part_out) == ["resize"] and part_out["resize"] == plain["resize"]
    plan.close()
    bare = ctx.plan(JW, JH, resize=RESIZE, thumbnail=None)
    out3, st3 = bare.run_jpeg_jpeg(files, texts=texts)
    assert st3 == st and list(out3) == ["resize"] and out3["resize"] == plain["resize"]
    bare.close()


PW, PH = 48, 40


@pytest.fixture(scope="module")
def png_case():
    kinds = [(0, 8, False), (2, 8, False), (6, 8, False), (3, 8, True)]      # *image.Gray, RGBA, NRGBA, Paletted
    files = [pc.of_type(*kinds[i % 4], PH, PW, seed=500 + i, kind=("photo", "flat")[i % 2]) for i in range(7)]
    return files, file_texts(7, PW, PH, 43)


def png_wm_frame(f, text, w, h):
    r = pdm.decode(f, fast=True)
    assert r["status"] == pdm.OK
    rect, z = (0, 0, w, h), np.zeros((h, w, 4), np.uint8)
    if r["kind"] == pdm.GRAY:
        y = r["pix"].reshape(h, w)
        wm = np.ascontiguousarray(np.dstack([y, y, y, np.full_like(y, 255)]))
    elif r["kind"] == pdm.RGBA:
        wm = np.ascontiguousarray(r["pix"].reshape(h, w, 4))
    elif r["kind"] == pdm.NRGBA:
        wm = oracle.draw_nrgba(z, rect, np.ascontiguousarray(r["pix"].reshape(h, w, 4)))
    else:
        assert r["kind"] == pdm.PALETTED
        wm = oracle.draw_paletted(z, rect, r["pix"].reshape(h, w), oracle.palette16(r["palette"], "nrgba"))
    return oracle.composite_glyphs(wm, text[0], text[1])


def test_png_leg(ctx, png_case, monkeypatch):
    files, texts = png_case
    assert [pdm.decode(f, fast=True)["kind"] for f in files] == [pdm.GRAY, pdm.RGBA, pdm.NRGBA, pdm.PALETTED, pdm.GRAY, pdm.RGBA, pdm.NRGBA]
    monkeypatch.setenv("IPX_HOST_CHUNK_PNG", "2")
    plan = ctx.plan(PW, PH, resize=RESIZE, thumbnail=THUMB, watermark=True)
    got, st = plan.run_png_png(files, texts=texts)
    assert st == [0] * 7
    for i in range(7):
        want = png_wm_frame(files[i], texts[i], PW, PH)
        if not (want[..., 3] == 255).all():
            want = png_model.unpremultiply(want)             # what png.Encode stores for an *image.RGBA that is not opaque
        back = np.asarray(PIL.open(io.BytesIO(got["watermark"][i])).convert("RGBA"))
        assert np.array_equal(back, want), "file %d does not carry its own text" % i
    plan.close()
    monkeypatch.delenv("IPX_HOST_CHUNK_PNG")
    for i in range(7):                                       # the file alone, with a plan that carries its text
        gs = ctx.glyphset(texts[i][0], texts[i][1])
        alone = ctx.plan(PW, PH, resize=RESIZE, thumbnail=THUMB, watermark=gs)
        want, st1 = alone.run_png_png([files[i]])
        assert st1 == [0]
        for k in ("resize", "thumbnail", "watermark"):
            assert got[k][i] == want[k][0], (k, i)
        alone.close()
        gs.close()


@pytest.fixture(scope="module")
def gif_case():
    files = [gif_corpus.make(PW, PH, 800 + i, ("photo", "flat")[i % 2], interlace=bool(i % 2), transparency=(i == 3)) for i in range(5)]
    return files, file_texts(5, PW, PH, 47)


def gif_wm_chain(f, text, w, h, quality):
    r = gdm.decode(f)
    assert r["ok"]
    wm = oracle.draw_paletted(np.zeros((h, w, 4), np.uint8), (0, 0, w, h), r["index"], oracle.palette16(r["palette"], "rgba"))
    return oracle.jpeg_encode_rgba(oracle.composite_glyphs(wm, text[0], text[1]), quality)


def test_gif_leg(ctx, gif_case, monkeypatch):
    files, texts = gif_case
    plan = ctx.plan(PW, PH, resize=RESIZE, thumbnail=THUMB, watermark=True)
    plain, plain_st = plan.run_gif_gif(files, quality=80)
    monkeypatch.setenv("IPX_HOST_CHUNK_GIF", "2")
    got, st = plan.run_gif_gif(files, quality=80, texts=texts)
    assert st == plain_st == [0] * 5
    assert got["resize"] == plain["resize"] and got["thumbnail"] == plain["thumbnail"]
    for i in range(5):
        assert got["watermark"][i] == gif_wm_chain(files[i], texts[i], PW, PH, 80), "file %d does not carry its own text" % i
    plan.close()


def test_pool_jobs_with_texts(ipx, ctx, jpeg_case, png_case, gif_case, monkeypatch):
    plans = {(JW, JH): ctx.plan(JW, JH, resize=RESIZE, thumbnail=THUMB, watermark=True), (PW, PH): ctx.plan(PW, PH, resize=RESIZE, thumbnail=THUMB, watermark=True)}
    direct = {"jpeg": plans[(JW, JH)].run_jpeg_jpeg(jpeg_case[0], 85, texts=jpeg_case[1]), "png": plans[(PW, PH)].run_png_png(png_case[0], texts=png_case[1]),
              "gif": plans[(PW, PH)].run_gif_gif(gif_case[0], 85, texts=gif_case[1])}
    for p in plans.values():
        p.close()
    for name in ("IPX_POOL_JPEG_CHUNK", "IPX_POOL_PNG_CHUNK", "IPX_POOL_GIF_CHUNK"):
        monkeypatch.setenv(name, "3")
    with ipx.Pool(devices=(0,)) as pool:
        for fmt, (files, texts), (sw, sh) in (("jpeg", jpeg_case, (JW, JH)), ("png", png_case, (PW, PH)), ("gif", gif_case, (PW, PH))):
            got, st = pool.submit_files(files, sw, sh, fmt, 85, resize=RESIZE, thumbnail=THUMB, texts=texts).wait()
            assert st == direct[fmt][1], fmt
            assert sorted(got) == ["resize", "thumbnail", "watermark"]
            for k in got:
                assert got[k] == direct[fmt][0][k], (fmt, k)
        # texts go with file jobs, and with no glyphs in the operators
        with pytest.raises(ipx.IpxError) as e:
            pool.submit_files(jpeg_case[0], JW, JH, "jpeg", texts=jpeg_case[1], glyphs=jpeg_case[1][2][0])
        assert e.value.status == -1 and "ops.glyphs" in e.value.text
        j = pool.submit(rgba_frames(1, JW, JH), resize=RESIZE, thumbnail=None)
        j.wait()
        tarr = ipx._text_array(jpeg_case[1][:1])
        j.job.texts = tarr[0]
        t = C.c_uint64()
        assert ipx.lib().ipx_job_submit(pool.handle, C.byref(j.job), C.byref(t)) == -1 and b"file jobs only" in ipx.lib().ipx_last_error()


def _batch(ipx, files, texts, sw, sh):
    """24 single files from 8 threads, file i with text i % 8; every thread submits its three files before anybody waits"""
    got, errs = {}, []
    with ipx.Pool(devices=(0,)) as pool, ipx.Batcher(pool, max_batch=8, max_wait_us=20000, quality=85) as b:
        gate = threading.Barrier(8)

        def work(part):
            try:
                tickets = [(i, b.submit(files[i], sw, sh, resize=RESIZE, thumbnail=THUMB, glyphs=texts[i % 8][0], col=texts[i % 8][1], watermark=True))
                           for i in part]
                gate.wait(timeout=60)
                for i, t in tickets:
                    got[i] = b.wait(t)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e)[:300])
        ts = [threading.Thread(target=work, args=(range(k, 24, 8),)) for k in range(8)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        stats = b.stats()
    assert not errs, errs
    assert len(got) == 24 and stats["files"] == 24
    return got, stats


def test_batcher_with_a_text_per_file(ipx, ctx, monkeypatch):
    files = [_jpeg(rgba_frames(1, JW, JH, seed=900 + i)[0][..., :3] // 2 + 30, quality=80, subsampling=2) for i in range(24)]
    texts = file_texts(9, JW, JH, 53)[1:]                    # eight texts, none of them empty
    plan = ctx.plan(JW, JH, resize=RESIZE, thumbnail=THUMB, watermark=True)
    direct, direct_st = plan.run_jpeg_jpeg(files, 85, texts=[texts[i % 8] for i in range(24)])
    plan.close()
    assert direct_st == [0] * 24
    monkeypatch.setenv("IPX_BATCHER_IDLE_FLUSH", "0")        # size and timer only: what a group holds does not depend on who ran first
    monkeypatch.setenv("IPX_BATCH_TEXTS", "1")
    got, stats = _batch(ipx, files, texts, JW, JH)
    assert stats["largest_batch"] > 1 and stats["batches"] < 24, stats
    for i in range(24):
        assert got[i][0] == 0
        assert got[i][1] == {k: direct[k][i] for k in ("resize", "thumbnail", "watermark")}, "file %d: not the _texts leg's streams" % i
    for i in (0, 9, 18, 3, 12, 21, 6, 15):                   # one file per text, against the oracle chain
        assert got[i][1]["watermark"] == jpeg_wm_chain(files[i], texts[i % 8], JW, JH), "file %d does not carry its own text" % i
    assert sorted(i % 8 for i in (0, 9, 18, 3, 12, 21, 6, 15)) == list(range(8))
    # without the switch: groups by text as always, the streams of the entry with a plan that carries the text
    monkeypatch.delenv("IPX_BATCH_TEXTS")
    off, stats_off = _batch(ipx, files, texts, JW, JH)
    assert stats_off["largest_batch"] <= 3                    # three files per text
    for t in range(8):
        gs = ctx.glyphset(texts[t][0], texts[t][1])
        plan = ctx.plan(JW, JH, resize=RESIZE, thumbnail=THUMB, watermark=gs)
        want, st = plan.run_jpeg_jpeg([files[i] for i in range(t, 24, 8)], 85)
        for j, i in enumerate(range(t, 24, 8)):
            assert off[i][0] == st[j] == 0 and off[i][1] == {k: want[k][j] for k in want}, "file %d" % i
        plan.close()
        gs.close()
