"""GPU: the entries that take frames in HBM (and the host seam on views) on padded, offset and misaligned layouts.

Every frame stride, row stride and pointer of include/ipx.h's device entries picks a path: launch_ks_fused (csrc/ipx_ks_fused.hip) takes
a batch only when they pass its alignment gates, launch_palette_expand has a vector path, src_check refuses some.  Here the same pixels
go through every layout of tests/layout_cases.py; the expected bytes come from the float64 reference (tests/scaler_reference.py, within
the unchanged caps) and the oracle, which never see a layout; every padding and guard byte of every output allocation must stay 0xA5;
and which path ran is asserted against a table written from the gates (layout_cases.one_pass), so a gate that moves fails here."""

import numpy as np
import pytest

import layout_cases as L
import layout_expected as E
import oracle
import scaler_reference as R
from layout_cases import COL, N
from scaler_cases import DEEP, KINDS, RATIO, Source, cap

pytestmark = pytest.mark.gpu

KNOBS = ["IPX_FUSED", "IPX_KS_FAST", "IPX_KS_TAIL", "IPX_HOST_DIRECT"]
ENVS = [{}, {"IPX_KS_FAST": "0"}, {"IPX_KS_TAIL": "0"}]
OUT_KEYS = ("resize", "thumbnail", "watermark")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipa
    c = ipa.Context()
    yield c
    c.close()


class Dev:
    """named allocations in HBM that the cases of one test share (each 256-byte aligned, as hipMalloc gives them)"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, {}

    def put(self, name, arr):
        """the bytes of `arr` at the start of the allocation `name` -> its address"""
        b = self.bufs.get(name)
        if b is None or b.nbytes < arr.nbytes:
            if b is not None:
                b.free()
            b = self.bufs[name] = self.ctx.alloc(max(arr.nbytes, 1 << 16))
            assert b.ptr % 256 == 0
        b.upload(arr)
        return b.ptr

    def get(self, name, nbytes):
        return self.bufs[name].download((nbytes,))

    def close(self):
        for b in self.bufs.values():
            b.free()


@pytest.fixture()
def dev(ctx):
    d = Dev(ctx)
    yield d
    ctx.device_sync()
    d.close()


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("IPX_KS_DEBUG", "1")


def _one_pass_ran(capfd):
    """the library prints a line beginning "[ipx ks] src" exactly when the one-pass kernel took the batch (IPX_KS_DEBUG=1)"""
    return any(l.startswith("[ipx ks] src") for l in capfd.readouterr().err.splitlines())


def _both(got, want, ref, kind, what):
    R.assert_matches(got, *ref, max_ambiguous=cap(kind), what="%s %s" % (kind, what))
    np.testing.assert_array_equal(got, want, err_msg="%s %s: the kernel differs from the oracle" % (kind, what))


# ---- the batch plans on frames in HBM -------------------------------------------------------------------------------------------------

def _plan(ctx, shape, glyphs):
    w, h, resize, thumb, wm = shape
    gs = ctx.glyphset(glyphs, COL) if wm else None
    return ctx.plan(w, h, resize=resize, thumbnail=thumb, watermark=gs), gs


def _put_sources(dev, c, layout, chroma, pal_offset=0):
    """-> [(address, row stride, frame stride)] per plane, and the palettes' address or None"""
    planes, pal = c.planes()
    args = []
    for j, p in enumerate(planes):
        off, es, ef = layout if j == 0 or chroma is None else chroma
        buf, o, stride, fs = L.lay_out(p, es, ef, off)
        args.append((dev.put("src%d" % j, buf) + o, stride, fs))
    pp = None
    if pal is not None:
        pp = dev.put("pal", np.concatenate([np.full(pal_offset, L.FILL, np.uint8), pal.reshape(-1)])) + pal_offset
    return args, pp


def _put_outputs(dev, plan, c, out_layouts):
    """out_layouts: one (offset, extra frame stride) for all outputs, or {output: layout} -> {output: (address, frame stride, (bytes of
    the allocation, first, frame bytes, shape))}"""
    i = plan.info
    outs = {}
    for k, fb, shape in (("resize", i.resize_bytes, (i.resize_h, i.resize_w, 4)), ("thumbnail", i.thumb_bytes, (i.thumb_h, i.thumb_w, 4)),
                         ("watermark", i.wm_bytes, (i.wm_h, i.wm_w, 4))):
        if k not in c.keys:
            continue
        lay = out_layouts.get(k, L.OUT_TIGHT) if isinstance(out_layouts, dict) else out_layouts
        buf, first, fs = L.out_alloc(N, fb, *lay)
        outs[k] = (dev.put("out_" + k, buf) + first, fs, (buf.size, first, fb, shape))
    return outs


def _call(plan, c, src, pal, outs, stream=None):
    k = c.kind
    o = {key: outs[key][0] if key in outs else None for key in OUT_KEYS}
    kw = dict(resize_ptr=o["resize"], thumb_ptr=o["thumbnail"], wm_ptr=o["watermark"], stream=stream,
              resize_frame_stride=outs["resize"][1] if "resize" in outs else None,
              thumb_frame_stride=outs["thumbnail"][1] if "thumbnail" in outs else None,
              wm_frame_stride=outs["watermark"][1] if "watermark" in outs else None)
    p, stride, fs = src[0]
    if k == "rgba":
        plan.run_dev(N, p, sstride=stride, src_frame_stride=fs, **kw)
    elif k == "nrgba":
        plan.run_dev_nrgba(N, p, sstride=stride, src_frame_stride=fs, **kw)
    elif k == "gray":
        plan.run_dev_gray(N, p, stride, fs, **kw)
    elif k.startswith("ycbcr"):
        assert src[1][1:] == src[2][1:]
        plan.run_dev_ycbcr(N, p, src[1][0], src[2][0], RATIO[k], stride, src[1][1], fs, src[1][2], **kw)
    elif k.startswith("paletted"):
        plan.run_dev_paletted(N, p, stride, fs, pal, **kw)
    else:
        plan.run_dev_deep(N, DEEP[k], p, stride, fs, **kw)


def _take_outputs(ctx, dev, outs, what):
    """-> {output: n x h x w x 4}, having checked every byte outside the frames"""
    ctx.sync()
    return {k: L.out_frames(dev.get("out_" + k, size), N, fb, first, fs, shape, "%s %s" % (what, k))
            for k, (_, fs, (size, first, fb, shape)) in outs.items()}


def _check_outputs(c, got, what):
    for i in range(N):
        for k in c.keys:
            w = "%s frame %d %s" % (k, i, what)
            if k == "watermark":      # the copy (drawRGBA's Src: the top bytes) and the text, exact integer arithmetic both
                np.testing.assert_array_equal(got[k][i], c.want_text[i], err_msg="%s %s: differs from the oracle" % (c.kind, w))
            else:
                _both(got[k][i], c.want[i][k], c.ref[i][k], c.kind, w)


def _untouched(ctx, dev, outs, what):
    ctx.sync()
    for k, (_, _, (size, *_)) in outs.items():
        assert (dev.get("out_" + k, size) == L.FILL).all(), "%s: the refused call wrote into the %s allocation" % (what, k)


def _run(ctx, dev, plan, c, layout, chroma, out_layout, what):
    src, pal = _put_sources(dev, c, layout, chroma)
    outs = _put_outputs(dev, plan, c, out_layout)
    _call(plan, c, src, pal, outs)
    _check_outputs(c, _take_outputs(ctx, dev, outs, what), what)


def combos(kind):
    """-> [(source layout, chroma layout | None, output layout)]"""
    lays = L.kind_layouts(kind)
    if kind in L.FULL_KINDS:
        return ([(l, ch, o) for l, ch in lays for o in (L.OUT_TIGHT, L.OUT_PADDED)] +
                [(L.TIGHT, None, o) for o in L.OUT_LAYOUTS if o not in (L.OUT_TIGHT, L.OUT_PADDED)])
    return [(l, ch, L.OUT_TIGHT if l == L.TIGHT and ch is None else L.OUT_PADDED) for l, ch in lays]


@pytest.mark.parametrize("kind", KINDS)
def test_batch_layouts(ctx, dev, kind, monkeypatch, capfd):
    """Every layout the kind runs, at every shape and under the three kernel-path environments: the outputs match the reference and
    the oracle, no byte outside the output frames is written, and the batch ran where the gates of launch_ks_fused send it."""
    for shape in L.SHAPES:
        c = E.case(kind, shape)
        plan, gs = _plan(ctx, shape, c.glyphs)
        try:
            for env in ENVS + [{"IPX_FUSED": "0"}]:
                _env(monkeypatch, env)
                runs = combos(kind) if "IPX_FUSED" not in env else [(L.MOST_PADDED, None, L.OUT_PADDED)]
                for layout, chroma, out_layout in runs:
                    what = "%r source %r chroma %r outputs %r %r" % (shape[:2], layout, chroma, out_layout, env)
                    capfd.readouterr()
                    _run(ctx, dev, plan, c, layout, chroma, out_layout, what)
                    assert _one_pass_ran(capfd) == L.one_pass(kind, shape, layout, chroma, env), \
                        "%s %s: the one-pass kernel %s" % (kind, what, "should have run" if L.one_pass(kind, shape, layout, chroma, env) else "should not have run")
        finally:
            plan.close()
            if gs:
                gs.close()


# ---- what the entries refuse, before any launch ----------------------------------------------------------------------------------------

def _refused(fn, what):
    import imageprocessor_amd as ipa
    with pytest.raises(ipa.IpxError) as e:
        fn()
    assert e.value.status == -1, "%s: status %d (%s), not IPX_ERR_INVALID" % (what, e.value.status, e.value.text)
    return e.value.text


@pytest.mark.parametrize("kind", ["rgba", "nrgba", "gray", "ycbcr420", "paletted-gif", "nrgba64"])     # one kind per device entry
def test_outputs_off_a_dword_are_refused(ctx, dev, kind, monkeypatch, capfd):
    """include/ipx.h: the address and the frame stride of every output in HBM are multiples of 4 (the kernels store whole pixels, the
    one-pass kernel four at a time, through buffer descriptors built at that address); anything else is IPX_ERR_INVALID, decided on
    the host: nothing is launched, nothing is written, and the next legal call is correct."""
    _env(monkeypatch, {})
    shape = L.SHAPES[0]
    c = E.case(kind, shape)
    plan, gs = _plan(ctx, shape, c.glyphs)
    try:
        for key in OUT_KEYS:
            for lay in L.OUT_REFUSED:
                what = "%s %s at %r" % (kind, key, lay)
                src, pal = _put_sources(dev, c, L.TIGHT, None)
                outs = _put_outputs(dev, plan, c, {key: lay})
                capfd.readouterr()
                text = _refused(lambda: _call(plan, c, src, pal, outs), what)
                assert key in text and "multiples of 4" in text, text
                assert "[ipx ks]" not in capfd.readouterr().err, "%s: something was launched" % what
                _untouched(ctx, dev, outs, what)
        _run(ctx, dev, plan, c, L.TIGHT, None, L.OUT_PADDED, "after the refusals")
    finally:
        plan.close()
        gs.close()


def test_sources_the_expansions_cannot_read_are_refused(ctx, dev, monkeypatch):
    """src_check (csrc/ipx_runtime.hip): the deep types are read a whole 16-bit sample (CMYK: a whole pixel) at a time, the palettes a
    whole entry: an address, row stride or frame stride off that is IPX_ERR_INVALID; the outputs stay untouched and the next legal
    call is correct."""
    _env(monkeypatch, {})
    shape = L.SHAPES[0]
    bad = {"nrgba64": [(1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 2, 2)], "rgba64": [(1, 0, 0)], "gray16": [(0, 1, 0), (0, 0, 3)],
           "cmyk": [(2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 0, 0), (0, 4, 1)]}
    for kind, layouts in bad.items():
        c = E.case(kind, shape)
        plan, gs = _plan(ctx, shape, c.glyphs)
        try:
            for layout in layouts:
                src, pal = _put_sources(dev, c, layout, None)
                outs = _put_outputs(dev, plan, c, L.OUT_PADDED)
                _refused(lambda: _call(plan, c, src, pal, outs), "%s at %r" % (kind, layout))
                _untouched(ctx, dev, outs, "%s at %r" % (kind, layout))
            _run(ctx, dev, plan, c, (4, 4, 4) if kind == "cmyk" else (2, 2, 2), None, L.OUT_PADDED, "after the refusals")
        finally:
            plan.close()
            gs.close()
    for kind in ("paletted-gif", "paletted-trns"):
        c = E.case(kind, shape)
        plan, gs = _plan(ctx, shape, c.glyphs)
        try:
            for pal_offset in (1, 2, 3):
                src, pal = _put_sources(dev, c, L.TIGHT, None, pal_offset)
                outs = _put_outputs(dev, plan, c, L.OUT_PADDED)
                _refused(lambda: _call(plan, c, src, pal, outs), "%s palettes at +%d" % (kind, pal_offset))
                _untouched(ctx, dev, outs, "%s palettes at +%d" % (kind, pal_offset))
            src, pal = _put_sources(dev, c, (1, 1, 1), None, 4)       # palettes 4-byte aligned and no more: legal
            outs = _put_outputs(dev, plan, c, L.OUT_PADDED)
            _call(plan, c, src, pal, outs)
            _check_outputs(c, _take_outputs(ctx, dev, outs, "palettes at +4"), "palettes at +4")
        finally:
            plan.close()
            gs.close()


# ---- the per-operation seam on frames in HBM -------------------------------------------------------------------------------------------

def _premultiplied(rng, h, w):
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    a[..., :3] = np.minimum(a[..., :3], a[..., 3:4])
    return a


class Window:
    """A dw x dh destination frame that is a window of a larger random (premultiplied) frame, itself laid out at an offset and with
    padded rows: what the entry may write is the window's pixels and nothing else."""

    def __init__(self, dev, name, dw, dh, seed, offset=4, extra_stride=20, at=(5, 3), margin=(9, 7)):
        rng = np.random.default_rng(seed)
        self.dev, self.name, self.dw, self.dh = dev, name, dw, dh
        self.big = _premultiplied(rng, dh + margin[1], dw + margin[0])
        self.buf, self.off, self.stride, _ = L.lay_out(self.big[None], extra_stride, 0, offset)
        self.at = at
        self.start = self.off + at[1] * self.stride + at[0] * 4
        self.ptr = dev.put(name, self.buf) + self.start
        self.before = self.big[at[1]:at[1] + dh, at[0]:at[0] + dw].copy()

    def after(self, ctx, what):
        """-> the window after the call; every byte of the allocation outside it is as it was"""
        ctx.sync()
        got = self.dev.get(self.name, self.buf.size)
        win = np.lib.stride_tricks.as_strided(got[self.start:], (self.dh, self.dw * 4), (self.stride, 1)).copy()
        was = self.buf.copy()
        np.lib.stride_tricks.as_strided(was[self.start:], (self.dh, self.dw * 4), (self.stride, 1))[...] = win
        np.testing.assert_array_equal(got, was, err_msg="%s: bytes outside the destination window changed" % what)
        return win.reshape(self.dh, self.dw, 4)


# source layouts of the seam: (offset, extra row stride); the last two are off a dword (include/ipx.h: served)
SEAM_SRC = [(8, 12), (0, 0), (1, 0), (4, 2)]


@pytest.mark.parametrize("size", [(61, 47), (104, 61)])
def test_device_seam_on_windows(ctx, dev, size, monkeypatch):
    """ipx_dev_scale_bilinear_rgba8 and ipx_dev_draw_rgba8 with both ops, strides wider than the rows, rectangles strictly inside the
    frames, onto a window of a larger frame; ipx_dev_composite_glyphs_rgba8 onto the same kind of window."""
    _env(monkeypatch, {})
    sw, sh = size
    src = Source("rgba", sw, sh, seed=sw + sh)
    dw, dh = sw * 2 // 3 + 1, sh * 2 // 3
    dr, sr = (2, 1, dw - 3, dh - 2), (3, 2, sw - 1, sh - 3)
    for off, es in SEAM_SRC:
        sbuf, so, sstride, _ = L.lay_out(src.data[None], es, 0, off)
        sp = dev.put("src", sbuf) + so
        for op in (oracle.OP_OVER, oracle.OP_SRC):
            what = "%r source at %r op %d" % (size, (off, es), op)
            win = Window(dev, "dst", dw, dh, seed=op + 10)
            ctx.dev_scale_bilinear(win.ptr, dw, dh, win.stride, dr, sp, sw, sh, sstride, sr, op=op)
            got = win.after(ctx, "scale " + what)
            want = oracle.scale_bilinear(src.data, dw, dh, sr=sr, dr=dr, op=op, dst=win.before.copy())
            np.testing.assert_array_equal(got, want, err_msg="scale %s: differs from the oracle" % what)
            sub = win.before[dr[1]:dr[3], dr[0]:dr[2]]      # Scale(dst, dr, ...) with dr inside dst is the scale onto dst's sub-image at dr
            ref = R.scale(src.ref, dr[2] - dr[0], dr[3] - dr[1], sr=sr, op=op, dst=sub)
            R.assert_matches(got[dr[1]:dr[3], dr[0]:dr[2]], *ref, max_ambiguous=cap("rgba"), what="scale " + what)

            win = Window(dev, "dst", dw, dh, seed=op + 20)
            r, spt = (4, 2, dw - 2, dh - 1), (3, 5)
            ctx.dev_draw(win.ptr, dw, dh, win.stride, r, sp, sw, sh, sstride, sp=spt, op=op)
            got = win.after(ctx, "draw " + what)
            np.testing.assert_array_equal(got, oracle.draw(win.before.copy(), r, src.data, spt, op), err_msg="draw %s: differs from the oracle" % what)
            R.assert_matches(got, *R.draw(win.before, r, src.ref, spt, op), max_ambiguous=cap("rgba"), what="draw " + what)

    # everything a multiple of 16 -- both addresses after the rectangle's and the source point's offsets, both strides -- and a
    # width that is a multiple of 4: ipx_dev_draw_rgba8 with Src copies 16 bytes per lane (launch_draw's gate, csrc/ipx_kernels.hip)
    sbuf, so, sstride, _ = L.lay_out(src.data[None], (-sw * 4) % 16, 0, 0)
    sp = dev.put("src", sbuf)
    win = Window(dev, "dst", dw, dh, seed=50, offset=0, extra_stride=(-(dw + 9) * 4) % 16, at=(4, 3))
    r, spt = (4, 2, 4 + 4 * ((dw - 6) // 4), dh - 1), (4, 5)
    assert sstride % 16 == 0 and win.stride % 16 == 0 and win.start % 16 == 0 and (r[2] - r[0]) % 4 == 0
    ctx.dev_draw(win.ptr, dw, dh, win.stride, r, sp, sw, sh, sstride, sp=spt, op=oracle.OP_SRC)
    got = win.after(ctx, "16-byte draw %r" % (size,))
    np.testing.assert_array_equal(got, oracle.draw(win.before.copy(), r, src.data, spt, oracle.OP_SRC), err_msg="16-byte draw %r" % (size,))

    glyphs = L.corner_glyphs(dw, dh)
    gs = ctx.glyphset(glyphs, COL)
    try:
        win = Window(dev, "dst", dw, dh, seed=30)
        ctx.dev_composite_glyphs(win.ptr, dw, dh, win.stride, gs)
        got = win.after(ctx, "composite %r" % (size,))
        np.testing.assert_array_equal(got, oracle.composite_glyphs(win.before.copy(), glyphs, COL))
        # a destination off a dword: refused, nothing written
        for name, call in (("scale", lambda p, st: ctx.dev_scale_bilinear(p, dw, dh, st, dr, sp, sw, sh, sstride, sr)),
                           ("draw", lambda p, st: ctx.dev_draw(p, dw, dh, st, dr, sp, sw, sh, sstride)),
                           ("composite", lambda p, st: ctx.dev_composite_glyphs(p, dw, dh, st, gs))):
            for offset, es in ((1, 20), (4, 22), (2, 21)):
                win = Window(dev, "dst", dw, dh, seed=40, offset=offset, extra_stride=es)
                assert "multiples of 4" in _refused(lambda: call(win.ptr, win.stride), "%s onto %r" % (name, (offset, es)))
                np.testing.assert_array_equal(win.after(ctx, name), win.before)
    finally:
        gs.close()


# ---- the host seam on views: a SubImage's Pix starts mid-allocation and its Stride is wider than its rows ------------------------------

def _window_of(a, rng, before, after, row_before, row_after):
    """`a` (H x row...) as a window of a larger random array: `before` / `after` whole rows around it, row_before / row_after elements
    of the second axis around each row -> (the view, the larger array)"""
    h = a.shape[0]
    big = rng.integers(0, 256, (h + before + after, a.shape[1] + row_before + row_after) + a.shape[2:], dtype=np.uint8)
    view = big[before:before + h, row_before:row_before + a.shape[1]]
    view[...] = a
    return view, big


def _unchanged_outside(big, was, view_slices, what):
    mask = np.ones(big.shape, bool)
    mask[view_slices] = False
    assert (big[mask] == was[mask]).all(), "%s: bytes outside the destination window changed" % what


HOST_KINDS = ["rgba", "nrgba", "nrgba64", "gray16", "cmyk", "ycbcr420", "ycbcr444"]


@pytest.mark.parametrize("kind", HOST_KINDS)
def test_host_seam_on_views(ctx, kind, monkeypatch):
    """Context.scale_bilinear* / draw* with a destination and a source that are windows of larger arrays: the result equals the call
    on packed copies and the oracle, and no byte outside the destination window changes."""
    _env(monkeypatch, {})
    rng = np.random.default_rng(len(kind))
    sw, sh, dw, dh = 61, 47, 40, 29
    src = Source(kind, sw, sh, seed=3)
    sr, dr, r, sp = (2, 1, sw - 3, sh - 2), (1, 2, dw - 2, dh - 1), (3, 2, dw - 1, dh - 2), (4, 3)
    under = _premultiplied(rng, dh, dw)
    yc = kind.startswith("ycbcr")
    if yc:        # planes of bytes: odd offsets and strides
        views = [_window_of(p, rng, 2, 1, o, 6)[0] for p, o in zip(src.data[:3], (3, 5, 5))]
        packed = tuple(np.ascontiguousarray(v) for v in views) + (src.data[3],)
        sargs = tuple(views) + (src.data[3],)
    elif kind in DEEP:   # Pix rows: an offset that is a multiple of the pixel; Gray16 in host memory also at an odd byte
        bpp = {"gray16": 2, "cmyk": 4}.get(kind, 8)
        view = _window_of(src.data, rng, 1, 2, bpp if kind != "gray16" else 3, 10)[0]
        packed, sargs = (np.ascontiguousarray(view), DEEP[kind]), (view, DEEP[kind])
    else:
        view = _window_of(src.data, rng, 1, 2, 3, 2)[0]
        packed, sargs = (np.ascontiguousarray(view),), (view,)
    scale = {"rgba": ctx.scale_bilinear, "nrgba": ctx.scale_bilinear_nrgba}.get(kind, ctx.scale_bilinear_ycbcr if yc else ctx.scale_bilinear_deep)
    draw = {"rgba": ctx.draw, "nrgba": ctx.draw_nrgba}.get(kind, ctx.draw_ycbcr if yc else ctx.draw_deep)
    for op in ((oracle.OP_OVER,) if yc else (oracle.OP_OVER, oracle.OP_SRC)):
        kw = {} if yc else {"op": op}
        what = "%s op %d" % (kind, op)
        dview, big = _window_of(under, rng, 3, 2, 2, 5)
        was = big.copy()
        got = scale(*sargs, dw, dh, sr=sr, dr=dr, dst=dview, **kw)
        assert got is dview
        np.testing.assert_array_equal(dview, scale(*packed, dw, dh, sr=sr, dr=dr, dst=under.copy(), **kw), err_msg="scale " + what)
        full = src.oracle_scale(dr[2] - dr[0], dr[3] - dr[1], sr=sr, op=op, dst=under[dr[1]:dr[3], dr[0]:dr[2]])
        np.testing.assert_array_equal(dview[dr[1]:dr[3], dr[0]:dr[2]], full, err_msg="scale %s: differs from the oracle" % what)
        _unchanged_outside(big, was, (slice(3, 3 + dh), slice(2, 2 + dw)), "scale " + what)

        dview, big = _window_of(under, rng, 1, 4, 7, 1)
        was = big.copy()
        if yc:
            draw(dview, r, *sargs, sp=sp)
            want = draw(under.copy(), r, *packed, sp=sp)
        else:
            draw(dview, r, *sargs, sp=sp, op=op)
            want = draw(under.copy(), r, *packed, sp=sp, op=op)
        np.testing.assert_array_equal(dview, want, err_msg="draw " + what)
        np.testing.assert_array_equal(dview, src.oracle_draw(under, r, sp, op if not yc else oracle.OP_SRC), err_msg="draw %s: differs from the oracle" % what)
        _unchanged_outside(big, was, (slice(1, 1 + dh), slice(7, 7 + dw)), "draw " + what)


def test_host_glyphs_on_views(ctx, monkeypatch):
    """Context.composite_glyphs onto a window of a larger frame, from masks that are windows of larger masks (mstride > mw)"""
    _env(monkeypatch, {})
    rng = np.random.default_rng(8)
    dw, dh = 61, 47
    under = _premultiplied(rng, dh, dw)
    glyphs = L.corner_glyphs(dw, dh)
    strided = [dict(g, mask=_window_of(g["mask"], rng, 1, 1, 3, 2)[0]) for g in glyphs]
    assert all(not g["mask"].flags.c_contiguous for g in strided)
    dview, big = _window_of(under, rng, 2, 3, 1, 6)
    was = big.copy()
    ctx.composite_glyphs(dview, strided, COL)
    np.testing.assert_array_equal(dview, oracle.composite_glyphs(under.copy(), glyphs, COL))
    np.testing.assert_array_equal(dview, ctx.composite_glyphs(under.copy(), glyphs, COL))
    _unchanged_outside(big, was, (slice(2, 2 + dh), slice(1, 1 + dw)), "composite")
    gs = ctx.glyphset(strided, COL)           # the device glyph set takes the same strided masks
    gs.close()


# ---- host batches into pinned outputs with gaps between the frames ---------------------------------------------------------------------

# (shape, frames, extra frame stride, do the kernels store straight into the outputs when IPX_HOST_DIRECT allows?)  run_host_packed
# (csrc/ipx_runtime.hip) does so only when every output pointer and frame stride is a multiple of 16.  The frames of SHAPES[0] are
# 6240, 2304 and 25376 bytes, all multiples of 16: + 16 keeps that, + 4 breaks it.  HOST_GAP_SHAPE's resize frame is 1500 bytes, which the
# lanes' scratch pads to 1536; outputs at that same stride are multiples of 16 again (direct), and with IPX_HOST_DIRECT=0 they are the
# case in which the download must not run over the gaps: host and scratch strides equal, larger than a frame, several frames per
# chunk -- a chunk is ceil(n / (4 * lanes)) frames, so 40 frames give chunks of two and more on the default context.
HOST_GAP_CASES = [(L.SHAPES[0], N, 16, True), (L.SHAPES[0], N, 4, False), (L.HOST_GAP_SHAPE, 40, "to 256", True)]


def _direct_ran(capfd):
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[ipx host] outputs")]
    assert len(lines) == 1, lines
    return "stored by the kernels" in lines[0]


@pytest.mark.parametrize("direct", ["1", "0"])
def test_host_batch_outputs_with_gaps(ctx, direct, monkeypatch, capfd):
    """ipx_plan_run_host into pinned outputs with gaps between the frames, on the kernel-stored path and on the copied one (which of
    the two ran is asserted): the frames are correct and the gaps and guards stay 0xA5."""
    import imageprocessor_amd as ipa
    _env(monkeypatch, {"IPX_HOST_DIRECT": direct})
    for shape, n, extra, aligned16 in HOST_GAP_CASES:
        c = E.case("rgba", shape)
        plan, gs = _plan(ctx, shape, c.glyphs)
        frames = np.stack([c.srcs[j % N].data for j in range(n)])       # the case's N sources, tiled over the batch
        i = plan.info
        sizes = {"resize": (i.resize_bytes, (i.resize_h, i.resize_w, 4)), "thumbnail": (i.thumb_bytes, (i.thumb_h, i.thumb_w, 4)),
                 "watermark": (i.wm_bytes, (i.wm_h, i.wm_w, 4))}
        what = "IPX_HOST_DIRECT=%s %r, %d frames, frame stride + %s" % (direct, shape[:3], n, extra)
        pinned, outs = [], {}
        try:
            for k, (fb, shp) in sizes.items():
                buf, first, fs = L.out_alloc(n, fb, 0, (-fb) % 256 if extra == "to 256" else extra)
                arr = ctx.host_alloc(buf.shape)
                arr[...] = buf
                pinned.append(arr)
                outs[k] = (arr, first, fs, fb, shp)
            assert all(fs % 16 == 0 for _, _, fs, _, _ in outs.values()) == aligned16 and all(a.ctypes.data % 16 == 0 for a in pinned)
            capfd.readouterr()
            plan._run(ipa.lib().ipx_plan_run_host, (), n, (frames.ctypes.data, shape[0] * 4, shape[0] * shape[1] * 4),
                      [outs[k][0].ctypes.data + outs[k][1] for k in OUT_KEYS], [outs[k][2] for k in OUT_KEYS])
            assert _direct_ran(capfd) == (aligned16 and direct == "1"), what
            got = {k: L.out_frames(arr, n, fb, first, fs, shp, "%s %s" % (what, k)) for k, (arr, first, fs, fb, shp) in outs.items()}
        finally:
            for arr in pinned:
                ctx.host_free(arr)
            plan.close()
            gs.close()
        for j in range(n):
            for k in OUT_KEYS:
                w = "%s frame %d %s" % (k, j, what)
                if k == "watermark":
                    np.testing.assert_array_equal(got[k][j], c.want_text[j % N], err_msg=w)
                else:
                    _both(got[k][j], c.want[j % N][k], c.ref[j % N][k], "rgba", w)


# ---- the output stage the pixel-out host legs share (csrc/ipx_runtime.hip: DstLayout, dst_direct, dst_download) ------------------------
# run_host_packed above, the pool's pixel chunks and ipx_plan_run_host_ycbcr place, store and download a batch's outputs by one piece of
# code; these hold the other two legs, and run_host_packed's single-frame path, to what test_host_batch_outputs_with_gaps asks.

def _sizes(plan):
    i = plan.info
    return {"resize": (i.resize_bytes, (i.resize_h, i.resize_w, 4)), "thumbnail": (i.thumb_bytes, (i.thumb_h, i.thumb_w, 4)),
            "watermark": (i.wm_bytes, (i.wm_h, i.wm_w, 4))}


def _check_host_outputs(c, got, n, what):
    for j in range(n):
        for k in got:
            w = "%s frame %d %s" % (k, j, what)
            if k == "watermark":
                np.testing.assert_array_equal(got[k][j], c.want_text[j % N], err_msg=w)
            else:
                _both(got[k][j], c.want[j % N][k], c.ref[j % N][k], c.kind, w)


@pytest.fixture(scope="module")
def pool():
    import imageprocessor_amd as ipa
    p = ipa.Pool(devices=(0,))
    yield p
    p.close()


def _submit_pixels(pool, frames, shape, glyphs, outs):
    """The ipx_job of Pool.submit for RGBA frames, with the caller's output addresses and frame strides: {output: (address, stride)}"""
    import imageprocessor_amd as ipa
    from imageprocessor_amd import _lib
    w, h, resize, thumb, wm = shape
    ops, keep = pool._ops(w, h, resize, thumb, glyphs, COL, wm)
    j = _lib.Job()
    j.kind, j.ops, j.n = pool.JOB_KINDS["rgba"][0], ops, frames.shape[0]
    j.src, j.sstride, j.src_frame_stride = frames.ctypes.data, w * 4, w * h * 4
    j.resize_out, j.resize_frame_stride = outs["resize"]
    j.thumb_out, j.thumb_frame_stride = outs["thumbnail"]
    j.wm_out, j.wm_frame_stride = outs["watermark"]
    return ipa.PoolJob(pool, j, {"frames": frames, "glyphs": keep}, None, frames.shape[0])


# (shape, frames, pinned?, extra frame stride): + 16 keeps every pointer and stride of SHAPES[0] on 16 bytes and + 4 breaks that, as in
# HOST_GAP_CASES; 40 frames go in several chunks of several frames; pageable outputs are always downloaded
POOL_GAP_CASES = [(L.SHAPES[0], N, True, 16), (L.SHAPES[0], N, True, 4), (L.SHAPES[0], N, False, 20),
                  (L.HOST_GAP_SHAPE, 40, True, "to 256"), (L.HOST_GAP_SHAPE, 40, False, 20)]


@pytest.mark.parametrize("direct", ["1", "0"])
def test_pool_pixel_outputs_with_gaps(ctx, pool, direct, monkeypatch):
    """Pixel jobs of the pool into outputs with gaps between the frames -- pinned on and off the 16-byte gate, pageable -- with the
    kernels allowed to store into pinned outputs and not: the frames are correct (the text reaches the watermark's last row and
    column) and the gaps and guards stay 0xA5.  (The pool does not say which path ran: bytes only.)"""
    _env(monkeypatch, {"IPX_HOST_DIRECT": direct})
    for shape, n, pinned, extra in POOL_GAP_CASES:
        c = E.case("rgba", shape)
        plan, gs = _plan(ctx, shape, c.glyphs)        # (for the sizes of the outputs)
        sizes = _sizes(plan)
        plan.close()
        gs.close()
        frames = np.stack([c.srcs[j % N].data for j in range(n)])
        what = "pool IPX_HOST_DIRECT=%s %r, %d frames, %s outputs, frame stride + %s" % (direct, shape[:3], n, "pinned" if pinned else "pageable", extra)
        held, outs = [], {}
        try:
            for k, (fb, shp) in sizes.items():
                buf, first, fs = L.out_alloc(n, fb, 0, (-fb) % 256 if extra == "to 256" else extra)
                arr = pool.host_alloc(0, buf.shape) if pinned else np.empty_like(buf)
                arr[...] = buf
                held.append(arr)
                outs[k] = (arr, first, fs, fb, shp)
            _submit_pixels(pool, frames, shape, c.glyphs, {k: (o[0].ctypes.data + o[1], o[2]) for k, o in outs.items()}).wait()
            got = {k: L.out_frames(arr, n, fb, first, fs, shp, "%s %s" % (what, k)) for k, (arr, first, fs, fb, shp) in outs.items()}
        finally:
            for arr in held:
                pool.host_free(arr)       # (a pageable array: nothing to free)
        _check_host_outputs(c, got, n, what)


@pytest.mark.parametrize("out_layout", [L.OUT_TIGHT, (16, 32), L.OUT_PADDED])
def test_ycbcr_host_batch_outputs_with_gaps(ctx, out_layout, monkeypatch):
    """ipx_plan_run_host_ycbcr into pageable outputs at an offset and with gaps between the frames: the frames are correct and the gaps
    and guards stay 0xA5."""
    import ctypes as C
    import imageprocessor_amd as ipa
    from imageprocessor_amd import _lib
    _env(monkeypatch, {})
    kind, shape = "ycbcr420", L.SHAPES[0]
    c = E.case(kind, shape)
    (y, cb, cr), _ = c.planes()
    b = _lib.YCbCrBatch(y.ctypes.data, cb.ctypes.data, cr.ctypes.data, y.shape[2], cb.shape[2], y.shape[1] * y.shape[2],
                        cb.shape[1] * cb.shape[2], RATIO[kind])
    plan, gs = _plan(ctx, shape, c.glyphs)
    try:
        what = "%s outputs at %r" % (kind, out_layout)
        outs = {k: L.out_alloc(N, fb, *out_layout) + (fb, shp) for k, (fb, shp) in _sizes(plan).items()}
        args = [a for k in OUT_KEYS for a in (outs[k][0].ctypes.data + outs[k][1], outs[k][2])]
        ipa._check(ipa.lib().ipx_plan_run_host_ycbcr(ctx.handle, plan.handle, N, C.byref(b), *args))
        got = {k: L.out_frames(buf, N, fb, first, fs, shp, "%s %s" % (what, k)) for k, (buf, first, fs, fb, shp) in outs.items()}
    finally:
        plan.close()
        gs.close()
    _check_host_outputs(c, got, N, what)


@pytest.mark.parametrize("shape", [L.SHAPES[0], L.HOST_GAP_SHAPE], ids=["shape0", "gap-shape"])
def test_single_pageable_frame_by_operator_subset(ctx, shape, monkeypatch, capfd):
    """One pageable frame through ipx_plan_run_host into pageable outputs -- run_host_packed's bounce through a pinned buffer of the
    lane, where the three outputs come down with one copy -- wanting each non-empty subset of the plan's outputs: the wanted ones are
    correct between guards of 0xA5.  (HOST_GAP_SHAPE's resize frame of 1500 bytes is padded to 1536 in scratch: the offsets of the
    outputs behind it are not sums of frame bytes.)"""
    import imageprocessor_amd as ipa
    _env(monkeypatch, {})
    c = E.case("rgba", shape)
    frame = c.srcs[0].data[None].copy()
    plan, gs = _plan(ctx, shape, c.glyphs)
    try:
        sizes = _sizes(plan)
        for bits in range(1, 8):
            keys = [k for b, k in enumerate(OUT_KEYS) if bits >> b & 1]
            what = "one frame %r wanting %s" % (shape[:3], "+".join(keys))
            outs = {k: L.out_alloc(1, sizes[k][0], 0, 0) for k in keys}
            capfd.readouterr()
            plan._run(ipa.lib().ipx_plan_run_host, (), 1, (frame.ctypes.data, shape[0] * 4, shape[0] * shape[1] * 4),
                      [outs[k][0].ctypes.data + outs[k][1] if k in outs else None for k in OUT_KEYS])
            assert not _direct_ran(capfd), what
            got = {k: L.out_frames(buf, 1, sizes[k][0], first, fs, sizes[k][1], "%s %s" % (what, k)) for k, (buf, first, fs) in outs.items()}
            _check_host_outputs(c, got, 1, what)
    finally:
        plan.close()
        gs.close()
