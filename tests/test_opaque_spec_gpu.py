"""GPU: RGBA frames that ONE pixel gives away as not opaque (tests/opaque_cases.py), byte for byte against the oracle, whose bytes
tests/test_opaque_cases.py holds to the float64 reference on the CPU.

The speculative opaque pass of the one-pass scaler (csrc/ipx_ks_fused.hip) runs every item with three channels and ANDs the alpha
bytes it stages.  An item that sees alpha != 0xff in its first four rows leaves at once; one that sees it later runs to its end --
three-channel bytes stored, undecided pixels appended to the frame's lists -- and only then raises its flag.  Every other
non-opaque frame of the suite shows its alpha in the first rows and in every column, so here are
  * the late exit, with list entries, ahead of the redo pass and the tail launch, in either order (IPX_KS_TAIL=0);
  * frames of which some items are redone and their neighbours keep three-channel bytes;
  * detection in the ragged last chunk, in apron rows, in the columns a strip stages outside its own, in rows past the first group;
  * the whole-image alpha scans of the per-operation scalers and png.Encode's opacity scan on one off pixel."""
import re

import numpy as np
import pytest

import opaque_cases as OC
import oracle
import png_model as pm
from helpers import DEFAULT_COL, rgba_frames
from test_tilings_gpu import LINE

pytestmark = pytest.mark.gpu

ENVS = [{}, {"IPX_KS_TAIL": "0"}, {"IPX_KS_FAST": "0"}, {"IPX_KS_FIX_CAP": "7"}, {"IPX_KS_SPEC": "0"}]   # (the last: the control)
STATS = re.compile(r"\[ipx ks stats\] (\d+) frames: .*; (\d+) of (\d+) items redone in float64")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipa
    c = ipa.Context()
    yield c
    c.close()


def _env(monkeypatch, *envs):
    for k in OC.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


def _run(ctx, case, frames, glyphs):
    """(the tiling knobs are read when the plan is made and when it runs: the environment is set before either)"""
    w, h, resize, thumb = OC.CASES[case][:4]
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(w, h, resize=resize, thumbnail=thumb, watermark=gs)
    try:
        return plan.run_host(frames)
    finally:
        plan.close()
        gs.close()


def _same(got, want, what, names):
    """got: {output: n x ...}; want: [per frame {output: ...}]"""
    for k in OC.KEYS:
        w = np.stack([f[k] for f in want])
        if not np.array_equal(got[k], w):
            bad = [i for i in range(len(want)) if not np.array_equal(got[k][i], w[i])]
            i = bad[0]
            at = np.argwhere(got[k][i] != w[i])[:4].tolist()
            raise AssertionError("%s: %s of %d frames differ from the oracle (%s), first: %s at (y, x, channel) %r got %r want %r"
                                 % (what, len(bad), len(want), k, names[i], at, [int(got[k][i][tuple(p)]) for p in at],
                                    [int(w[i][tuple(p)]) for p in at]))


def _tilings(err):
    out = []
    for l in err.splitlines():
        if l.startswith("[ipx ks] src"):
            m = LINE.match(l)
            assert m, "cannot read %r" % l
            out.append((int(m.group(2)), int(m.group(3))))      # strips, segments
    return out


# ---- the sweep -------------------------------------------------------------------------------------------------------------------

_SWEEP = {}


def _sweep_batch(case, alpha):
    """One batch per frame size and probe alpha (cases a and b share theirs): a frame per position of the sweep that has teeth, two
    opaque base frames among them, the oracle's outputs of each."""
    w, h = OC.CASES[case][:2]
    if (w, h, alpha) not in _SWEEP:
        pos = OC.sweep(w, h)
        glyphs = OC.glyphs_for(w, h)
        frames, base = OC.one_pixel_frames(w, h, pos, alpha, seed=w * 31 + h)
        want = [OC.expected(f, case, glyphs) for f in frames]
        keep = [i for i in range(len(pos)) if OC.has_teeth(want[i])]
        assert len(keep) * 10 >= len(pos) * 9                   # (tests/test_opaque_cases.py names the dropped ones)
        names = ["pixel (x, y) = %r" % (pos[i],) for i in keep]
        frames, want = [frames[i] for i in keep], [want[i] for i in keep]
        wb = OC.expected(base, case, glyphs)
        assert not OC.has_teeth(wb)
        for at in (2 * len(frames) // 3, len(frames) // 3):
            frames.insert(at, base); want.insert(at, wb); names.insert(at, "an opaque frame")
        assert sum(OC.in_text(glyphs, *pos[i]) for i in keep) >= 10
        _SWEEP[(w, h, alpha)] = (np.stack(frames), want, names, glyphs)
    return _SWEEP[(w, h, alpha)]


@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("case", OC.SWEEP_CASES)
def test_one_pixel_anywhere(ctx, case, alpha, monkeypatch, capfd):
    frames, want, names, glyphs = _sweep_batch(case, alpha)
    knobs = OC.CASES[case][4]
    for env in ENVS:
        _env(monkeypatch, knobs, env, {"IPX_KS_DEBUG": "1"})
        capfd.readouterr()
        got = _run(ctx, case, frames, glyphs)
        ran = _tilings(capfd.readouterr().err)
        assert ran, "case %s %r: the one-pass kernel did not take the batch" % (case, env)
        if case == "a":                                          # the forced tiling cannot quietly fall away
            assert all(strips >= 3 and segs >= 2 for strips, segs in ran), ran
        _same(got, want, "case %s alpha %d %r" % (case, alpha, env), names)


# ---- the late exit behind full lists ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", [0, 1])
def test_late_pixel_behind_full_lists(ctx, alpha, monkeypatch):
    """Exactly 2:1 on the period-2 tile: every interior value of the resize sits on a rounding boundary, so every wave of the float
    pass lists pixels, and the item that meets the one pixel late has stored bytes and list entries before it is flagged.  y = 0 is
    the early exit on the same frames.  With lists of seven entries the overflow and the alpha both flag the item."""
    w, h = OC.CASES["d"][:2]
    tile = OC.boundary_frame(w, h)
    assert OC.on_boundary(tile) == 3 * (w // 2 - 2) * (h // 2 - 2)                    # the boundary values are really there
    pos = [(x, y) for y in (0, 4, 5, 47, 48, 95) for x in (3, 128, 255)]
    probes, _ = OC.one_pixel_frames(w, h, pos, alpha, seed=0, base=tile)
    assert all(OC.on_boundary(f) > 3 * (w // 2 - 2) * (h // 2 - 2) - 3 * 16 for f in probes)
    frames = np.concatenate([probes[:9], tile[None], probes[9:], rgba_frames(1, w, h, seed=0xD)])
    names = ["pixel (x, y) = %r" % (p,) for p in pos[:9]] + ["the untouched tile"] + ["pixel (x, y) = %r" % (p,) for p in pos[9:]] + ["a random opaque frame"]
    glyphs = OC.glyphs_for(w, h)
    want = [OC.expected(f, "d", glyphs) for f in frames]
    assert all(OC.has_teeth(want[i]) == (n.startswith("pixel")) for i, n in enumerate(names))
    for env in ({}, {"IPX_KS_FIX_CAP": "7"}, {"IPX_KS_TAIL": "0"}):
        _env(monkeypatch, env)
        _same(_run(ctx, "d", frames, glyphs), want, "alpha %d %r" % (alpha, env), names)


# ---- how many items are redone ------------------------------------------------------------------------------------------------------

def _redone(err):
    """-> (items redone, items launched as the stats count them, items launched as the tiling lines say)"""
    n = m = 0
    for l in err.splitlines():
        s = STATS.search(l)
        if s:
            n += int(s.group(2)); m += int(s.group(3))
    launched = 0
    for l in err.splitlines():
        if l.startswith("[ipx ks] src"):
            g = re.match(r"^\[ipx ks\] src \d+ nacc \d+ frames (\d+) strips (\d+) segs (\d+) ", l)
            launched += int(g.group(1)) * int(g.group(2)) * int(g.group(3))
    return n, m, launched


@pytest.mark.parametrize("split", ["1", "0"], ids=["split-segments", "whole-frames"])
def test_items_redone(ctx, split, monkeypatch, capfd):
    """IPX_KS_STATS=1 counts the flags of the items that ran.  Opaque frames: none redone.  k frames with one pixel among opaque
    ones: at least k items, and not all -- the opaque frames' items and the probe frames' far items keep their three-channel
    bytes.  Under the whole-frame segmentation fewer items run than the flag block has room for; the count covers the launched ones."""
    w, h = OC.CASES["a"][:2]
    glyphs = OC.glyphs_for(w, h)
    pos = [(0, 0), (w // 2, h // 2), (w - 1, h - 1)]
    probes, base = OC.one_pixel_frames(w, h, pos, 0, seed=w * 31 + h)
    opaque = np.repeat(base[None], 12, axis=0)
    mixed = opaque.copy()
    for i, at in enumerate((1, 6, 11)):
        mixed[at] = probes[i]
    _env(monkeypatch, OC.FORCED, {"IPX_KS_SPLIT": split, "IPX_KS_STATS": "1", "IPX_KS_DEBUG": "1"})
    capfd.readouterr()
    got = _run(ctx, "a", opaque, glyphs)
    n, m, launched = _redone(capfd.readouterr().err)
    assert launched >= 12 * 3 * (2 if split == "1" else 1)
    assert (n, m) == (0, launched)
    got = _run(ctx, "a", mixed, glyphs)
    n, m, launched = _redone(capfd.readouterr().err)
    assert m == launched and len(pos) <= n < m, (n, m, launched)
    if split == "1":
        assert n < 3 * m // 12, (n, m)      # even within the three probe frames some items are not redone
    _same(got, [OC.expected(f, "a", glyphs) for f in mixed], "mixed batch, IPX_KS_SPLIT=%s" % split, ["frame %d" % i for i in range(12)])


# ---- the whole-image alpha scans of the per-operation scalers ---------------------------------------------------------------------

SCAN_SIZES = [(37, 23, 20, 15), (300, 5, 40, 5)]


def _scan_positions(w, h):
    return [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 1, h // 2), (w // 2, h - 1)]


def _scan_entry(ctx, kind):
    """-> (the product's entry, the oracle's, frame maker (base values, position or None, alpha) -> source argument, probe alphas)"""
    if kind in ("rgba", "nrgba"):
        def make(px, p, alpha):
            f = px.copy()
            if p is not None:
                x, y = p
                f[y, x, 3] = alpha
                if kind == "rgba":
                    f[y, x, :3] = np.minimum(f[y, x, :3], alpha)
            return f
        if kind == "rgba":
            return ctx.scale_bilinear, oracle.scale_bilinear, make, (0, 254)
        return ctx.scale_bilinear_nrgba, oracle.scale_bilinear_nrgba, make, (0, 254)
    dk = oracle.DEEP_RGBA64 if kind == "rgba64" else oracle.DEEP_NRGBA64

    def make16(px, p, alpha):
        v = px.astype(np.uint16) * 257
        if p is not None:
            x, y = p
            v[y, x, 3] = alpha
            if kind == "rgba64":
                v[y, x, :3] = np.minimum(v[y, x, :3], alpha)
        return oracle.deep_pix(v, dk)
    # 0xfffe / 0xfeff: one byte of the sample alone is 0xff; 0x00ff: the other
    return (lambda s, *a, **k: ctx.scale_bilinear_deep(s, dk, *a, **k)), (lambda s, *a, **k: oracle.scale_bilinear_deep(s, dk, *a, **k)), \
        make16, (0xfffe, 0xfeff, 0x00ff)


@pytest.mark.parametrize("kind", ["rgba", "nrgba", "nrgba64", "rgba64"])
def test_whole_image_scans(ctx, kind, monkeypatch):
    """kernelScaler.Scale asks the WHOLE source image's Opaque() and turns Over into Src when it holds -- the source rectangle does
    not matter.  One pixel off, in a corner, in the last column, in the last row, inside the source rectangle or outside it: Over
    onto a used destination is the oracle's.  (A pixel outside the rectangle reaches no tap, and Over under alpha 0xffff stores
    Src's bytes: there the bytes cannot tell a miss, only the positions inside can.)  The all-opaque twin comes out as Src."""
    _env(monkeypatch)
    entry, model, make, alphas = _scan_entry(ctx, kind)
    for sw, sh, dw, dh in SCAN_SIZES:
        px = rgba_frames(1, sw, sh, seed=sw + sh)[0]
        under = np.random.default_rng(dw).integers(0, 256, (dh, dw, 4), dtype=np.uint8)
        under[..., :3] = np.minimum(under[..., :3], under[..., 3:4])
        inner = (2, 1, sw - 3, sh - 1)
        for sr in (None, inner):
            twin = make(px, None, 0)
            as_src = entry(twin, dw, dh, sr=sr, op=oracle.OP_SRC, dst=under.copy())
            np.testing.assert_array_equal(as_src, model(twin, dw, dh, sr=sr, op=oracle.OP_SRC, dst=under.copy()))
            np.testing.assert_array_equal(entry(twin, dw, dh, sr=sr, op=oracle.OP_OVER, dst=under.copy()), as_src,
                                          err_msg="%s %dx%d sr %r: Over of an opaque image is not Src" % (kind, sw, sh, sr))
            for p in _scan_positions(sw, sh):
                inside = sr is None or (sr[0] <= p[0] < sr[2] and sr[1] <= p[1] < sr[3])
                for alpha in alphas:
                    src = make(px, p, alpha)
                    want = model(src, dw, dh, sr=sr, op=oracle.OP_OVER, dst=under.copy())
                    if inside and alpha in (0, 0x00ff):          # the probe has teeth: a scan that misses the pixel stores other bytes
                        assert not np.array_equal(want, model(src, dw, dh, sr=sr, op=oracle.OP_SRC, dst=under.copy()))
                    got = entry(src, dw, dh, sr=sr, op=oracle.OP_OVER, dst=under.copy())
                    np.testing.assert_array_equal(got, want, err_msg="%s %dx%d -> %dx%d sr %r pixel %r alpha %#x" % (kind, sw, sh, dw, dh, sr, p, alpha))


# ---- png.Encode's colour type -------------------------------------------------------------------------------------------------------

def _colour_type(stream):
    assert stream[:8] == pm.SIGNATURE and stream[12:16] == b"IHDR"
    return stream[25]


def _png_positions(w, h):
    return [(0, 0), (w - 1, h - 1), (w - 1, 0)]                 # the first pixel, the last pixel, the last column of the first row


def test_png_colour_type_on_one_pixel(ctx, monkeypatch):
    """png.Encode writes colour type 6 for a frame that is not Opaque() and 2 for one that is, per output frame.  One pixel of alpha
    254 -- the first, the last, the end of the first row -- among opaque neighbours in the same batch."""
    _env(monkeypatch)
    # through the plan, at equal size: the pixel survives the resize exactly; all three positions lie outside the thumbnail's crop
    w, h = OC.CASES["e"][:2]
    pos = _png_positions(w, h)
    probes, base = OC.one_pixel_frames(w, h, pos, 254, seed=w * 31 + h)
    frames = np.stack([base, probes[0], probes[1], base, probes[2], base])
    probe = [False, True, True, False, True, False]
    glyphs = OC.glyphs_for(w, h)
    assert not any(OC.in_text(glyphs, *p) for p in pos)
    want = [OC.expected(f, "e", glyphs) for f in frames]
    _, _, resize, thumb = OC.CASES["e"][:4]
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(w, h, resize=resize, thumbnail=thumb, watermark=gs)
    try:
        got = plan.run_host_png(frames)
    finally:
        plan.close()
        gs.close()
    for i in range(len(frames)):
        for k in OC.KEYS:
            assert got[k][i] == pm.png_encode(want[i][k]), "%s of frame %d" % (k, i)
        assert _colour_type(got["resize"][i]) == (6 if probe[i] else 2), i
        assert _colour_type(got["watermark"][i]) == (6 if probe[i] else 2), i
        assert _colour_type(got["thumbnail"][i]) == 2, i
    # the encoder's batch entry on frames in device memory
    for w, h in ((61, 47), (257, 33)):
        probes, base = OC.one_pixel_frames(w, h, _png_positions(w, h), 254, seed=w + h)
        frames = np.ascontiguousarray(np.stack([base, probes[0], probes[1], base, probes[2], base]))
        d = ctx.alloc(frames.nbytes).upload(frames)
        try:
            got = ctx.png_encode_batch_dev(d.ptr, w, h, len(frames))
        finally:
            d.free()
        for i in range(len(frames)):
            assert got[i] == pm.png_encode(frames[i]), "%dx%d frame %d" % (w, h, i)
            assert _colour_type(got[i]) == (6 if probe[i] else 2), (w, h, i)
