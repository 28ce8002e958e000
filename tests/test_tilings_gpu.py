"""GPU: the one-pass scaler at the tilings ks_fused_plan picks BY ITSELF for wide frames, for every kind of
scaler_cases.KINDS: every source type the one-pass kernel is instantiated for, YCbCr at 4:1:1 and 4:1:0 (KS_YCC4, 8-byte tiles) included.

No tiling knob is set.  Each case of tests/tiling_cases.py claims a class per tile size -- strips, accumulators, one or two tile
buffers in either LDS layout, the float pass's list entries per wave, lanes per column -- and the library's IPX_KS_DEBUG line has to
show exactly that, so that a planner change cannot quietly move a case to an easier tiling (tests/test_ks_plan_host.py checks the
same claims on the CPU, and that the classes real upload sizes reach are all here).  The bytes are held to both conditions of
tests/test_scaler_reference_gpu.py: the float64 reference wherever it is clear of a rounding boundary, the oracle everywhere; the
watermark copy checks the strips' ownership of source columns.  Each case runs by default, with the float pass off, and with lists
of nine entries, which every frame overflows: float64 again, under the float pass's layout.

`python tests/test_tilings_gpu.py` is the CPU half: the oracle against the reference at every case and kind."""
import os
import re
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle
import scaler_reference as R
from scaler_cases import KINDS, cap
from test_scaler_reference_gpu import KNOBS, _both, _run_plan, plan_case
from tiling_cases import CASES, JPEG_CASE, tile_bytes

ENVS = [{}, {"IPX_KS_FAST": "0"}, {"IPX_KS_FIX_CAP": "9"}]
ALL_KNOBS = sorted(set(KNOBS) | {"IPX_KS_TAPSPLIT", "IPX_KS_FAST_DBUF", "IPX_NO_FUSE"})
LINE = re.compile(r"^\[ipx ks\] src \d+ nacc (\d+) frames \d+ strips (\d+) segs (\d+) threads \d+ pitch \d+ dbuf (\d+) lds \d+ \(float pass: dbuf (\d+) lds \d+\) "
                  r".*\| float pass: open_per_wave (\d+) split (\d+) (\d+)$")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipa
    c = ipa.Context()
    yield c
    c.close()


def _env(monkeypatch, env):
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("IPX_KS_DEBUG", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _tilings(capfd):
    """-> [((nacc, strips, dbuf, float pass dbuf, list entries per wave, lanes per column), segments)], one per one-pass launch"""
    out = []
    for l in capfd.readouterr().err.splitlines():
        if l.startswith("[ipx ks] src"):
            m = LINE.match(l)
            assert m, "cannot read %r" % l
            nacc, strips, segs, dbuf, fdbuf, per_wave, s0, s1 = (int(v) for v in m.groups())
            out.append(((nacc, strips, dbuf, fdbuf, per_wave, max(1, s0, s1)), segs))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_natural_tilings_against_reference(ctx, ci, kind, monkeypatch, capfd):
    case, frames, claims = CASES[ci]
    w, h, resize, thumb = case
    srcs, want, ref = plan_case(kind, case, n=frames)
    for env in ENVS:
        _env(monkeypatch, env)
        capfd.readouterr()
        plan = ctx.plan(w, h, resize=resize, thumbnail=thumb, watermark=True)
        try:
            got = _run_plan(plan, kind, srcs)
        finally:
            plan.close()
        ran = _tilings(capfd)
        assert ran, "%s %r %r: the one-pass kernel did not take the batch" % (kind, case, env)
        for tiling, _ in ran:
            assert tiling == claims[tile_bytes(kind)], "%s %r %r: ran as %r, the case claims %r" % (kind, case, env, tiling, claims[tile_bytes(kind)])
        for i in range(len(srcs)):
            for k in ("resize", "thumbnail", "watermark"):
                _both(got[k][i], want[i][k], ref[i][k], kind, "%s frame %d %r %r" % (k, i, case, env))


@pytest.mark.gpu
@pytest.mark.parametrize("subsampling", [2, 0])
def test_wide_jpeg_files_through_the_two_strip_tiling(ctx, subsampling, monkeypatch, capfd):
    from helpers import DEFAULT_COL, text_glyphs
    from test_jpeg_decode import picture, pil_jpeg
    from test_sources_gpu import _expect_ycbcr_ops
    (w, h, resize, thumb), tiling = JPEG_CASE
    files = [pil_jpeg(picture(w, h, seed=70 + i), quality=88, subsampling=subsampling) for i in range(2)]
    glyphs = text_glyphs(w, h, n=4, width_px=30, height_px=12)
    _env(monkeypatch, {})
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(w, h, resize=resize, thumbnail=thumb, watermark=gs)
    try:
        capfd.readouterr()
        got, st = plan.run_jpeg_jpeg(files, 85)
        ran = _tilings(capfd)
    finally:
        plan.close()
        gs.close()
    assert st == [0, 0]
    assert ran and all(t == tiling for t, _ in ran), ran
    for i, f in enumerate(files):
        d = oracle.jpeg_decode(f)
        assert d["ratio"] == subsampling and d["y"].shape[1] != w     # the padded stride this case is about
        chh, cw = oracle.chroma_shape(w, h, d["ratio"])
        e = _expect_ycbcr_ops(np.ascontiguousarray(d["y"][:h, :w]), np.ascontiguousarray(d["cb"][:chh, :cw]), np.ascontiguousarray(d["cr"][:chh, :cw]),
                              d["ratio"], resize, thumb, glyphs, DEFAULT_COL)
        for k in ("resize", "thumbnail", "watermark"):
            assert got[k][i] == oracle.jpeg_encode_rgba(e[k], 85), "%s of file %d (subsampling %d)" % (k, i, subsampling)


if __name__ == "__main__":
    # the CPU half of this file (oracle against reference at every case and kind), for a machine without a GPU
    for case, frames, _ in CASES:
        for kind in KINDS:
            srcs, want, ref = plan_case(kind, case, n=frames)
            for i in range(len(srcs)):
                for k in ("resize", "thumbnail", "watermark"):
                    R.assert_matches(want[i][k], *ref[i][k], max_ambiguous=cap(kind), what="%s %s %r" % (kind, k, case))
    print("oracle matches the reference at every case of %s" % os.path.basename(__file__))
