"""GPU: the kernels against the float64 reference of tests/scaler_reference.py, at the edge geometries: the batch plans for every
kind of scaler_cases.KINDS (RGBA, NRGBA, Gray, YCbCr at 4:4:4, 4:2:2, 4:2:0, 4:4:0, 4:1:1 and 4:1:0, both palettes, the four deep
types), the per-operation seam for the kinds that have entries there (SEAM_KINDS: all but Gray and the palettes).

Two conditions per byte: it equals the reference wherever the reference is clear of a rounding boundary, and it equals the oracle
everywhere -- where the exact value is ambiguous, Go's order of operations decides, and the oracle restates that order.  The
per-operation seam (Context.scale_bilinear*, Context.draw*) and the batch plans (run_host*: resize, thumbnail, a watermark copy
without text) run under the kernel-path switches the rest of the suite enumerates.  For 4:1:1 and 4:1:0 the oracle's bytes are those
of its 4:4:4 routine on replicated chroma samples (scaler_cases.Source); the reference reads the subsampled planes."""
import os

import numpy as np
import pytest

import oracle
import scaler_reference as R
from scaler_cases import GEOMETRIES, KINDS, Source, cap
from test_parity_gpu import PATH_ENVS

pytestmark = pytest.mark.gpu

# the fused / path lists of test_sources_gpu.py and test_deep_gpu.py, as environments
SOURCE_PATHS = [{"IPX_FUSED": "1"}, {"IPX_FUSED": "0"},
                {"IPX_FUSED": "1", "IPX_KS_STRIPS": "3", "IPX_KS_SPLIT": "1", "IPX_KS_SPLIT_ROWS": "23"},
                {"IPX_FUSED": "1", "IPX_KS_FAST": "0"}, {"IPX_FUSED": "1", "IPX_KS_FIX_CAP": "9"}]
ALL_PATHS = PATH_ENVS + [e for e in SOURCE_PATHS if e not in PATH_ENVS]
SEAM_PATHS = [{}, {"IPX_KS_FAST": "0"}, {"IPX_FUSED": "0"}]
SEAM_KINDS = ["rgba", "nrgba", "ycbcr444", "ycbcr422", "ycbcr420", "ycbcr440", "ycbcr411", "ycbcr410", "nrgba64", "rgba64", "gray16", "cmyk"]
KNOBS = sorted({k for e in ALL_PATHS + SEAM_PATHS for k in e})

# (w, h, resize, thumbnail) for the batch plans
PLAN_CASES = [(333, 251, (200, 100, False), (64, True)),        # odd sizes, crop origin (41, 0)
              (251, 333, (1024, 768, True), (64, True)),        # an upscale, crop origin (0, 41)
              (97, 61, (155, 97, False), (40, False)),          # x1.6, a non-crop thumbnail
              (495, 37, (10, 37, False), (20, True)),           # nx + ny = 100: the float pass's last tap count
              (500, 37, (10, 37, False), (20, True)),           # nx + ny = 101: float64 throughout
              (4000, 41, (8, 41, False), (20, True))]           # 500 horizontal taps


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipa
    c = ipa.Context()
    yield c
    c.close()


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _both(got, want, ref, kind, what):
    R.assert_matches(got, *ref, max_ambiguous=cap(kind), what="%s %s" % (kind, what))
    np.testing.assert_array_equal(got, want, err_msg="%s %s: the kernel differs from the oracle" % (kind, what))


# ---- the per-operation seam --------------------------------------------------------------------------------------------------

def _seam_scale(ctx, src, dw, dh, sr, op, dst):
    k = src.kind
    dst = dst.copy()
    if k == "rgba":
        return ctx.scale_bilinear(src.data, dw, dh, sr=sr, op=op, dst=dst)
    if k == "nrgba":
        return ctx.scale_bilinear_nrgba(src.data, dw, dh, sr=sr, op=op, dst=dst)
    if k.startswith("ycbcr"):
        return ctx.scale_bilinear_ycbcr(*src.data, dw, dh, sr=sr, dst=dst)
    return ctx.scale_bilinear_deep(src.data, oracle.DEEP_NRGBA64 if k == "nrgba64" else {"rgba64": oracle.DEEP_RGBA64, "gray16": oracle.DEEP_GRAY16,
                                                                                       "cmyk": oracle.DEEP_CMYK}[k], dw, dh, sr=sr, op=op, dst=dst)


def _seam_draw(ctx, src, dst, r, sp, op):
    k = src.kind
    dst = dst.copy()
    if k == "rgba":
        return ctx.draw(dst, r, src.data, sp, op)
    if k == "nrgba":
        return ctx.draw_nrgba(dst, r, src.data, sp, op)
    if k.startswith("ycbcr"):
        return ctx.draw_ycbcr(dst, r, *src.data, sp)
    return ctx.draw_deep(dst, r, src.data, {"nrgba64": oracle.DEEP_NRGBA64, "rgba64": oracle.DEEP_RGBA64, "gray16": oracle.DEEP_GRAY16,
                                            "cmyk": oracle.DEEP_CMYK}[k], sp, op)


def seam_cases(kind):
    """-> [(what, call, oracle bytes, Ref)] with call = ("scale", dw, dh, sr, op, dst) | ("draw", dst, r, sp, op)"""
    out = []
    for geom in GEOMETRIES:
        sw, sh, dw, dh, sr = geom
        src = Source(kind, sw, sh, seed=sw * 7 + sh)
        zeros = np.zeros((dh, dw, 4), np.uint8)
        under = np.random.default_rng(dw).integers(0, 256, (dh, dw, 4), dtype=np.uint8)
        under[..., :3] = np.minimum(under[..., :3], under[..., 3:4])
        for op, dst in ((oracle.OP_OVER, zeros), (oracle.OP_SRC, under), (oracle.OP_OVER, under)):
            if kind.startswith("ycbcr") and op == oracle.OP_SRC:
                continue
            out.append(("scale %r op %d" % (geom, op), src, ("scale", dw, dh, sr, op, dst), src.oracle_scale(dw, dh, sr=sr, op=op, dst=dst),
                        R.scale(src.ref, dw, dh, sr=sr, op=op, dst=dst)))
    src = Source(kind, 157, 93, seed=11)
    under = np.random.default_rng(4).integers(0, 256, (93, 157, 4), dtype=np.uint8)
    under[..., :3] = np.minimum(under[..., :3], under[..., 3:4])
    for op in (oracle.OP_SRC, oracle.OP_OVER):
        for r, sp in (((0, 0, 157, 93), (0, 0)), ((5, 7, 75, 60), (3, 1)), ((-4, -3, 200, 200), (9, 13))):
            out.append(("draw %r %r op %d" % (r, sp, op), src, ("draw", under, r, sp, op), src.oracle_draw(under, r, sp, op),
                        R.draw(under, r, src.ref, sp, op)))
    return out


@pytest.mark.parametrize("kind", SEAM_KINDS)
def test_seam_against_reference(ctx, kind, monkeypatch):
    cases = seam_cases(kind)
    for env in SEAM_PATHS:
        _env(monkeypatch, env)
        for what, src, call, want, ref in cases:
            if call[0] == "scale":
                got = _seam_scale(ctx, src, *call[1:])
            else:
                got = _seam_draw(ctx, src, *call[1:])
            _both(got, want, ref, kind, "%s %r" % (what, env))


# ---- the batch plans ---------------------------------------------------------------------------------------------------------

def plan_case(kind, case, n=2):
    """-> (sources, oracle outputs per frame, Refs per frame)"""
    w, h, resize, thumb = case
    srcs = [Source(kind, w, h, seed=w * 31 + h + i) for i in range(n)]
    want, ref = [], []
    for s in srcs:
        o, stage1 = s.oracle_ops(resize, thumb)
        want.append(o)
        ref.append(s.ref_ops(resize, thumb, stage1))
    return srcs, want, ref


def _run_plan(plan, kind, srcs):
    if kind == "rgba":
        return plan.run_host(np.stack([s.data for s in srcs]))
    if kind == "nrgba":
        return plan.run_host_nrgba(np.stack([s.data for s in srcs]))
    if kind == "gray":
        return plan.run_host_gray(np.stack([s.data for s in srcs]))
    if kind.startswith("ycbcr"):
        return plan.run_host_ycbcr(*(np.stack([s.data[c] for s in srcs]) for c in range(3)), srcs[0].data[3])
    if kind.startswith("paletted"):
        return plan.run_host_paletted(np.stack([s.data[0] for s in srcs]), np.stack([s.data[1] for s in srcs]))
    from scaler_cases import DEEP
    return plan.run_host_deep(np.stack([s.data for s in srcs]), DEEP[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_batch_plans_against_reference(ctx, kind, monkeypatch):
    for case in PLAN_CASES:
        w, h, resize, thumb = case
        srcs, want, ref = plan_case(kind, case)
        for env in ALL_PATHS:
            _env(monkeypatch, env)
            plan = ctx.plan(w, h, resize=resize, thumbnail=thumb, watermark=True)
            try:
                got = _run_plan(plan, kind, srcs)
            finally:
                plan.close()
            for i in range(len(srcs)):
                for k in ("resize", "thumbnail", "watermark"):
                    _both(got[k][i], want[i][k], ref[i][k], kind, "%s frame %d %r %r" % (k, i, case, env))


if __name__ == "__main__":
    # the CPU half of this file (oracle against reference at every case it uses), for a machine without a GPU
    for kind in SEAM_KINDS:
        for what, src, call, want, ref in seam_cases(kind):
            R.assert_matches(want, *ref, max_ambiguous=cap(kind), what="%s %s" % (kind, what))
    for kind in KINDS:
        for case in PLAN_CASES:
            srcs, want, ref = plan_case(kind, case)
            for i in range(len(srcs)):
                for k in ("resize", "thumbnail", "watermark"):
                    R.assert_matches(want[i][k], *ref[i][k], max_ambiguous=cap(kind), what="%s %s %r" % (kind, k, case))
    print("oracle matches the reference at every case of %s" % os.path.basename(__file__))
