"""ks_fused_plan on the CPU: tools/ks_plan_check.cpp builds the planner as host C++ (no device code, no GPU), asks it for the tiling
of every case of tests/tiling_cases.py, of the upload sizes with their operator sets and of a seeded sweep (widths to 65 532, crop
rectangles, one operator or both, up- and downscales), for tiles of 4, 8 and 2 bytes, and checks in every plan what ks_fused_kernel
relies on: strips, column ownership, tap bounds, weight tables bit for bit, both LDS layouts, segments and row entries.

Three assertions: no violation; every case of the GPU table is planned into the class it claims; every class the upload sizes
reach at widths of 2560 and more is claimed by some case -- so what tests/test_tilings_gpu.py runs is what real uploads reach."""
import os
import shutil
import subprocess

import pytest

import tiling_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = 3200
KNOBS = ("IPX_KS_STRIPS", "IPX_KS_SPLIT_ROWS", "IPX_KS_TAPSPLIT", "IPX_KS_FAST_DBUF")


def _hip_include(hipcc):
    exe = shutil.which(hipcc) or hipcc
    for root in (os.path.dirname(os.path.dirname(os.path.realpath(exe))), os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return ["-I" + os.path.join(root, "include")]
    return []


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """-> {"P": {tag: {px: claim}}, "N": [...], "V": [...], "T": {class: count}, "summary": str} of one run over all three sets"""
    from imageprocessor_amd.build import CSRC, hipcc
    exe = str(tmp_path_factory.mktemp("ks_plan") / "ks_plan_check")
    cmd = [hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__"] + _hip_include(hipcc()) + \
          [os.path.join(CSRC, "ipx_ks_host.cpp"), os.path.join(CSRC, "ipx_host.cpp"), os.path.join(ROOT, "tools", "ks_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [T.shape_line("case:%d" % i, *case) for i, (case, _, _) in enumerate(T.CASES)] + [T.shape_line(*u) for u in T.upload_shapes()] + \
            [T.shape_line("jpeg", *T.JPEG_CASE[0])]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([exe, "--sweep", str(SWEEP), "20261019"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-4000:]
    out = {"P": {}, "N": [], "V": [], "X": [], "T": {}, "summary": ""}
    for l in r.stdout.splitlines():
        f = l.split()
        if f[0] == "P":
            out["P"].setdefault(f[1], {})[int(f[2])] = tuple(int(v) for v in f[3:9])
        elif f[0] == "T":
            out["T"][tuple(int(v) for v in f[1:8])] = int(f[8])
        elif f[0] in ("N", "X"):
            out[f[0]].append(f[1])
        elif f[0] == "V":
            out["V"].append(l)
        elif f[0] == "ks_plan_check:":
            out["summary"] = l
    assert out["summary"], r.stdout[-2000:]
    print(out["summary"])
    return out


def test_no_plan_violates_what_the_kernel_relies_on(report):
    assert not report["V"], "\n".join(report["V"][:40])
    assert report["summary"].endswith(" 0 violations"), report["summary"]
    # the sweep ran and met both answers: plans in many classes, and geometries the planner leaves to the per-output kernels
    sweep = [t for t in report["P"] if t.startswith("sweep:")]
    declined = [t for t in report["N"] if t.startswith("sweep:")]
    assert len(set(sweep) | set(declined)) + len([t for t in report["X"] if t.startswith("sweep:")]) >= 3000
    assert len(sweep) >= 1500 and declined
    assert max(int(t.split(":")[1].split(",")[0]) for t in sweep) == 65532
    assert len([k for k in report["T"] if k[0] == 8]) >= 30, sorted(report["T"])


def test_every_case_is_planned_into_the_class_it_claims(report):
    for i, (case, frames, claims) in enumerate(T.CASES):
        assert case[0] % 4 == 0 and frames in (1, 2)
        got = report["P"].get("case:%d" % i, {})
        for px in T.TILE_BYTES:
            assert got.get(px) == claims[px], "case %d %r, %d-byte tile: planned %r, claimed %r" % (i, case, px, got.get(px), claims[px])
    assert report["P"]["jpeg"][8] == T.JPEG_CASE[1] and T.JPEG_CASE[0][0] % 4 == 0


def test_every_class_wide_uploads_reach_is_claimed_by_a_case(report):
    claimed = {T.klass(px, claims[px]) for _, _, claims in T.CASES for px in T.TILE_BYTES}
    missing = {}
    for tag, w, h, resize, thumb in T.upload_shapes():
        plans = report["P"].get(tag, {})
        assert sorted(plans) == sorted(T.TILE_BYTES), "%s: the planner declined an upload size" % tag
        if w < T.UPLOAD_MIN_WIDTH:
            continue
        for px, claim in plans.items():
            if T.klass(px, claim) not in claimed:
                missing.setdefault(T.klass(px, claim), []).append(tag)
    assert not missing, "classes no case of tiling_cases.CASES runs: %r" % missing
