"""The host half of the 4:1:1 / 4:1:0 JPEG decoder (IPX_JPEG_411=1) on the CPU: the marker parser, the routes and the scan decoder.

  - ipx_jpeg_scan_route (host only, no GPU): with the switch unset (or set to anything but 1) both shapes are IPX_ERR_UNSUPPORTED, as
    they always were; with it set they are IPX_OK -- the parallel route for one baseline scan, the host-scans route for progressive and
    multi-scan files, IPX_JPEG_PROG_GPU or not.  Y (4,4), Y (4,1) over (2,1) chroma and Y (3,1) stay UNSUPPORTED, a truncated file is
    INVALID.  The switch-on test fails on a library without the feature.
  - tools/sanitize/jpeg411_host_test.cpp, built with the two host sources under -fsanitize=address,undefined, decodes the corpus's
    files and seeded mutations of them; the coefficients it returns are compared with the layout the IDCT kernel reads, laid out here
    from the same blocks: block j of an MCU at (j % 4, j / 4), six or ten blocks per MCU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_411_corpus as c4
import jpeg_writer as jw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -4
SIZES = [(1, 1), (33, 9), (65, 17)]


def files():
    """[(name, file, kind)]: kind baseline | restarts | multiscan | progressive"""
    out = []
    for v0 in (1, 2):
        for w, h in SIZES:
            fr = c4.frame(w, h, v0)
            b = c4.blocks(fr, 7 * w + v0)
            tag = "%s_%dx%d" % ("411" if v0 == 1 else "410", w, h)
            out += [(tag + "_baseline", c4.baseline(fr, b), "baseline", fr, b), (tag + "_ri1", c4.baseline(fr, b, ri=1), "baseline", fr, b),
                    (tag + "_multiscan", c4.multiscan(fr, b), "multiscan", fr, b), (tag + "_progressive", c4.progressive(fr, b), "progressive", fr, b)]
    return out


def refused():
    return [(name, c4.refused_file(40, 24, **kw)) for name, kw in c4.REFUSED]


@pytest.fixture(scope="module")
def ipx():
    from imageprocessor_amd import build
    build.build()
    import imageprocessor_amd as m
    return m


@pytest.mark.parametrize("value", [None, "0", "2", "on"])
def test_without_the_switch_both_shapes_are_unsupported(ipx, monkeypatch, value):
    monkeypatch.delenv("IPX_JPEG_411", raising=False) if value is None else monkeypatch.setenv("IPX_JPEG_411", value)
    for name, data, *_ in files():
        st, _ = ipx.Context.jpeg_scan_route(data)
        assert st == UNSUPPORTED, name
    for name, data in refused():
        assert ipx.Context.jpeg_scan_route(data)[0] == UNSUPPORTED, name


@pytest.mark.parametrize("prog_gpu", [None, "1"])
def test_with_the_switch_the_two_shapes_have_a_route(ipx, monkeypatch, prog_gpu):
    monkeypatch.setenv("IPX_JPEG_411", "1")
    monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False) if prog_gpu is None else monkeypatch.setenv("IPX_JPEG_PROG_GPU", prog_gpu)
    for name, data, kind, *_ in files():
        st, route = ipx.Context.jpeg_scan_route(data)
        want = ipx.Context.JPEG_ROUTE_PAR if kind == "baseline" else ipx.Context.JPEG_ROUTE_HOST_SCANS     # never the GPU scan walk
        assert (st, route) == (OK, want), name
    for name, data in refused():
        assert ipx.Context.jpeg_scan_route(data)[0] == UNSUPPORTED, name
    good = files()[4][1]
    assert ipx.Context.jpeg_scan_route(c4.cut_in_scan(good))[0] == INVALID
    assert ipx.Context.jpeg_scan_route(good[:len(good) // 3])[0] == INVALID


def test_the_switch_leaves_the_other_samplings_alone(ipx, monkeypatch):
    """4:2:0 and 4:4:4 files answer the same with and without it (a progressive one still reaches the GPU scan walk)"""
    import jpeg_prog_writer as pw
    fr = pw.colour_frame(33, 17, 2, 2)
    b = c4.blocks(fr, 3)
    for data in (pw.baseline(fr, b), pw.progressive(fr, b, pw.libjpeg_script(fr))):
        answers = []
        for value in (None, "1"):
            monkeypatch.delenv("IPX_JPEG_411", raising=False) if value is None else monkeypatch.setenv("IPX_JPEG_411", value)
            monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
            answers.append(ipx.Context.jpeg_scan_route(data))
        assert answers[0] == answers[1] and answers[0][0] == OK


def expected_words(fr, b, kind):
    """the coefficients as jpeg_host_decode leaves them: blocks in MCU order (the MCU's Y blocks row-major, four to a row, then Cb, Cr),
    natural coefficient order, element 0 zero; then every block's DC term.  A non-interleaved scan carries no data for a block outside
    the image by its component's own grid: in a progressive file (interleaved DC scans, AC bands per component) its AC terms stay zero,
    in the sequential multi-scan file the whole block."""
    h0, v0 = fr.hv[0]
    order = []
    for my in range(fr.myy):
        for mx in range(fr.mxx):
            order += [(0, v0 * my + j // h0, h0 * mx + j % h0) for j in range(h0 * v0)] + [(1, my, mx), (2, my, mx)]
    coefs = np.zeros((len(order), 64), np.int16)
    dcs = np.zeros(len(order), np.int16)
    for n, (comp, by, bx) in enumerate(order):
        zz = b[comp][by, bx]
        outside = bx * 8 >= fr.w or by * 8 >= fr.h
        if not (kind == "multiscan" and outside):
            dcs[n] = zz[0]
        if not (kind in ("multiscan", "progressive") and outside):
            coefs[n, jw.ZIG[1:]] = zz[1:]
    return coefs.tobytes() + dcs.tobytes()


def test_host_decoder_under_sanitizers_and_its_layout(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    csrc = os.path.join(ROOT, "imageprocessor_amd", "csrc")
    exe = str(tmp_path / "jpeg411_host_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
           "-fno-sanitize=shift-base", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-pthread", "-o", exe,
           os.path.join(ROOT, "tools", "sanitize", "jpeg411_host_test.cpp"), os.path.join(csrc, "ipx_jpeg_dec_host.cpp"), os.path.join(csrc, "ipx_jpeg_dec_prog.cpp")]
    subprocess.check_call(cmd)
    paths = []

    def put(name, data, head, words=b""):
        p = str(tmp_path / (name.replace(" ", "_") + ".jpg"))
        with open(p, "wb") as fh:
            fh.write(data)
        with open(p + ".want", "wb") as fh:
            fh.write(struct.pack("<6i", *head) + words)
        paths.append(p)

    for name, data, kind, fr, b in files():
        h0, v0 = fr.hv[0]
        put(name, data, (OK, h0, v0, int(kind != "baseline"), int(kind == "progressive"), 7 if kind == "multiscan" else 0), expected_words(fr, b, kind))
    for name, data in refused():
        put(name, data, (UNSUPPORTED, 0, 0, 0, 0, 0))
    good = files()[4][1]
    put("cut", c4.cut_in_scan(good), (INVALID, 0, 0, 0, 0, 0))
    put("no_eoi", good[:-2], (INVALID, 0, 0, 0, 0, 0))
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "%d files, %d with expectations" % (len(paths), len(paths)) in r.stdout and " 0 wrong" in r.stdout
