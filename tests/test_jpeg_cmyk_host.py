"""The host half of the four-component JPEG decoder (IPX_JPEG_CMYK=1) on the CPU: the marker parser and the scan decoder.

  - tools/sanitize/jpeg4_host_test.cpp, built with the two host sources under -fsanitize=address,undefined, decodes the writer's files
    (both vectors, every transform, baseline, restart intervals, progressive, APP14 absent or short, the illegal vectors) and seeded
    mutations of them; the two coefficient sets it returns are compared with the layouts the IDCT kernel reads, laid out here from the
    same blocks, at 1x1, 9x7 and 17x15
  - ipx_jpeg_scan_route (host only): without the switch every four-component file is IPX_ERR_UNSUPPORTED, as it always was"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cmyk_writer as cw
import jpeg_writer as jw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -4


def expected_words(frame, blocks, progressive):
    """the two sets as jpeg_host_decode4 leaves them: components 0..2 in MCU order (Y blocks row-major, Cb, Cr), then component 3 raster
    by block; natural coefficient order, element 0 zero; then every block's DC term.  A progressive file's band scans carry no data for
    a block wholly outside the image: its AC coefficients stay zero."""
    v = frame.hv[0][0]
    seq = [(0, v * my + j // v, v * mx + j % v) for my in range(frame.myy) for mx in range(frame.mxx) for j in range(v * v)]
    order = []
    it = iter(seq)
    for my in range(frame.myy):
        for mx in range(frame.mxx):
            order += [next(it) for _ in range(v * v)] + [(1, my, mx), (2, my, mx)]
    rows, cols = frame.grid(3)
    order += [(3, by, bx) for by in range(rows) for bx in range(cols)]
    coefs = np.zeros((len(order), 64), np.int16)
    dcs = np.zeros(len(order), np.int16)
    for n, (c, by, bx) in enumerate(order):
        zz = blocks[c][by, bx]
        dcs[n] = zz[0]
        if not (progressive and (bx * 8 >= frame.w or by * 8 >= frame.h)):
            coefs[n, jw.ZIG[1:]] = zz[1:]
    return coefs.tobytes() + dcs.tobytes()


def corpus():
    """[(name, file, expected status, transform, progressive, words or None)]"""
    out = []
    for w, h in ((1, 1), (9, 7), (17, 15)):
        for v in (1, 2):
            f = cw.frame4(w, h, v)
            b = cw.blocks4(f, 40 + w + v)
            for transform, prog, dri in ((0, False, 0), (2, False, 1), (1, True, 0)):
                out.append(("%dx%d_v%d_t%d_p%d_r%d" % (w, h, v, transform, prog, dri), cw.cmyk_file(f, b, transform=transform, progressive=prog, dri=dri),
                            OK, transform, int(prog), expected_words(f, b, prog)))
    f = cw.frame4(17, 15, 2)
    b = cw.blocks4(f, 77)
    out.append(("app14_absent", cw.cmyk_file(f, b, app14="absent"), UNSUPPORTED, 0, 0, None))
    out.append(("app14_short", cw.cmyk_file(f, b, app14="short", progressive=True), UNSUPPORTED, 0, 0, None))
    for name, hv in cw.ILLEGAL_VECTORS.items():
        fi = cw.frame4(17, 15, hv=hv)
        out.append(("vector_" + name.replace(" ", "_"), cw.cmyk_file(fi, cw.blocks4(fi, 78)), UNSUPPORTED, 0, 0, None))
    good = cw.cmyk_file(f, b, transform=2)
    out.append(("truncated", good[:len(good) * 2 // 3], INVALID, 0, 0, None))
    out.append(("no_eoi", good[:-2], INVALID, 0, 0, None))
    return out


def test_host_decoder_under_sanitizers_and_its_layouts(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    csrc = os.path.join(ROOT, "imageprocessor_amd", "csrc")
    exe = str(tmp_path / "jpeg4_host_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
           "-fno-sanitize=shift-base", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-pthread", "-o", exe,
           os.path.join(ROOT, "tools", "sanitize", "jpeg4_host_test.cpp"), os.path.join(csrc, "ipx_jpeg_dec_host.cpp"), os.path.join(csrc, "ipx_jpeg_dec_prog.cpp")]
    subprocess.check_call(cmd)
    paths = []
    for name, data, status, transform, prog, words in corpus():
        p = str(tmp_path / (name + ".jpg"))
        with open(p, "wb") as fh:
            fh.write(data)
        with open(p + ".want", "wb") as fh:
            fh.write(struct.pack("<3i", status, transform, prog) + (words or b""))
        paths.append(p)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "%d files, %d with expectations" % (len(paths), len(paths)) in r.stdout and " 0 wrong" in r.stdout


@pytest.fixture(scope="module")
def ipx():
    from imageprocessor_amd import build
    build.build()
    import imageprocessor_amd as m
    return m


@pytest.mark.parametrize("value", [None, "0", "2", "on"])
def test_without_the_switch_every_four_component_file_is_unsupported(ipx, monkeypatch, value):
    monkeypatch.delenv("IPX_JPEG_CMYK", raising=False) if value is None else monkeypatch.setenv("IPX_JPEG_CMYK", value)
    for name, data, *_ in corpus():
        st, _ = ipx.Context.jpeg_scan_route(data)
        assert st == UNSUPPORTED, name


def test_with_the_switch_the_legal_vectors_take_the_host_route(ipx, monkeypatch):
    monkeypatch.setenv("IPX_JPEG_CMYK", "1")
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")          # a four-component file never takes the GPU scan walk
    for name, data, status, *_ in corpus():
        st, route = ipx.Context.jpeg_scan_route(data)
        if name.startswith("vector_"):
            assert st == UNSUPPORTED, name
        else:                              # (APP14 and the scans are the scan decoder's to judge)
            assert (st, route) == (OK, ipx.Context.JPEG_ROUTE_HOST_SCANS), name
