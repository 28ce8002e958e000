"""PNG uploads of mixed sizes in one batch, the part that needs no GPU: the three new entries and the two structs are declared in the
header, bound in the ctypes table, wrapped in Python and called from the Go source; and the mixed leg's ordering and cutting (files ->
decode groups -> chunks -> runs, csrc/ipx_mixed_cut.h) and the layouts of decoded frames and palettes (csrc/ipx_png_layout.h) hold their rules in tools/png_mixed_plan_test.cpp, built with the address and
undefined-behaviour sanitizers and run as a program of its own."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ipx_png_decode_mixed", "ipx_png_encode_mixed_dev", "ipx_run_png_png_mixed"]


def test_the_new_entries_are_declared_bound_and_wrapped():
    from imageprocessor_amd import _lib
    h = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ipx.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, h), n
        assert n in _lib.SIGNATURES, n
    # the two structs: the header's fields, in order, are the ctypes mirror's
    for name, mirror in (("ipx_png_frame", _lib.PngFrame), ("ipx_rgba_frame", _lib.RgbaFrame)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, h)
        assert body, name
        fields = re.findall(r"\*?\b(\w+)\s*[,;]", body.group(1))
        assert fields == [f[0] for f in mirror._fields_], (name, fields)
    assert _lib.PngFrame.pix.offset == 16 and _lib.PngFrame.palette.offset == 32 and C.sizeof(_lib.PngFrame) == 40
    assert _lib.RgbaFrame.w.offset == 8 and C.sizeof(_lib.RgbaFrame) == 24
    # the prototypes' parameter counts are the ctypes table's
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % n, h, flags=re.S).group(1)
        assert params.count(",") + 1 == len(_lib.SIGNATURES[n][1]), n
    assert "#define IPX_ABI_VERSION 1" in h or re.search(r"IPX_ABI_VERSION\s*=?\s*1\b", h)
    go = open(os.path.join(ROOT, "go", "ipx", "png.go")).read()
    assert "func (x *Context) RunPNGPNGMixed(" in go and "C.ipx_run_png_png_mixed(" in go
    import imageprocessor_amd as m
    for n in ("png_decode_mixed", "png_encode_mixed_dev", "run_png_png_mixed"):
        assert hasattr(m.Context, n), n


def test_the_library_exports_the_new_entries():
    from imageprocessor_amd import build
    build.build()
    import imageprocessor_amd as m
    L = m.lib()
    for n in NAMES:
        assert hasattr(L, n), n


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_legs_ordering_and_cutting_under_sanitizers(tmp_path):
    exe = str(tmp_path / "png_mixed_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "png_mixed_plan_test.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "png mixed plan ok" in r.stdout
