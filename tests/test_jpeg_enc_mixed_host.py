"""jpeg.Encode of frames of mixed sizes in one call, the part that needs no GPU: the new entry is declared in the header, bound in
the ctypes table with the prototype's parameter count, wrapped in Python and called from the Go source; the built library exports it;
the new header is in the build's lists; and the host side of the per-frame records (csrc/ipx_jpeg_enc_mixed_plan.h: the geometry, the
64-bit prefix sums of MCUs, workgroups, chunks and bytes, the workgroup -> frame search of each grid) holds its rules against a
transcription of the uniform encoder's arithmetic in tools/jpeg_enc_mixed_plan_test.cpp, built with the address and
undefined-behaviour sanitizers and run as a program of its own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ipx_jpeg_encode_mixed_dev"


def test_the_new_entry_is_declared_bound_and_wrapped():
    from imageprocessor_amd import _lib
    h = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ipx.h")).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, h)
    assert NAME in _lib.SIGNATURES
    # the prototype's parameter count is the ctypes table's, and it takes the frame struct the PNG entry takes
    params = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % NAME, h, flags=re.S).group(1)
    assert params.count(",") + 1 == len(_lib.SIGNATURES[NAME][1]) == 7
    assert "const ipx_rgba_frame *frames" in params and "int quality" in params
    assert h.index("} ipx_rgba_frame;") < h.index(NAME)
    # the leg's contract no longer says that there is no such encode
    assert "no mixed-size jpeg.Encode" not in re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "ipx.h")).read())
    go = open(os.path.join(ROOT, "go", "ipx", "jpeg_mixed.go")).read()
    assert "func (x *Context) EncodeJPEGMixed(" in go and "C.ipx_jpeg_encode_mixed_dev(" in go
    import imageprocessor_amd as m
    assert hasattr(m.Context, "jpeg_encode_mixed_dev")
    # the sources of the feature are in the build's lists
    from imageprocessor_amd import build
    assert "ipx_jpeg_enc_mixed_plan.h" in build.HEADERS and "ipx_jpeg_runtime.hip" in build.SOURCES and "ipx_jpeg_legs.hip" in build.SOURCES
    assert {f for f in os.listdir(build.CSRC) if f.endswith((".h", ".inc"))} <= set(build.HEADERS)
    assert {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))} <= set(build.SOURCES)


def test_the_library_exports_the_new_entry():
    from imageprocessor_amd import build
    build.build()
    import imageprocessor_amd as m
    assert hasattr(m.lib(), NAME)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_records_under_sanitizers(tmp_path):
    exe = str(tmp_path / "jpeg_enc_mixed_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "jpeg_enc_mixed_plan_test.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "jpeg enc mixed plan ok" in r.stdout
