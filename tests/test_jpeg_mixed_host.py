"""JPEG uploads of mixed sizes in one batch, the part that needs no GPU: the two new entries and the frame struct are declared in the
header, bound in the ctypes table, wrapped in Python and called from the Go source; the built library exports them; and the host side
of the per-image records (csrc/ipx_jpeg_mixed_plan.h: 64-bit prefix sums of blocks, workgroups and plane bytes, the workgroup -> image
search) and the leg's cut by size and class hold their rules in tools/jpeg_mixed_plan_test.cpp, built with the address and
undefined-behaviour sanitizers and run as a program of its own."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ipx_jpeg_decode_mixed", "ipx_run_jpeg_jpeg_mixed"]


def test_the_new_entries_are_declared_bound_and_wrapped():
    from imageprocessor_amd import _lib
    h = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ipx.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, h), n
        assert n in _lib.SIGNATURES, n
        # the prototype's parameter count is the ctypes table's
        params = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % n, h, flags=re.S).group(1)
        assert params.count(",") + 1 == len(_lib.SIGNATURES[n][1]), n
    # the struct: the header's fields, in order, are the ctypes mirror's, with C's sizes and offsets on a 64-bit target
    body = re.search(r"typedef struct \{([^}]*)\} ipx_jpeg_frame;", h)
    assert body
    fields = re.findall(r"\*?\b(\w+)\s*[,;]", body.group(1))
    assert fields == [f[0] for f in _lib.JpegFrame._fields_] == ["w", "h", "ratio", "y", "cb", "cr", "ystride", "cstride"]
    F = _lib.JpegFrame
    assert [getattr(F, f).offset for f in fields] == [0, 4, 8, 16, 24, 32, 40, 44] and C.sizeof(F) == 48
    assert [getattr(F, f).size for f in fields] == [4, 4, 4, 8, 8, 8, 4, 4]
    go = open(os.path.join(ROOT, "go", "ipx", "jpeg_mixed.go")).read()
    assert "func (x *Context) DecodeJPEGMixed(" in go and "C.ipx_jpeg_decode_mixed(" in go
    assert "func (x *Context) RunJPEGJPEGMixed(" in go and "C.ipx_run_jpeg_jpeg_mixed(" in go
    import imageprocessor_amd as m
    for n in ("jpeg_decode_mixed", "run_jpeg_jpeg_mixed"):
        assert hasattr(m.Context, n), n
    # the sources of the feature are in the build's lists
    from imageprocessor_amd import build
    assert "ipx_jpeg_legs.hip" in build.SOURCES and "ipx_jpeg_mixed_plan.h" in build.HEADERS and "ipx_mixed_leg.h" in build.HEADERS
    assert "ipx_mixed_cut.h" in build.HEADERS and "ipx_align.h" in build.HEADERS
    # (build.py drops a listed header that does not exist: a renamed one would leave the rebuild check without a word)
    assert {f for f in os.listdir(build.CSRC) if f.endswith((".h", ".inc"))} <= set(build.HEADERS)


def test_the_library_exports_the_new_entries():
    from imageprocessor_amd import build
    build.build()
    import imageprocessor_amd as m
    L = m.lib()
    for n in NAMES:
        assert hasattr(L, n), n


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_records_and_the_cut_under_sanitizers(tmp_path):
    exe = str(tmp_path / "jpeg_mixed_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "jpeg_mixed_plan_test.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "jpeg mixed plan ok" in r.stdout
