"""GIF uploads of mixed sizes in one batch, the part that needs no GPU: the three new entries and ipx_gif_frame are declared in the
header, bound in the ctypes table, wrapped in Python and called from the Go source; the library exports them; and the per-frame records
of the mixed-size gif.Encode (csrc/ipx_gif_mixed_plan.h) hold their rules in tools/gif_mixed_plan_test.cpp, built with the address and
undefined-behaviour sanitizers and run as a program of its own."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ipx_gif_decode_mixed", "ipx_gif_encode_mixed_dev", "ipx_run_gif_gif_mixed"]


def test_the_new_entries_are_declared_bound_and_wrapped():
    from imageprocessor_amd import _lib
    h = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ipx.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, h), n
        assert n in _lib.SIGNATURES, n
    # the struct: the header's fields, in order, are the ctypes mirror's
    body = re.search(r"typedef struct \{([^}]*)\} ipx_gif_frame;", h)
    assert body
    fields = re.findall(r"\*?\b(\w+)\s*[,;]", body.group(1))
    assert fields == [f[0] for f in _lib.GifFrame._fields_] == ["w", "h", "index", "stride", "palette"], fields
    assert (_lib.GifFrame.w.offset, _lib.GifFrame.h.offset, _lib.GifFrame.index.offset, _lib.GifFrame.stride.offset,
            _lib.GifFrame.palette.offset, C.sizeof(_lib.GifFrame)) == (0, 4, 8, 16, 24, 32)
    # the prototypes' parameter counts are the ctypes table's
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % n, h, flags=re.S).group(1)
        assert params.count(",") + 1 == len(_lib.SIGNATURES[n][1]), n
    go = open(os.path.join(ROOT, "go", "ipx", "gif.go")).read()
    for fn, entry in (("GIFDecodeMixed", "ipx_gif_decode_mixed"), ("GIFEncodeMixedDev", "ipx_gif_encode_mixed_dev"),
                      ("RunGIFGIFMixed", "ipx_run_gif_gif_mixed")):
        assert "func (x *Context) %s(" % fn in go and "C.%s(" % entry in go, fn
    import imageprocessor_amd as m
    for n in ("gif_decode_mixed", "gif_encode_mixed_dev", "run_gif_gif_mixed"):
        assert hasattr(m.Context, n), n


def test_the_sources_are_in_the_build():
    from imageprocessor_amd import build
    assert "ipx_gif_mixed.hip" in build.SOURCES and "ipx_gif_mixed_plan.h" in build.HEADERS and "ipx_gif_kernels.h" in build.HEADERS
    assert {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))} <= set(build.SOURCES)


def test_the_library_exports_the_new_entries():
    from imageprocessor_amd import build
    build.build()
    import imageprocessor_amd as m
    L = m.lib()
    for n in NAMES:
        assert hasattr(L, n), n


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_encoders_records_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gif_mixed_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "gif_mixed_plan_test.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "gif mixed plan ok" in r.stdout
