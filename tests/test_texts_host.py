"""The micro-batcher's per-file text switch on the CPU: tools/texts_batcher_host_test.cpp binds ipx::Batcher to a fake backend (plain g++,
no GPU) and shows that with the switch on files differing only in their text share one job whose texts[i] is file i's own deep copy,
that with it off they go out as before, and that a 257-glyph text is refused at submit, alone.  The header, the ctypes table and the Go
text are held together by tests/test_abi.py and tests/test_go_binding_source.py; here, that the new names are where they belong."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batcher_groups_files_that_differ_only_in_text(tmp_path):
    exe = str(tmp_path / "texts_batcher_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-o", exe, os.path.join(ROOT, "tools", "texts_batcher_host_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "switch on: 8 files with 8 different texts in one job" in r.stdout
    assert "switch off: 9 jobs of one file each, texts == NULL" in r.stdout and "texts batcher ok" in r.stdout


def test_the_new_entries_are_declared_bound_and_wrapped():
    from imageprocessor_amd import _lib
    h = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ipx.h")).read(), flags=re.S)
    names = ["ipx_textset_create", "ipx_textset_destroy", "ipx_dev_composite_texts_rgba8", "ipx_plan_run_jpeg_jpeg_texts",
             "ipx_plan_run_png_png_texts", "ipx_plan_run_gif_gif_texts"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, h), n
        assert n in _lib.SIGNATURES, n
    # ipx_job ends in the texts, in the header and in the ctypes mirror, and ipx_text has the three fields in order
    job = re.search(r"typedef struct \{[^}]*\} ipx_job;", h, flags=re.S).group(0)
    assert re.search(r"const ipx_text \*texts;\s*\} ipx_job;", job)
    assert _lib.Job._fields_[-1][0] == "texts" and [f[0] for f in _lib.Text._fields_] == ["glyphs", "n_glyphs", "col"]
    go = "".join(open(os.path.join(ROOT, "go", "ipx", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "go", "ipx"))) if f.endswith(".go"))
    for n in ("type Text struct", "RunJPEGJPEGTexts(", "RunPNGPNGTexts(", "RunGIFGIFTexts(", "SubmitFilesTexts("):
        assert n in go, n
    for n in names[3:]:
        assert "C.%s(" % n in go, n
    import imageprocessor_amd as m
    assert hasattr(m, "TextSet") and hasattr(m.Context, "textset") and hasattr(m.Context, "dev_composite_texts")
