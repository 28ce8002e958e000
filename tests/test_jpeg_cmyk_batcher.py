"""The micro-batcher's grouping key and four-component JPEGs, on the CPU: tools/sanitize/jpeg4_batcher_key_test.cpp drives
csrc/ipx_batcher.cpp against a fake backend under -fsanitize=address,undefined.  Files of one, three and four components with luma
sampling 1 x 1 and 2 x 2 arrive interleaved from four threads; no job the backend receives may mix component counts or samplings.
(jpeg_shape has always keyed on the component count: this passes before and after the four-component decoder.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_four_and_three_component_files_never_share_a_group(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "jpeg4_batcher_key_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tools", "sanitize", "jpeg4_batcher_key_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "mixed jobs: 0" in r.stdout and "jpeg4 batcher key ok" in r.stdout
