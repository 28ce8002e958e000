"""The micro-batcher's format routing on the CPU, under ThreadSanitizer (tools/sanitize/run_tsan_formats.sh builds and runs
tools/sanitize/batcher_formats_host_test.cpp): PNG and GIF uploads are told from JPEG ones by the full signature, a group is one
format, and it goes to the backend as a job of that format."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batcher_routes_png_and_gif_groups_as_jobs_of_their_format_under_tsan():
    """8 submitters, 3600 files of six signatures (PNG, GIF87a, GIF89a, FF D8, and the look-alikes 89 50 and GIF8 that are neither),
    three sizes, two operator sets, against a fake backend that records every job's kind: one format per job and the one the files'
    signatures name (IPX_JOB_PNG, IPX_JOB_GIF, IPX_JOB_JPEG for everything else), every ticket its own bytes, max_batch held, a
    refused job fails its own files only, destruction with work pending, no sanitizer report."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "run_tsan_formats.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no sanitizer report" in r.stdout and "batcher formats ok" in r.stdout
