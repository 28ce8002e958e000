"""bench.py's two kinds of run: a plain one does what the headline figure needs and nothing else, `--full` adds the check against
the oracle, the copy ceiling, the CPU baseline and the PCIe-inclusive legs.  The result line keeps its headline keys in both."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_an_option_and_off_by_default(monkeypatch):
    assert _parse(["--gpus", "1", "--steps", "5", "--warmup", "2"], monkeypatch).full is False
    assert _parse(["--gpus", "1", "--steps", "5", "--warmup", "2", "--full"], monkeypatch).full is True


def _run(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "64"] + list(argv),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_measures_nothing_else():
    d = _run()
    assert all(k in d for k in HEADLINE) and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["roofline"]["avg_launch_ms"] > 0                      # from the events of the timed steps themselves
    assert d["checked"] is False and d["cpu_baseline"] is None and d["e2e"] is None
    assert "copy_ceiling" not in d["roofline"] and "frac_of_copy_ceiling" not in d["roofline"]


@pytest.mark.gpu
def test_full_run_checks_and_measures_the_rest():
    d = _run("--full", "--cpu-seconds", "0.5", "--copy-gib", "1", "--e2e-frames", "16", "--e2e-reps", "1")
    assert all(k in d for k in HEADLINE) and d["value"] > 0
    assert d["checked"] is True
    assert d["roofline"]["copy_ceiling"]["best"] > 0 and d["roofline"]["frac_of_copy_ceiling"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["at_reference_concurrency_3"] > 0
    assert set(d["e2e"]["legs"]) == {"pixels_to_pixels", "pixels_to_jpeg", "jpeg_to_jpeg", "pool_pixels_to_pixels"}
    assert all(leg["images_per_s"] > 0 for leg in d["e2e"]["legs"].values())
