"""bench.py's command line: a plain run times the steps and prints the headline fields only, --full adds
the other measurements, --dump-outputs writes the last timed step's image (the C1 workload, the smallest)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "shadow_roofline", "output_check", "stage_ms_per_step", "stage_ms_untimed_step", "render_ms",
             "overlap_probe", "interactive", "cpu_baseline", "graph_replay")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_whole_and_sampled(bench, tmp_path, monkeypatch):
    """Arrays within the byte limit are written whole as float32; past it, each is cut to the same seeded
    sample of its flattened elements in every call, and the files together stay within the limit."""
    img = (np.arange(40 * 30 * 3) % 256).astype(np.uint8).reshape(30, 40, 3)
    bench.dump_outputs(str(tmp_path / "a"), {"image": img})
    a = np.load(tmp_path / "a" / "image.npy")
    assert a.dtype == np.float32 and a.shape == img.shape and np.array_equal(a, img)
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 2000)
    big = {"x": np.arange(1000, dtype=np.float64), "y": np.arange(100, dtype=np.int32)}
    bench.dump_outputs(str(tmp_path / "b"), big)
    bench.dump_outputs(str(tmp_path / "c"), big)
    x, y = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "b" / "y.npy")
    assert x.dtype == y.dtype == np.float32 and x.nbytes + y.nbytes <= 2000
    assert x.size == 250 and np.all(np.diff(x) > 0) and np.array_equal(y, big["y"])
    assert np.array_equal(x, np.load(tmp_path / "c" / "x.npy"))


def _run(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True,
                       text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_image(tmp_path):
    """A plain run: --steps sets the timed steps, the line holds the headline fields and none of the --full
    ones, and image.npy is the step's RGB8 image: the committed C1 fixture's, within the golden tests'
    exact-pixel fraction (tests/test_gpu_golden.py), and the same bytes in a second run."""
    lines = [_run(["--workload", "c1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)], 120)
             for d in ("a", "b")]
    line = lines[0]
    for k in HEADLINE:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["full"] is False
    assert line["value"] > 0 and line["rays_per_step"] > 256 * 256 * 4
    assert not [k for k in FULL_ONLY if k in line]
    a, b = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "b" / "image.npy")
    assert a.dtype == np.float32 and a.shape == (256, 256, 3) and np.array_equal(a, b)
    g = np.load(os.path.join(ROOT, "tests", "golden", "c1_default_256_4spp.npz"), allow_pickle=False)
    assert float((a == g["rgb"]).all(axis=2).mean()) >= 0.999


@pytest.mark.gpu
def test_full_run_reports_the_other_measurements():
    """--full: the same headline plus the rooflines, the output check (identical to an untimed render) and
    the stage timings; the interactive legs and the CPU baseline are switched off here to keep the test short
    (they run in a --full run without these flags)."""
    line = _run(["--workload", "c1", "--steps", "2", "--warmup", "1", "--full", "--no-interactive",
                 "--no-cpu-baseline"], 180)
    for k in HEADLINE + ("roofline", "shadow_roofline", "output_check", "stage_ms_per_step", "stage_ms_untimed_step",
                         "render_ms", "overlap_probe", "step_roofline", "pixel_lanes", "graph_replay", "cpu_baseline"):
        assert k in line, k
    assert line["full"] is True and line["output_check"]["identical"] is True
