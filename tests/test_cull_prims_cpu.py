"""The bounce-0 cull's exact primitive tests (csrc/cull_prims.h) on the CPU: tests/cpp/test_cull_prims.cpp
checks every "outside" answer of seeded sphere and triangle cases against a dense float64 ray bundle,
and that clearly separated primitives are reported outside."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cull_prims_cpp(tmp_path):
    exe = tmp_path / "tcp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "simple-path-tracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_cull_prims.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
