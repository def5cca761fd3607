"""The SAH order of LDS-staged scenes (csrc/sah_order.h) on the CPU: tests/cpp/test_sah_order.cpp checks that the
path keys are unique and prefix-free, that the radix tree over the sorted keys is the builder's tree, the leaf
ranges' invariants, determinism and the fallback guards, on 1, 2 and 9 references, identical centres, a chain
70 deep, the default scene with its emitter and random scenes of 8 to 430 boxes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sah_order_cpp(tmp_path):
    exe = tmp_path / "tso"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "simple-path-tracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_sah_order.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
