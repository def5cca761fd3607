"""The shadow entry table's cell tests (csrc/shadow_entry.h) on the CPU: tests/cpp/test_shadow_entry.cpp places
origins and primitives under axis-aligned, oblique and nearly horizontal lights and checks that whatever a
float64 ray from an origin along the light hits is never reported outside the origin's cell, and that clearly
separated primitives are reported outside."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shadow_entry_cpp(tmp_path):
    exe = tmp_path / "tse"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "simple-path-tracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_shadow_entry.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
