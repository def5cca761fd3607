"""CPU: what the ray-render GPU tests (tests/test_gpu_ray_render.py) rely on, without a device.

The ctypes layout of sptr_ray_render against the header's field order and size, the flag values, the seed rule
of csrc/ray_batch.h against a numpy wang_hash, and tests/cpp/test_ray_batch.cpp: the chunk plan (every path
exactly once; whole rays unless one ray is split, then contiguous sample ranges in order; capacities 1, n - 1,
n, n + 1 and n * samples) and the rule itself in C++."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sptr_hip.h")


def wang_hash(a):
    """wf::wang_hash on uint32 arrays."""
    a = np.asarray(a, np.uint32).copy()
    a = (a ^ np.uint32(61)) ^ (a >> np.uint32(16))
    a = a * np.uint32(9)
    a = a ^ (a >> np.uint32(4))
    a = a * np.uint32(0x27D4EB2D)
    a = a ^ (a >> np.uint32(15))
    return a


def ray_rng(seeds, n, samples, frame_index, s):
    """The rng state of sample s of rays 0..n-1 (include/sptr_hip.h, sptr_render_rays)."""
    if seeds is not None and samples == 1:
        return np.asarray(seeds, np.uint32)
    b = np.asarray(seeds, np.uint32) if seeds is not None else np.arange(n, dtype=np.uint32)
    return wang_hash((b ^ np.uint32((frame_index + s) & 0xFFFFFFFF)) ^ np.uint32(1))


def _header_struct(name):
    """[(C type, is pointer, field, array length)] of `typedef struct name {...} name;` in the header, in order."""
    with open(HEADER) as f:
        text = f.read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)(\[(\d+)\])?", decl)
        assert m, decl
        out.append((m.group(2), bool(m.group(3)), m.group(4), int(m.group(6)) if m.group(6) else 0))
    return out


def test_ray_render_struct_layout():
    import sptr

    fields = _header_struct("sptr_ray_render")
    assert [f[2] for f in fields] == [n for n, _ in sptr.RayRender._fields_]
    assert [f[2] for f in fields] == ["rays", "seeds", "n", "samples", "frame_index", "max_depth", "flags", "radiance",
                                      "reserved"]
    scalar = {"uint32_t": (C.c_uint32, 4), "float": (C.c_float, 4)}
    off = 0
    for (ctype, ptr, name, count), (pname, ptype) in zip(fields, sptr.RayRender._fields_):
        size = 8 if ptr else scalar[ctype][1]
        off = (off + size - 1) // size * size
        desc = getattr(sptr.RayRender, pname)
        assert desc.offset == off, (name, desc.offset, off)
        assert desc.size == size * max(1, count), name
        if ptr:
            assert ptype is C.c_void_p
        elif count:
            assert ptype._type_ is scalar[ctype][0] and ptype._length_ == count
        else:
            assert ptype is scalar[ctype][0]
        off += size * max(1, count)
    assert C.sizeof(sptr.RayRender) == (off + 7) // 8 * 8 == 64
    with open(HEADER) as f:
        text = f.read()
    for flag, value in (("SPTR_RAYS_DEVICE_PTRS", 1), ("SPTR_RAYS_ACCUMULATE", 2), ("SPTR_RAYS_NORMALIZE", 4)):
        assert getattr(sptr, flag) == value
        assert re.search(r"%s = %du" % (flag, value), text)
    for sym in ("sptr_render_rays", "sptr_ray_render_info"):
        assert sym in sptr.EXPORTS and re.search(r"\bint %s\(" % sym, text)


def test_wang_hash_known_values():
    """The numpy hash is the reference's (include/wavefront/wf_math.h:35-43), evaluated by hand in Python ints."""
    def ref(a):
        a = ((a ^ 61) ^ (a >> 16)) & 0xFFFFFFFF
        a = (a * 9) & 0xFFFFFFFF
        a = a ^ (a >> 4)
        a = (a * 0x27D4EB2D) & 0xFFFFFFFF
        return a ^ (a >> 15)

    xs = [0, 1, 2, 61, 12299, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF]
    assert [int(v) for v in wang_hash(np.array(xs, np.uint32))] == [ref(x) for x in xs]


def test_seed_rule():
    n = 12300
    # no seeds: ray i draws what pixel i of frame frame_index + s draws, primary_at's wang_hash((ps ^ acc) ^ 1)
    for fi, s in ((1, 0), (7, 3), (0xFFFFFFF0, 4)):
        acc = np.uint32(fi + s)
        want = wang_hash((np.arange(n, dtype=np.uint32) ^ acc) ^ np.uint32(1))
        assert np.array_equal(ray_rng(None, n, 1, fi, s), want)
        assert np.array_equal(ray_rng(None, n, 5, fi, s), want)
    seeds = wang_hash(np.arange(n, dtype=np.uint32) + np.uint32(17))
    assert np.array_equal(ray_rng(seeds, n, 1, 9, 0), seeds)  # one sample: the seed itself
    got = ray_rng(seeds, n, 5, 9, 2)                           # several: b = seeds[i]
    assert np.array_equal(got, wang_hash((seeds ^ np.uint32(11)) ^ np.uint32(1)))
    assert not np.array_equal(got, seeds)


def test_ray_batch_cpp(tmp_path):
    exe = tmp_path / "trb"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "simple-path-tracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_ray_batch.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
