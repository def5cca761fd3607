"""CPU: what the adaptive-sampling GPU tests (tests/test_gpu_adaptive.py) rely on, without a device.

The ctypes layouts of sptr_adaptive_params / sptr_adaptive_info against the header; tests/adaptive_ref.py on
synthetic samples; and tests/cpp/test_adaptive_rule.cpp, a stand-alone program built with
-fsanitize=address,undefined that prints what csrc/adaptive_rule.h (the text the kernels call) computes for a
table of inputs, compared here bit for bit with adaptive_ref, and checks the chunk plan over a list."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import adaptive_ref as AR
from test_ray_render_cpu import HEADER, ROOT, _header_struct

F = np.float32


def _layout(struct, name, want_fields, want_size):
    fields = _header_struct(name)
    assert [f[2] for f in fields] == [n for n, _ in struct._fields_] == want_fields
    scalar = {"uint32_t": (C.c_uint32, 4), "float": (C.c_float, 4), "uint64_t": (C.c_uint64, 8), "double": (C.c_double, 8)}
    off = 0
    for (ctype, ptr, fname, count), (pname, ptype) in zip(fields, struct._fields_):
        assert not ptr
        size = scalar[ctype][1]
        off = (off + size - 1) // size * size
        desc = getattr(struct, pname)
        assert desc.offset == off, (fname, desc.offset, off)
        assert desc.size == size * max(1, count), fname
        if count:
            assert ptype._type_ is scalar[ctype][0] and ptype._length_ == count
        else:
            assert ptype is scalar[ctype][0]
        off += size * max(1, count)
    assert C.sizeof(struct) == (off + 7) // 8 * 8 == want_size


def _header_decls(name):
    """The header's struct with `a, b` declarators split into one field each (as _header_struct expects)."""
    with open(HEADER) as f:
        text = f.read()
    return re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)


def test_struct_layouts():
    import sptr

    _layout(sptr.AdaptiveParams, "sptr_adaptive_params", ["threshold", "min_samples", "max_samples", "step", "flags", "reserved"], 32)
    # sptr_adaptive_info declares several fields per line: the order and types, field by field
    body = re.sub(r"/\*.*?\*/", "", _header_decls("sptr_adaptive_info"), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for nm in names.split(","):
            m = re.fullmatch(r"(\w+)(\[(\d+)\])?", nm.strip())
            fields.append((ctype, m.group(1), int(m.group(3)) if m.group(3) else 0))
    want = [("uint64_t", "samples", 0), ("uint64_t", "rays_closest", 0), ("uint64_t", "rays_shadow", 0), ("uint32_t", "passes", 0),
            ("uint32_t", "chunks", 0), ("uint32_t", "active_first", 0), ("uint32_t", "active_last", 0), ("uint32_t", "min_count", 0),
            ("uint32_t", "max_count", 0), ("double", "ms", 0), ("uint32_t", "reserved", 4)]
    assert fields == want
    ct = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}
    off = 0
    for (ctype, name, count), (pname, ptype) in zip(fields, sptr.AdaptiveInfo._fields_):
        assert name == pname
        size = C.sizeof(ct[ctype])
        off = (off + size - 1) // size * size
        assert getattr(sptr.AdaptiveInfo, pname).offset == off, name
        assert (ptype._type_ is ct[ctype] and ptype._length_ == count) if count else ptype is ct[ctype]
        off += size * max(1, count)
    assert C.sizeof(sptr.AdaptiveInfo) == (off + 7) // 8 * 8 == 72
    with open(HEADER) as f:
        text = f.read()
    assert sptr.SPTR_ADAPTIVE_CONTINUE == 1 and re.search(r"SPTR_ADAPTIVE_CONTINUE = 1u", text)
    assert re.search(r"#define SPTR_ABI_VERSION 9\b", text) and sptr.SPTR_ABI_VERSION == 9
    for sym in ("sptr_render_adaptive", "sptr_read_sample_counts"):
        assert sym in sptr.EXPORTS and re.search(r"\bint %s\(" % sym, text)


def _noise(P, n, seed=7):
    """P pixels x n samples: pixel p's samples are 1 + noise of amplitude p / P (pixel 0 is constant)."""
    rng = np.random.default_rng(seed)
    amp = (np.arange(P, dtype=F) / F(P))[None, :, None]
    return (F(1.0) + amp * (rng.random((n, P, 3), dtype=F) - F(0.5))).astype(F)


def test_ref_threshold_zero_takes_max_everywhere():
    L = _noise(50, 11)
    L[:, 0] = F(0.25)  # a constant pixel has err 0, and 0 < 0 is false
    S, E, n, passes = AR.run(L, 0.0, 4, 11, 3)
    assert (n == 11).all() and passes == 1 + 3  # takes 4, 3, 3, 1
    want = np.zeros((50, 3), F)
    even = np.zeros((50, 3), F)
    for i in range(1, 12):
        want = want + L[i - 1]
        if i % 2 == 0:
            even = even + L[i - 1]
    assert np.array_equal(S.view(np.uint32), want.view(np.uint32)) and np.array_equal(E.view(np.uint32), even.view(np.uint32))


def test_ref_huge_threshold_takes_min():
    S, E, n, passes = AR.run(_noise(50, 32), 1e30, 8, 32, 4)
    assert (n == 8).all() and passes == 1


def test_ref_constant_pixels_stop_at_min():
    L = np.full((32, 9, 3), F(0.75))  # (dyadic: the sums are exact, so the two means are equal)
    L[:, 3] = F(0.0)  # black: the denominator sits at its floor
    assert (AR.err(L[:8].sum(0), L[1:8:2].sum(0), np.full(9, 8)) == 0).all()
    S, E, n, passes = AR.run(L, 0.02, 8, 32, 4)
    assert (n == 8).all() and passes == 1


def test_ref_nan_runs_to_max():
    L = np.full((32, 4, 3), F(0.7))
    L[2, 1, 0] = np.nan   # pixel 1: a NaN in sample 3 (odd: S only)
    L[3, 2, 1] = np.nan   # pixel 2: in sample 4 (even: S and E)
    S, E, n, passes = AR.run(L, 0.02, 8, 32, 4)
    assert n.tolist() == [8, 32, 32, 8] and passes == 7
    assert np.isnan(S[1, 0]) and not np.isnan(E[1]).any() and np.isnan(E[2, 1])
    # n = 1 is well defined: E / 0 with E = 0 is a NaN, which is not below any threshold
    assert AR.active(L[0], np.zeros((4, 3), F), np.ones(4, np.uint32), 1e30, 1, 32).all()


def test_ref_last_take_is_cut():
    L = _noise(40, 7)
    S, E, n, passes = AR.run(L, 0.0, 2, 7, 3)
    assert (n == 7).all() and passes == 3  # 2 + 3 + 2
    assert AR.take(np.array([0, 2, 5, 6]), 2, 7, 3).tolist() == [2, 3, 2, 1]


def test_ref_continue_equals_one_call():
    L = _noise(300, 32)
    one = AR.run(L, 0.004, 8, 32, 4)
    assert len(np.unique(one[2])) >= 4  # pixels stop at several counts
    first = AR.run(L, 0.004, 8, 16, 4)
    second = AR.run(L, 0.004, 8, 32, 4, state=first[:3])
    for a, b in zip(one[:3], second[:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert first[3] + second[3] == one[3]
    # a sample function instead of an array, asked only for indices within 1 .. max
    asked = set()

    def sample(i):
        asked.add(i)
        return L[i - 1]

    again = AR.run(sample, 0.004, 8, 32, 4)
    assert np.array_equal(again[2], one[2]) and asked == set(range(1, 33))


def test_adaptive_rule_cpp(tmp_path):
    """The header's err bits, predicate, take and key for the program's table against adaptive_ref; the plan."""
    exe = tmp_path / "tar"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "simple-path-tracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_adaptive_rule.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rules = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("RULE ")]
    plans = [ln for ln in out.stdout.splitlines() if ln.startswith("PLAN ")]
    assert len(rules) > 1500 and len(plans) >= 5 * 4 * 5 and all(p.endswith(" ok") for p in plans)
    f32 = lambda words: np.array([int(w, 16) for w in words], np.uint32).view(F)  # noqa: E731
    S = np.stack([f32([r[1 + k] for r in rules]) for k in range(3)], axis=1)
    E = np.stack([f32([r[4 + k] for r in rules]) for k in range(3)], axis=1)
    n = np.array([int(r[7]) for r in rules], np.uint32)
    thr = f32([r[8] for r in rules])
    mn, mx, st = (np.array([int(r[9 + k]) for r in rules], np.int64) for k in range(3))
    assert all(r[12] == "->" for r in rules)
    got_err = np.array([int(r[13], 16) for r in rules], np.uint32)
    got_act = np.array([int(r[14]) for r in rules], bool)
    got_take = np.array([int(r[15]) for r in rules], np.int64)
    got_key = np.array([int(r[16]) for r in rules], np.int64)
    want_err = AR.err(S, E, n).view(np.uint32)
    nan = np.isnan(want_err.view(F))
    assert np.array_equal(np.isnan(got_err.view(F)), nan)          # (a NaN's payload is not part of the rule)
    assert np.array_equal(got_err[~nan], want_err[~nan])
    want_act = np.array([AR.active(S[i], E[i], n[i], thr[i], mn[i], mx[i]) for i in range(len(n))], bool)
    assert np.array_equal(got_act, want_act)
    below = n < mx
    want_take = np.array([AR.take(n[i], mn[i], mx[i], st[i]) for i in range(len(n))], np.int64)
    assert np.array_equal(got_take[below], want_take[below]) and (got_take[~below] == 0).all()
    assert np.array_equal(got_key[below], np.where(n[below] == 0, 0x7FFFFFFF, want_take[below]))
    # the table exercises both outcomes at counts between min and max
    mid = (n >= mn) & (n < mx)
    assert got_act[mid].any() and (~got_act[mid]).any() and nan.any() and (~nan).any()
