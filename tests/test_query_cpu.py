"""CPU: what the ray-query GPU tests (tests/test_gpu_query.py) rely on, without a device.

The barycentric bound and the vertex convention of tests/query_common.py, evaluated on the oracle's hits of
the query tests' own rays with the kernel's float32 arithmetic emulated (fused multiply-adds included): when
this was written the worst ratio to the bound was 0.078 on default_emitter (1 313 triangle hits) and 0.053 on
the 30x70 sphere mesh (743), with no violation, and the float32 hit point reconstructed o + t d to 5.4e-6.  And the ctypes layout of sptr_ray_query against the header's
field order and size."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import query_common as Q
import refit_common as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_barycentric_bound_on_the_oracle_hits(cfg):
    name, p0, p1, _ = cfg
    scene = oracle.builtin_scene(name, p0, p1)
    rays = R.rays(oracle.camera(aspect=R.W / R.H))
    geom, prim, t, _ = oracle.Prepared(scene, bvh=True).intersect(rays)
    mask, tri = Q.triangle_hits(scene["tri_geom_first"], geom, prim)
    u, v = Q.emulated_uv(scene["positions"], scene["indices"], rays[mask], tri)
    ratio = Q.check_barycentrics(u, v, scene["positions"], scene["indices"], rays[mask], tri, f"{name} emulated float32")
    assert ratio <= 1.0 / 3.0  # the factor the bound keeps in hand
    # the convention against the oracle's own distance: the float32 hit point reconstructs o + t d
    p = scene["positions"].astype(np.float64)
    i = scene["indices"].astype(np.int64)[tri]
    w = 1.0 - u.astype(np.float64) - v.astype(np.float64)
    point = w[:, None] * p[i[:, 0]] + u[:, None].astype(np.float64) * p[i[:, 1]] + v[:, None].astype(np.float64) * p[i[:, 2]]
    r = rays[mask].astype(np.float64)
    gap = np.linalg.norm(point - (r[:, 0:3] + t[mask].astype(np.float64)[:, None] * r[:, 3:6]), axis=1)
    print(f"{name}: worst |(1-u-v) v0 + u v1 + v v2 - (o + t d)| = {gap.max():.2e}")
    # u, v and t each carry a few float32 roundings of coordinates and distances of up to ~20: 2^-24 * 20 * 16
    assert gap.max() <= 2e-5


def test_a_swapped_convention_fails_the_check():
    """The check tells u from v: the bound is far below the barycentrics' own size."""
    name, p0, p1, _ = R.SCENES[1]
    scene = oracle.builtin_scene(name, p0, p1)
    rays = R.rays(oracle.camera(aspect=R.W / R.H))
    geom, prim, _, _ = oracle.Prepared(scene, bvh=True).intersect(rays)
    mask, tri = Q.triangle_hits(scene["tri_geom_first"], geom, prim)
    u, v = Q.emulated_uv(scene["positions"], scene["indices"], rays[mask], tri)
    with pytest.raises(AssertionError):
        Q.check_barycentrics(v, u, scene["positions"], scene["indices"], rays[mask], tri, "swapped")


def _header_struct(name):
    """[(C type, field)] of `typedef struct name {...} name;` in include/sptr_hip.h, in order."""
    with open(os.path.join(ROOT, "include", "sptr_hip.h")) as f:
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


def test_ray_query_struct_layout():
    import sptr

    fields = _header_struct("sptr_ray_query")
    assert [f[2] for f in fields] == [n for n, _ in sptr.RayQuery._fields_]
    scalar = {"uint32_t": (C.c_uint32, 4), "uint64_t": (C.c_uint64, 8)}
    off = 0
    for (ctype, ptr, name, count), (pname, ptype) in zip(fields, sptr.RayQuery._fields_):
        size = 8 if ptr else scalar[ctype][1]
        align = size
        off = (off + align - 1) // align * align
        desc = getattr(sptr.RayQuery, pname)
        assert desc.offset == off, (name, desc.offset, off)
        assert desc.size == size * max(1, count), name
        if ptr:
            assert ptype is C.c_void_p
        elif count:
            assert ptype._type_ is scalar[ctype][0] and ptype._length_ == count
        else:
            assert ptype is scalar[ctype][0]
        off += size * max(1, count)
    assert C.sizeof(sptr.RayQuery) == (off + 7) // 8 * 8 == 96
    for flag, value in (("SPTR_QUERY_ANY_HIT", 1), ("SPTR_QUERY_DEVICE_PTRS", 2), ("SPTR_QUERY_SORT", 4),
                        ("SPTR_QUERY_NO_SORT", 8)):
        assert getattr(sptr, flag) == value
        with open(os.path.join(ROOT, "include", "sptr_hip.h")) as f:
            assert re.search(r"%s = %du" % (flag, value), f.read())


# ------------------------------------------------------------- the host path the four query kinds share
def test_query_stage_cpp(tmp_path):
    """tests/cpp/test_query_stage.cpp, a stand-alone program over csrc/query_stage.h built with
    -fsanitize=address,undefined: the staging layout of the four kinds' field tables up to 2^28 rows."""
    import subprocess

    exe = tmp_path / "tqs"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "simple-path-tracer_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_query_stage.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"query_stage: (\d+) tables, 0 failures", out.stdout)
    assert m and int(m.group(1)) >= 6 * 4 + 21  # four tables at six counts, multi-hit at every (n, K) with n K <= 2^28


_RAY_LIST = "geom, prim, t, ng, uv"
_POINT_LIST = "['geom', 'prim', 'dist2', 'dist', 'point', 'uv', 'ng']"
_SIGNED_LIST = _POINT_LIST[:-1] + ", 'signed_dist', 'normal', 'feature']"
# method, row width, table, extra arguments, how its messages list the fields, how they state the size of out['ng']
_HELPER_KINDS = [
    ("query_rays", 8, "_QUERY_FIELDS", {}, _RAY_LIST, "5 x 3"),
    ("query_multi_hit", 8, "_QUERY_FIELDS", dict(per_row=2, always=(("count", 1, np.uint32),)), _RAY_LIST, "(5, 2, 3)"),
    ("query_points", 4, "_POINT_FIELDS", {}, _POINT_LIST, "5 x 3"),
    ("query_signed_distance", 4, "_POINT_FIELDS+_SIGNED_FIELDS", {}, _SIGNED_LIST, "5 x 3"),
]


@pytest.mark.parametrize("who,width,tables,extra,listing,ng_size", _HELPER_KINDS, ids=[k[0] for k in _HELPER_KINDS])
def test_query_arrays_helper(who, width, tables, extra, listing, ng_size):
    """sptr._query_arrays with numpy inputs and no Renderer: what the four methods return and raise (the texts are
    those of the methods before they shared the helper)."""
    import sptr

    table = sum((getattr(sptr, t) for t in tables.split("+")), ())
    K = extra.get("per_row")
    head = ["count"] if K else []
    n = 5
    x = np.arange(n * width, dtype=np.float64).reshape(n, width)  # (the helper converts to float32)

    def shape(name, rows=n):
        if name == "count":
            return (rows,)
        cols = dict((f, c) for f, c, _ in table)[name]
        return (rows,) + ((K,) if K else ()) + ((cols,) if cols > 1 else ())

    def call(fields=None, out=None, stream=None, inp=x):
        return sptr._query_arrays(inp, width, who, table, fields, out, stream, **extra)

    xin, got_n, device, res, addr = call()
    assert got_n == n and device is False and xin.dtype == np.float32 and xin.shape == (n, width) and xin.flags.c_contiguous
    assert (xin == x).all() and addr(xin) == xin.ctypes.data
    assert list(res) == head + [f for f, _, _ in table]  # the default: every field, in the table's order
    dtypes = dict([("count", np.uint32)] + [(f, d) for f, _, d in table])
    for name, a in res.items():
        assert a.shape == shape(name) and a.dtype == dtypes[name] and a.flags.c_contiguous and not a.any(), name
        assert addr(a) == a.ctypes.data
    for name, _, _ in table:  # a one-field subset: exactly that key (and what every result holds)
        one = call(fields=(name,))[3]
        assert list(one) == head + [name] and one[name].shape == shape(name) and one[name].dtype == dtypes[name]
    assert list(call(fields=())[3]) == head
    with pytest.raises(sptr.SptrError) as e:
        call(fields=("geom", "colour"))
    assert str(e.value) == f"{who}: fields must name some of {listing} (got ['geom', 'colour'])"
    if head:
        with pytest.raises(sptr.SptrError):  # (not a field to choose: every result holds it)
            call(fields=("count",))
    # out: taken as it is when it fits; refused by dtype, contiguity or size
    mine = np.zeros(shape("ng"), np.float32)
    assert call(out={"ng": mine})[3]["ng"] is mine
    assert call(fields=("geom",), out={"ng": mine})[3].keys() == set(head + ["geom"])  # (an out that is not wanted)
    text = f"{who}: out['ng'] must be contiguous, of {ng_size} float32"
    wide = np.zeros(shape("ng")[:-1] + (6,), np.float32)
    for bad in (np.zeros(shape("ng"), np.float64), wide[..., ::2], np.zeros(shape("ng", n + 1), np.float32),
                np.zeros(shape("ng"), np.float32).tolist()):
        with pytest.raises(sptr.SptrError) as e:
            call(out={"ng": bad})
        assert str(e.value) == text
    if head:
        with pytest.raises(sptr.SptrError) as e:
            call(out={"count": np.zeros(n, np.int32)})
        assert str(e.value) == f"{who}: out['count'] must be contiguous, of (5,) uint32"
    with pytest.raises(sptr.SptrError) as e:
        call(stream=1234)
    assert str(e.value) == f"{who}: a stream needs device tensors"
    # n == 0
    xin, got_n, device, res, addr = call(inp=np.zeros((0, width), np.float32))
    assert got_n == 0 and not device and list(res) == head + [f for f, _, _ in table]
    for name, a in res.items():
        assert a.shape == shape(name, 0) and a.dtype == dtypes[name], name


def test_query_flags():
    import sptr

    D, S, N = sptr.SPTR_QUERY_DEVICE_PTRS, sptr.SPTR_QUERY_SORT, sptr.SPTR_QUERY_NO_SORT
    assert [sptr._query_flags(s, d) for s in (None, True, False) for d in (False, True)] == [0, D, S, S | D, N, N | D]
