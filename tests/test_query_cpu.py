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
