"""Shared inputs of the transform tests (test_transform_cpu.py, test_gpu_transforms.py): two composite scenes
of three triangle geometries each, the per-geometry matrices of step k, and the float32 restatement of the
device's per-vertex arithmetic.  Rays and the comparison rule are tests/refit_common.py's.

Scenes, composed in numpy from builtin-scene pieces (the same function serves sptr.builtin_scene's arrays and
the oracle's):
  lds : default_emitter's cube geometry (12 triangles, centre (0, 1, 2)) three times, shifted by x = -4, 0, 4,
        plus its 9 spheres: 3 triangle geometries in a BVH2 staged in LDS (leaf ranges of 8);
  wide: the sphere_mesh 30 70 mesh geometry (radius 0.75, centre (0, 1, 2)) three times, shifted by x = -2.5,
        0, 2.5, plus its 8 spheres, with set_bvh_width(4): treelets, the quantised BVH4 walked from L2.
Every copy has vertices of its own, so a vertex belongs to one geometry.

Step k (k = 0: identity, bit for bit): geometry g turns by 0.4 k (g + 1) about AXES[g] through its own centre
c_g, is scaled by (1 + 0.1 k g, 1, 1 - 0.05 k) there, and moves by k * SHIFT[g]:
M = T(c_g + k SHIFT[g]) R S T(-c_g), composed in float64 and cast to float32, stored glm style M[col][row].
The spheres of step k are refit_common.deform's.  transform_point is the device's arithmetic in numpy float32:
per component (M[0][k] x + M[1][k] y) + (M[2][k] z + M[3][k] 1), every product and sum rounded to float32, so
expected() gives the world positions sptr_update_transforms must produce bit for bit."""
import numpy as np

import refit_common as R

# name, builtin scene, p0, p1, set_bvh_width, x shifts of the three copies
SCENES = [("lds", "default_emitter", 0, 0, 0, (-4.0, 0.0, 4.0)), ("wide", "sphere_mesh", 30, 70, 4, (-2.5, 0.0, 2.5))]
SCENE_IDS = [s[0] for s in SCENES]
CENTRE = np.array([0.0, 1.0, 2.0])  # of the builtin scenes' one triangle geometry
AXES = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
SHIFT = np.array([[0.35, 0.1, -0.3], [-0.1, 0.25, 0.2], [-0.3, 0.15, -0.45]])


def compose(base: dict, shifts) -> dict:
    """base: positions (V,3), indices (T,3), tri_geom_first (2,), spheres (S,4), geom_material (1+S,) of a builtin
    scene with one triangle geometry.  Returns the same arrays with that geometry once per shift."""
    assert len(base["tri_geom_first"]) == 2
    p = np.asarray(base["positions"], np.float32)
    i = np.asarray(base["indices"], np.uint32)
    pos, idx = [], []
    for g, dx in enumerate(shifts):
        q = p.copy()
        q[:, 0] += np.float32(dx)
        pos.append(q)
        idx.append(i + np.uint32(g * len(p)))
    gm = np.asarray(base["geom_material"], np.uint32)
    out = {"positions": np.concatenate(pos), "indices": np.concatenate(idx),
           "tri_geom_first": (np.arange(len(shifts) + 1) * len(i)).astype(np.uint32),
           "spheres": np.asarray(base["spheres"], np.float32).copy(),
           "geom_material": np.concatenate([np.repeat(gm[:1], len(shifts)), gm[1:]]).astype(np.uint32)}
    for a in out.values():
        a.setflags(write=False)
    return out


def _rotation(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)


def matrices(shifts, k: int) -> np.ndarray:
    """(G, 4, 4) float32, [g][col][row]."""
    out = np.zeros((len(shifts), 4, 4), np.float32)
    for g, dx in enumerate(shifts):
        c = CENTRE + np.array([dx, 0.0, 0.0])
        A = _rotation(AXES[g], 0.4 * k * (g + 1)) @ np.diag([1.0 + 0.1 * k * g, 1.0, 1.0 - 0.05 * k])  # row-major 3x3
        M = np.eye(4)
        M[:3, :3] = A
        M[:3, 3] = c + k * SHIFT[g] - A @ c
        out[g] = M.T.astype(np.float32)  # glm: [col][row]
    out.setflags(write=False)
    return out


def identity(n: int) -> np.ndarray:
    return np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))


def transform_point(M: np.ndarray, p: np.ndarray) -> np.ndarray:
    """M (4,4) float32 [col][row], p (N,3) float32 -> (N,3) float32, the order of scene::transform_point."""
    M = np.asarray(M, np.float32)
    p = np.asarray(p, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    one = np.float32(1.0)
    for k in range(3):
        m0, m1, m2, m3 = M[0, k] * x, M[1, k] * y, M[2, k] * z, M[3, k] * one
        out[:, k] = (m0 + m1) + (m2 + m3)
    assert out.dtype == np.float32
    return out


def transform_geometries(scene: dict, mats: np.ndarray, rest=None) -> np.ndarray:
    """World positions (V,3) float32: the vertices of geometry g (each copy owns its vertices) through mats[g]."""
    rest = np.asarray(scene["positions"] if rest is None else rest, np.float32)
    out = rest.copy()
    first = scene["tri_geom_first"]
    idx = np.asarray(scene["indices"])
    for g in range(len(first) - 1):
        v = np.unique(idx[first[g]:first[g + 1]])
        out[v] = transform_point(mats[g], rest[v])
    return out


def expected(scene: dict, shifts, k: int):
    """(positions, spheres) of step k, read-only."""
    pos = transform_geometries(scene, matrices(shifts, k))
    sph = R.deform(scene["positions"], scene["spheres"], k)[1]
    pos.setflags(write=False)
    sph.setflags(write=False)
    return pos, sph
