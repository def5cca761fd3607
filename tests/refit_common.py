"""Shared inputs of the dynamic-scene tests (test_refit_cpu.py, test_gpu_refit.py): the two scene
configurations, the deformation, the rays and the comparison of two sets of query results.

Scenes: default_emitter (12 triangles + 9 spheres: an LDS-staged BVH2 with leaf ranges of 8) and the 30x70
sphere mesh with set_bvh_width(4) (treelets, the quantised BVH4 walked from L2).

Deformation k (float64, cast to float32): vertices: ang = 0.35 k (y - 1), (x, z - 2) rotated by ang,
y <- y (1 + 0.15 k) + 0.1 k; sphere i: centre += (0.3 k sin 1.7i, 0.2 k (i mod 3), 0.25 k cos 2.3i), radius
*= 1 + 0.1 k (2 (i mod 2) - 1).  An injective map of points: coincident vertices stay coincident, so a
triangle that is degenerate before is degenerate after.

Rays: the 150x82 pixel-centre rays of the default camera plus 8192 rays from default_rng(7), origins
uniform in [-6,6]x[0,5]x[-6,8] aimed at targets uniform in [-3,3]x[0,3]x[-3,5]: 20 492 in all.

Comparison: the results of two traversals of the same primitives are expected identical.  Allowed: at most
1e-4 of the rays (2 of 20 492) may name another (geomID, primID), and only with a bit-equal t (two
primitives at one distance, visited in another order); every other ray's geomID, primID, t and Ng are
bit-equal."""
import numpy as np

import denoise_ref as D

W, H = 150, 82
SCENES = [("default_emitter", 0, 0, 0), ("sphere_mesh", 30, 70, 4)]  # name, p0, p1, set_bvh_width
SCENE_IDS = [s[0] for s in SCENES]
CAP = 1e-4


def deform(positions: np.ndarray, spheres: np.ndarray, k: int):
    """(positions (V,3), spheres (S,4)) float32 of deformation k of the given float32 arrays; k = 0: copies."""
    p = np.asarray(positions, np.float64).reshape(-1, 3)
    s = np.asarray(spheres, np.float64).reshape(-1, 4)
    if k == 0:
        return p.astype(np.float32), s.astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2] - 2.0
    ang = 0.35 * k * (y - 1.0)
    ca, sa = np.cos(ang), np.sin(ang)
    q = np.stack([x * ca - z * sa, y * (1.0 + 0.15 * k) + 0.1 * k, 2.0 + x * sa + z * ca], axis=1)
    i = np.arange(len(s), dtype=np.float64)
    im = np.arange(len(s))
    t = s.copy()
    t[:, 0] += 0.3 * k * np.sin(1.7 * i)
    t[:, 1] += 0.2 * k * (im % 3)
    t[:, 2] += 0.25 * k * np.cos(2.3 * i)
    t[:, 3] *= 1.0 + 0.1 * k * (2 * (im % 2) - 1)
    return q.astype(np.float32), t.astype(np.float32)


def rays(cam: np.ndarray) -> np.ndarray:
    """(20492, 8) float32: o3 d3 tnear tfar."""
    rng = np.random.default_rng(7)
    o = rng.uniform([-6.0, 0.0, -6.0], [6.0, 5.0, 8.0], (8192, 3))
    tg = rng.uniform([-3.0, 0.0, -3.0], [3.0, 3.0, 5.0], (8192, 3))
    d = tg - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((8192, 8), np.float32)
    r[:, 0:3] = o
    r[:, 3:6] = d
    r[:, 7] = np.inf
    out = np.concatenate([D.pixel_centre_rays(cam, W, H), r], axis=0)
    out.setflags(write=False)
    return out


def compare_hits(a, b, what: str = "") -> int:
    """a, b: (geom, prim, t, ng).  Prints and returns the number of rays naming another primitive; asserts
    the rule of the module docstring."""
    ga, pa, ta, na = a
    gb, pb, tb, nb = b
    n = len(ga)
    ids = (ga != gb) | (pa != pb)
    t_eq = ta.view(np.uint32) == tb.view(np.uint32)
    ng_eq = (na.view(np.uint32) == nb.view(np.uint32)).all(axis=1)
    print(f"{what}: {int(ids.sum())} of {n} rays name another primitive, {int((~t_eq).sum())} differ in t, "
          f"{int((~ng_eq & ~ids).sum())} in Ng alone; {int((ga != 0xFFFFFFFF).sum())} hits")
    assert ids.sum() <= CAP * n
    assert t_eq[ids].all(), "a ray naming another primitive must report the same distance"
    assert t_eq[~ids].all() and ng_eq[~ids].all()
    return int(ids.sum())


def compare_occluded(a: np.ndarray, b: np.ndarray, what: str = "") -> int:
    d = int((a != b).sum())
    print(f"{what}: occluded differs on {d} of {len(a)} rays; {int(a.sum())} occluded")
    assert d <= CAP * len(a)
    return d
