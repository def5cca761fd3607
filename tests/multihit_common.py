"""Shared inputs of the multi-hit tests (test_multihit_cpu.py, test_gpu_multihit.py): which scenes, rays and K, and
their references (tests/multihit_ref.py), each computed once per process and read-only.

Query scenes: refit_common.SCENES.  Rays: refit_common.rays' construction, 20 492 rays (the 150x82 pixel-centre rays
of the default camera plus 8192 random rays over the same boxes), with default_rng(SEED) in place of its
default_rng(7).  The GPU test excuses a ray only if one of its first K + 1 reference candidates is marginal in
float64, and at most refit_common.CAP of the rays (2 of them), so the ray set must hold no more marginal rays than
that; with K = 16 the random rays of seed 7 hold 4 (default_emitter) and 2 (sphere mesh), seeds 8, 9, 11 and 12
hold 1 to 6, seed 10 holds none in either scene, and the pixel-centre rays hold none
(tests/test_multihit_cpu.py asserts the condition).  Adversarial cases, by family and index
into adversarial_common.family():
  equal     K coincident triangles, K identical spheres and K concentric spheres for K in 2, 17, 64;
  spheres   origins inside, tangent rays, a zero-radius sphere; zero-radius spheres on a line and at one point;
  interval  ends of (tnear, tfar] one ulp around a hit;
  tiny      0, 1, 2, 5 and 9 primitives as triangles, spheres and mixed;
  staging   one triangle above the largest LDS-staged count, where split references are made (uploaded by the GPU test with set_bvh_width(4) and
            set_split_refs(8))."""
import functools

import numpy as np

import adversarial_common as A
import multihit_ref as MR
import oracle
import refit_common as R

KS = (1, 2, 4, 5, 16)
SEED = 10


def rays(cam):
    """(20492, 8) float32: o3 d3 tnear tfar; refit_common.rays with default_rng(SEED)."""
    base = R.rays(cam)
    rng = np.random.default_rng(SEED)
    o = rng.uniform([-6.0, 0.0, -6.0], [6.0, 5.0, 8.0], (8192, 3))
    tg = rng.uniform([-3.0, 0.0, -3.0], [3.0, 3.0, 5.0], (8192, 3))
    d = tg - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = base.copy()
    out[-8192:, 0:3] = o
    out[-8192:, 3:6] = d
    out.setflags(write=False)
    return out


_TINY = [3 * A.COUNTS.index(n) + kind for n in (0, 1, 2, 5, 9) for kind in range(3)]
ADVERSARIAL = ([("equal", i) for i in range(9)] + [("spheres", i) for i in range(3)] + [("interval", 0)]
               + [("tiny", i) for i in _TINY] + [("staging", 2)])


@functools.lru_cache(maxsize=None)
def scene_reference(name):
    """(flat scene dict, rays, multihit_ref.lists of them) of the query scene `name`."""
    cfg = next(c for c in R.SCENES if c[0] == name)
    scene = oracle.builtin_scene(cfg[0], cfg[1], cfg[2])
    rr = rays(oracle.camera(aspect=R.W / R.H))
    return scene, rr, MR.lists(scene, rr)


@functools.lru_cache(maxsize=None)
def case_reference(fam, k):
    """(adversarial case, multihit_ref.lists of its scene and rays)."""
    case = A.family(fam)[k]
    return case, MR.lists(case.scene, case.rays)
