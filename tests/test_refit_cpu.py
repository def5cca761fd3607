"""CPU: the inputs of the dynamic-scene GPU tests (tests/test_gpu_refit.py) on the oracle alone.

The GPU tests compare two traversals of the same moved primitives (a refitted tree against a freshly built
one) and allow 1e-4 of the rays to name another primitive at a bit-equal distance.  Here the same
comparison is made between the oracle's BVH and its brute-force loop over every primitive, on the same
scenes, deformations and rays: 0 of 20 492 rays disagreed when this was written, for both scenes and
k = 0, 1, 2, so the scenes hold no distance ties and the cap is reachable by the reference alone.  The
deformation must also matter: it changed the result of 30-37 % of the rays, so a refit that does nothing
cannot pass; a fifth is asserted."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
import refit_common as R


@pytest.fixture(scope="module")
def query_rays():
    return R.rays(oracle.camera(aspect=R.W / R.H))


@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_deformed_scenes_have_no_distance_ties(cfg, query_rays):
    name, p0, p1, _ = cfg
    scene = oracle.builtin_scene(name, p0, p1)

    def both(k):
        pos, sph = R.deform(scene["positions"], scene["spheres"], k)
        P = oracle.Prepared(dict(scene, positions=pos, spheres=sph), bvh=True)
        return P.intersect(query_rays, use_bvh=True), P.intersect(query_rays, use_bvh=False)

    with ThreadPoolExecutor(3) as pool:  # (the brute-force loops run outside the interpreter lock)
        res = list(pool.map(both, (0, 1, 2)))
    for k, (tree, brute) in enumerate(res):
        R.compare_hits(tree, brute, f"{name} k={k} oracle BVH vs brute force")
        if k:
            base = res[0][1]
            changed = (brute[0] != base[0]) | (brute[1] != base[1]) | (brute[2].view(np.uint32) != base[2].view(np.uint32))
            print(f"{name} k={k}: the deformation changes {changed.mean():.3f} of the rays' results")
            assert changed.mean() >= 0.2


def test_deformation_keeps_coincident_vertices_coincident():
    scene = oracle.builtin_scene("sphere_mesh", 30, 70)
    p0 = scene["positions"]
    for k in (1, 2):
        p, _ = R.deform(p0, scene["spheres"], k)
        _, inv0 = np.unique(p0.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
        _, inv1 = np.unique(p.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
        # vertices equal before are equal after (the reverse may fail only by float32 rounding)
        first = {}
        for a, b in zip(inv0.ravel(), inv1.ravel()):
            assert first.setdefault(int(a), int(b)) == int(b)
