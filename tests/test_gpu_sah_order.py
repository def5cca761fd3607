"""GPU tests of the SAH order of LDS-staged scenes (csrc/sah_order.h through build_lbvh; sptr_set_tree_order,
sptr_tree_info).

1. Hits: 2 and 9 primitives, 40 triangles whose box centres are all exactly 0, the default scene with its
   emitter and the largest scene that is staged into LDS, each uploaded in the automatic order and in Morton
   order: intersect and occluded against the CPU oracle's brute force by adversarial_common.compare (t
   bit-equal, occluded equal).  tree_info must tell the two uploads apart, and its depth is the device's.
2. Fewer visits: default + emitter at 480 x 270 x 16 spp, depth 6, with SPTR_FRAME_COUNT_VISITS: the SAH order
   is in use, node visits + primitive tests of the closest-hit walks and of the shadow walks are each lower
   than in Morton order (no margin beyond "lower": the CPU model of the walk put the swept SAH trees 25-40 %
   lower), and the two images agree within test_gpu_golden.py's allowance (they may differ where two
   primitives tie exactly).
3. Refit: a dynamic upload in SAH order, moved with update_geometry and moved back, gives the fresh build's
   hits bit for bit; and moved, the hits of a fresh build of the moved scene up to ties.

Each context is the module's own and is closed before the next."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library, as tests/conftest.py's renderer fixture does)

import adversarial_common as A
import refit_common as R
import sptr

pytestmark = pytest.mark.gpu

SAH, MORTON = 0, 1


def _case(fam, name):
    for k, c in enumerate(A.family(fam)):
        if c.name == name:
            return k, c
    raise KeyError(name)


def _cases():
    t, _ = A.staging_counts()
    return [("tiny", "tiny_mix2"), ("tiny", "tiny_mix9"), ("equal", "equal_flat3"), ("scale", "scale_0"),
            ("staging", f"staging_{t}")]


def _flat(sc):
    return sptr.FlatScene(sc["positions"], sc["indices"], sc["tri_geom_first"], sc["spheres"], sc["geom_material"])


@pytest.fixture(scope="module", autouse=True)
def _session_context_first(renderer):
    """(The session's context exists before this module's own, as before every other module's.)"""
    yield


@pytest.mark.parametrize("fam,name", _cases(), ids=[n for _, n in _cases()])
def test_hits_in_both_orders(fam, name):
    k, case = _case(fam, name)
    ref_hits, ref_occ = A.reference(fam, k)
    n = case.num_tris + case.num_spheres
    infos = {}
    for order in (SAH, MORTON):
        r = sptr.Renderer(0)
        try:
            r.set_tree_order(order)
            r.upload_scene(_flat(case.scene))
            lay, info = r.scene_layout(), r.tree_info()
            infos[order] = info
            print(f"{name} order {order}: {info}, layout depth {lay['bvh_depth']} leaf {lay['leaf_size']} lds {lay['lds_bytes']}")
            assert lay["lds_bytes"] > 0 and lay["bvh_width"] == 2 and lay["leaf_size"] == 8, lay
            assert lay["node_bytes"] == (n - 1) * 64
            if order == MORTON:
                assert info["order"] == 1 and info["fallback"] == 1
            else:
                assert info["fallback"] != 1 and info["order"] == (0 if info["fallback"] == 0 else 1)
                assert info["depth"] == lay["bvh_depth"] == r.scene_info()["depth"], (info, lay)
                assert info["cost_morton"] > 0.0
                if info["order"] == 0:
                    assert info["cost_sah"] < info["cost_morton"]
            A.compare(case, r.intersect(case.rays), r.occluded(case.rays), ref_hits, ref_occ, f"{name} order {order}")
        finally:
            r.close()
    if name == "scale_0":  # default + emitter: the SAH order applies
        assert infos[SAH]["order"] == 0 and infos[SAH]["fallback"] == 0, infos[SAH]


def test_fewer_visits_same_image():
    W, H, spp = 480, 270, 16
    cam = sptr.camera_lookat(pos=(0.0, 3.0, 8.0), target=(0.0, 1.0, 0.0), aspect=W / H)
    got = {}
    for order in (SAH, MORTON):
        r = sptr.Renderer(0)
        try:
            r.set_tree_order(order)
            sptr.setup_default(r, "default_emitter")
            info = r.tree_info()
            assert info["order"] == order, info
            st = r.render(cam, W, H, spp=spp, max_depth=6, flags=sptr.SPTR_FRAME_COUNT_VISITS)
            got[order] = (st.node_visits + st.tri_tests + st.sphere_tests, st.shadow_node_visits + st.shadow_prim_tests,
                          r.read_accum().copy(), r.read_rgb8().copy(), (st.rays_closest, st.rays_shadow))
            print(f"order {order}: {info}; closest-hit walks: nodes {st.node_visits} tri {st.tri_tests} sphere {st.sphere_tests}; "
                  f"shadow walks: nodes {st.shadow_node_visits} prims {st.shadow_prim_tests}; rays {got[order][4]}; "
                  f"per traced camera ray: nodes {st.node_visits_primary / st.traced_primary:.4f} "
                  f"prims {(st.tri_tests_primary + st.sphere_tests_primary) / st.traced_primary:.4f}")
        finally:
            r.close()
    s, m = got[SAH], got[MORTON]
    assert s[0] < m[0], (s[0], m[0])
    assert s[1] < m[1], (s[1], m[1])
    # test_gpu_golden.py's _image_close against the oracle: exact-pixel fraction 0.999, relative L1 1e-3
    frac = float((s[3] == m[3]).all(axis=2).mean())
    fin = np.isfinite(s[2]) & np.isfinite(m[2])
    assert (np.isfinite(s[2]) != np.isfinite(m[2])).sum() <= max(3, 1e-6 * fin.size)
    rel = float(np.abs(s[2][fin] - m[2][fin]).sum() / max(1e-12, np.abs(m[2][fin]).sum()))
    print(f"images: exact-pixel fraction {frac}, relative L1 {rel:.3e}, bit-equal accumulation "
          f"{np.array_equal(s[2].view(np.uint32), m[2].view(np.uint32))}")
    assert frac >= 0.999 and rel <= 1e-3, (frac, rel)


def test_refit_there_and_back():
    base = sptr.builtin_scene("default_emitter")
    rays = R.rays(sptr.camera_lookat(aspect=R.W / R.H).as_array())
    mp, ms = R.deform(base.positions, base.spheres, 2)
    moved = sptr.FlatScene(mp, base.indices, base.tri_geom_first, ms, base.geom_material)
    ctx = []
    try:
        fresh = sptr.Renderer(0)
        ctx.append(fresh)
        fresh.upload_scene(base)
        info_base = fresh.tree_info()
        assert info_base["order"] == 0
        ref = fresh.intersect(rays), fresh.occluded(rays)
        fresh.upload_scene(moved)
        ref_moved = fresh.intersect(rays), fresh.occluded(rays)
        dyn = sptr.Renderer(0)
        ctx.append(dyn)
        dyn.set_dynamic(True)
        dyn.upload_scene(base)
        assert dyn.tree_info() == info_base  # dynamic and ordinary uploads build the same tree
        dyn.update_geometry(mp, ms)
        R.compare_hits(dyn.intersect(rays), ref_moved[0], "moved: refit vs fresh build")
        R.compare_occluded(dyn.occluded(rays), ref_moved[1], "moved: refit vs fresh build")
        assert not np.array_equal(dyn.intersect(rays)[2].view(np.uint32), ref[0][2].view(np.uint32))
        dyn.update_geometry(base.positions, base.spheres)
        assert dyn.refit_info()["refits"] == 2
        got = dyn.intersect(rays), dyn.occluded(rays)
        for a, b in zip(got[0], ref[0]):
            assert a.tobytes() == b.tobytes()
        assert got[1].tobytes() == ref[1].tobytes()
    finally:
        for r in ctx:
            r.close()
