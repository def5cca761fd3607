"""GPU tests of the BVH build (build_lbvh) and of the traversals (bvh2_walk, the wide walks) on adversarial
geometry, against an independent yardstick: the CPU oracle's brute force, oracle.Prepared(scene, bvh=False).

Families, rays and the comparison rule are tests/adversarial_common.py's (pinned on the CPU by
tests/test_adversarial_cpu.py): t bit-equal and occluded equal for every ray, zero mismatches expected, at
most 1e-4 of a case's rays excused when float64 shows the hit marginal; a ray naming another primitive must
name one really hit at the bit-equal t; Ng bit-equal and the barycentrics within query_common's bound where
the ids agree.

One test is one family under one build configuration; every case of the family goes through intersect,
occluded and query_rays (closest-hit and any-hit, unsorted and sorted, from device tensors).  scene_layout()
and refit_info() must show that the configuration took effect (width, leaf size, lds_bytes, num_prim_refs,
excluded_prims).  The dynamic configuration uploads refit_common.deform(..., 1)'s coordinates (_deformed) and moves them
to the real ones with update_geometry, so the boxes under test are the refitted ones (and the tree's shape is
that of the deformed scene).  The split-reference configuration
runs the scenes above the LDS-staging threshold only (split references are never made below it).

One context per configuration, one at a time."""
import time

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import adversarial_common as A
import query_common as Q
import refit_common as R
import sptr

pytestmark = pytest.mark.gpu
MISS = A.MISS
f32 = np.float32

CONFIGS = {
    "defaults": dict(),
    "w2_leaf1": dict(width=2, leaf=1),
    "w2_leaf16": dict(width=2, leaf=16),
    "w4_leaf1": dict(width=4, leaf=1),
    "w4_leaf4": dict(width=4, leaf=4),
    "w4_dynamic": dict(width=4, dynamic=True),
    "split8": dict(split=8),
}
PAIRS = [(c, f) for c in CONFIGS for f in A.FAMILIES if c != "split8" or f == "staging"]
_contexts = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts(renderer):
    """(The session's context exists before this module's, as it does before every other module's own
    contexts: its streams are the process's first.)"""
    yield
    for r in _contexts.values():
        r.close()
    _contexts.clear()


def _context(name):
    """The configuration's context; one at a time (the tests come grouped by configuration), so that the
    module never holds more streams than the other modules that make contexts of their own."""
    if name not in _contexts:
        for r in _contexts.values():
            r.close()
        _contexts.clear()
        cfg = CONFIGS[name]
        r = sptr.Renderer(0)
        r.set_bvh_width(cfg.get("width", 0))
        r.set_leaf_size(cfg.get("leaf", 0))
        r.set_dynamic(cfg.get("dynamic", False))
        r.set_split_refs(cfg.get("split", 0))
        _contexts[name] = r
    return _contexts[name]


def _deformed(sc):
    """refit_common.deform(..., 1) in the scene's own frame: the coordinates are brought to default_emitter's
    place and size (box centre -> (0, 1, 2), half diagonal -> at most 3, by a power of two), deformed and
    brought back, so that the map stays injective in float32 for scenes of any scale and offset (a triangle
    that is degenerate at upload stays out of the tree for good, include/sptr_hip.h)."""
    c, rad, _, _ = A.bounds(sc)
    u = 2.0 ** np.ceil(np.log2(rad / 3.0))
    at = np.array([0.0, 1.0, 2.0])
    q = (sc["positions"].astype(np.float64) - c) / u + at
    sp = sc["spheres"].astype(np.float64)
    sp = np.concatenate([(sp[:, :3] - c) / u + at, sp[:, 3:] / u], axis=1)
    q, sp = R.deform(q, sp, 1)
    q = ((q.astype(np.float64) - at) * u + c).astype(f32)
    sp = np.concatenate([(sp[:, :3].astype(np.float64) - at) * u + c, sp[:, 3:].astype(np.float64) * u], axis=1).astype(f32)
    if len(sc["indices"]):
        flat = lambda p: (A.stored_normals(A.transformed(sc, positions=p)) == 0).all(axis=1)
        if (flat(q) != flat(sc["positions"])).any():
            # float32 cannot hold the deformed scene (the deep tree's clusters near the origin collapse once
            # moved away from it): scale the axes by 2, 1/2 and 1 instead, which is exact
            print("  (uploaded with the axes scaled by 2, 1/2, 1: refit_common.deform's image does not fit float32)")
            f = np.array([2.0, 0.5, 1.0], f32)
            sp = sc["spheres"] * np.array([2.0, 0.5, 1.0, 2.0], f32)
            return sc["positions"] * f, sp
    return q, sp


def _upload(r, cfg, case):
    sc = case.scene
    flat = sptr.FlatScene(sc["positions"], sc["indices"], sc["tri_geom_first"], sc["spheres"], sc["geom_material"])
    if not cfg.get("dynamic"):
        r.upload_scene(flat)
        return
    p, s = _deformed(sc)
    r.upload_scene(sptr.FlatScene(p, sc["indices"], sc["tri_geom_first"], s, sc["geom_material"]))
    if case.num_tris + case.num_spheres:
        r.update_geometry(sc["positions"] if len(sc["positions"]) else None, sc["spheres"] if len(sc["spheres"]) else None)
        assert r.refit_info()["refits"] == 1


def _check_layout(r, name, cfg, case):
    """The configuration took effect, by the formulas of build_lbvh and scene_view."""
    lim, stack = A.header_constant("kLdsSceneBytes"), A.header_constant("kStack")
    lay, info = r.scene_layout(), r.refit_info()
    T, S = case.num_tris, case.num_spheres
    assert lay["num_tris"] == T and lay["num_spheres"] == S
    refs = lay["num_prim_refs"]
    if T + S == 0:
        assert refs == 0
        return lay
    ex = info["excluded_prims"]
    if not case.all_deg and case.ndeg is not None:
        assert ex == case.ndeg, (case.name, ex)
    if "split" in cfg:
        assert refs >= T + S
    else:
        assert refs == T + S
    n = refs - ex
    tri_refs = refs - S
    auto = 8 if A.staged_bytes(n, tri_refs, S, n) <= lim else 1
    assert lay["leaf_size"] == cfg.get("leaf", auto), (case.name, lay)
    want_w = cfg.get("width") or (2 if A.staged_bytes(n, tri_refs, S, refs) <= lim else 4)
    if lay["bvh_width"] != want_w:
        # the only permitted departure: a wide stack bound beyond kStack (3 entries per wide level, and no
        # more wide levels than BVH2 levels) sends a BVH4 request to BVH2
        assert (want_w, lay["bvh_width"]) == (4, 2) and 3 * lay["bvh_depth"] > stack, (case.name, lay)
    if lay["bvh_width"] == 2:
        assert lay["node_bytes"] == max(n - 1, 0) * 64
    total = lay["node_bytes"] + tri_refs * 48 + S * 16 + (refs + 3) // 4 * 16
    assert lay["lds_bytes"] == (total if total <= lim else 0), (case.name, lay, total)
    assert lay["bvh_depth"] <= stack
    print(f"{name} {case.name}: layout {lay}, excluded {ex}")
    return lay


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _run_case(r, name, cfg, fam, k, case):
    _upload(r, cfg, case)
    lay = _check_layout(r, name, cfg, case)
    ref_hits, ref_occ = A.reference(fam, k)
    rays = case.rays
    what = f"{name} {case.name}"
    hits, occ = r.intersect(rays), r.occluded(rays)
    A.compare(case, hits, occ, ref_hits, ref_occ, what + " intersect / occluded")
    dev = torch.from_numpy(rays.copy()).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    got = {}
    for sort in (False, True):
        q = _np(r.query_rays(dev, sort=sort))
        o = _np(r.query_rays(dev, any_hit=True, sort=sort))["occluded"]
        assert r.query_info()["sorted"] == int(sort)
        A.compare(case, (q["geom"], q["prim"], q["t"], q["ng"]), o, ref_hits, ref_occ, what + f" query_rays sort={sort}")
        got[sort] = (q, o)
    for key in got[False][0]:
        assert got[False][0][key].tobytes() == got[True][0][key].tobytes(), (what, key)
    assert got[False][1].tobytes() == got[True][1].tobytes(), what
    q = got[False][0]
    assert q["geom"].tobytes() == hits[0].tobytes() and q["t"].tobytes() == hits[2].tobytes(), what
    # barycentrics, where the ids are the oracle's
    same = (q["geom"] == ref_hits[0]) & (q["prim"] == ref_hits[1])
    mask, tri = Q.triangle_hits(case.scene["tri_geom_first"], np.where(same, q["geom"], MISS), q["prim"])
    if mask.any():
        Q.check_barycentrics(q["uv"][mask, 0], q["uv"][mask, 1], case.scene["positions"], case.scene["indices"],
                             rays[mask], tri, what)
    assert not q["uv"][~Q.triangle_hits(case.scene["tri_geom_first"], q["geom"], q["prim"])[0]].any()
    return lay, hits


@pytest.mark.parametrize("name,fam", PAIRS, ids=[f"{c}-{f}" for c, f in PAIRS])
def test_family(name, fam):
    t0 = time.perf_counter()
    cfg = CONFIGS[name]
    r = _context(name)
    done = {}
    for k, case in enumerate(A.family(fam)):
        if "split" in cfg and not case.meta.get("above"):
            continue
        try:
            done[k] = _run_case(r, name, cfg, fam, k, case)
        except sptr.SptrError as e:
            if "rc=-2:" not in str(e):  # (SPTR_ERR_HIP; any other code is a refused argument: this test fails)
                raise
            # a failed HIP call leaves the device in doubt: nothing more runs on it
            pytest.exit(f"{name} {case.name}: {e}", returncode=3)
    assert done
    cases = A.family(fam)
    if fam == "tiny":
        # an empty upload: no root, every ray misses (compare has checked t = +inf and occluded = 0)
        for k, case in enumerate(cases):
            if case.num_tris + case.num_spheres == 0:
                assert (done[k][1][0] == MISS).all()
    if fam == "degenerate":
        assert (done[2][1][0] == MISS).all()  # a tree over degenerate triangles only: nothing to hit
    if fam == "scale":
        # metamorphic: the device's own results at 2^k against its unscaled ones
        g0, p0, t0_, _ = done[0][1]
        for k, case in enumerate(cases[1:], start=1):
            g, p, t, _ = done[k][1]
            assert (g == g0).all() and (p == p0).all(), case.name
            assert (t / f32(2.0) ** f32(case.meta["k"])).astype(f32).tobytes() == t0_.tobytes(), case.name
    if fam == "deep":
        # beyond the 12 LDS stack entries: hits of the deeper clusters come from spilled entries
        # (test_deep_tree_depth holds the stated bound where the tree is built from the scene itself)
        print(f"{name} deep: bvh_depth {done[0][0]['bvh_depth']}, width {done[0][0]['bvh_width']}")
        assert done[0][0]["bvh_depth"] > 12
        # the short chain keeps BVH4 where it is asked for or chosen, deep enough for the wide walks' stacks
        # (up to 3 entries per wide level) to spill as well
        short = done[1][0]
        print(f"{name} deep_short: bvh_depth {short['bvh_depth']}, width {short['bvh_width']}")
        assert short["bvh_depth"] > 12 and short["bvh_width"] == cfg.get("width", 4)
    if fam == "staging" and cfg.get("width") == 2:
        for k, case in enumerate(cases[:3]):  # as BVH2 the scene leaves LDS exactly above the derived count
            assert (done[k][0]["lds_bytes"] == 0) == case.meta["above"], case.name
    if fam == "staging" and name == "defaults":
        # ... where the automatic choice turns to single-primitive leaves and BVH4 (whose fewer nodes may fit again)
        for k, case in enumerate(cases[:3]):
            assert done[k][0]["bvh_width"] == (4 if case.meta["above"] else 2)
            assert done[k][0]["leaf_size"] == (1 if case.meta["above"] else 8)
        assert [done[k][0]["leaf_size"] for k in (3, 4, 5)] == [8, 8, 1]  # N decides the leaf size, NP the splitting
    if "split" in cfg:
        assert any(lay["num_prim_refs"] > lay["num_tris"] for lay, _ in done.values())
    print(f"{name}-{fam}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name", [c for c in CONFIGS if c != "split8"])
def test_deep_tree_depth(name):
    """The deep tree's bvh_depth is at least 30.  Measured on an MI355X: 68 under every configuration (63
    chain levels and the clusters' own).  The clusters' spars keep it there for single-primitive leaves too:
    without them the three SAH treelet passes regrouped the thin rings and left 25.  At that depth the BVH4
    stack bound (3 entries per wide level) exceeds kStack, so a BVH4 request is answered with BVH2, which
    _check_layout holds against the header's constant.  (w4_dynamic builds its tree from the axis-scaled upload,
    whose Morton keys, normalised per axis, are the scene's own.)"""
    cfg = CONFIGS[name]
    r = _context(name)
    case = A.family("deep")[0]
    _upload(r, cfg, case)
    lay = _check_layout(r, name, cfg, case)
    print(f"{name}: deep tree bvh_depth {lay['bvh_depth']} (scene_info {r.scene_info()['depth']}), width {lay['bvh_width']}")
    assert r.scene_info()["depth"] == lay["bvh_depth"]
    assert lay["bvh_depth"] >= 30
