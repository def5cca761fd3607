"""CPU pins of tests/adversarial_common.py's fixtures (no GPU): the generators are deterministic, every
scene has the property its family is named for, the rays produce hits and misses, and the CPU oracle's brute
force and its own BVH agree by the module's comparison rule with no ray excused — so that
tests/test_gpu_adversarial.py cannot pass vacuously."""
import numpy as np
import pytest

import adversarial_common as A
import oracle

MISS = A.MISS
f32 = np.float32


def _ref(fam, k):
    return A.reference(fam, k)


@pytest.mark.parametrize("fam", A.FAMILIES)
def test_generators_are_deterministic(fam):
    a = A.family(fam)
    b = A._BUILDERS[fam]()
    assert len(a) == len(b) > 0 and len({c.name for c in a}) == len(a)
    for x, y in zip(a, b):
        assert x.name == y.name and x.rays.tobytes() == y.rays.tobytes() and x.rays.dtype == np.float32
        assert not x.rays.flags.writeable and np.isfinite(x.rays[:, :7]).all() and not np.isnan(x.rays[:, 7]).any()
        for k in x.scene:
            assert x.scene[k].tobytes() == y.scene[k].tobytes() and not x.scene[k].flags.writeable, (x.name, k)
        assert np.isfinite(x.scene["positions"]).all() and np.isfinite(x.scene["spheres"]).all()
        assert (x.scene["spheres"][:, 3] >= 0).all()
        assert len(x.rays) <= 21000 and x.num_tris + x.num_spheres <= 4000


@pytest.mark.parametrize("fam", A.FAMILIES)
def test_oracle_brute_force_equals_its_bvh(fam):
    """Prepared(bvh=False) against Prepared(bvh=True) under the rule, zero excused; and hits and misses."""
    hits = misses = 0
    for k, c in enumerate(A.family(fam)):
        rh, ro = _ref(fam, k)
        P = oracle.Prepared(c.scene, bvh=True)
        assert A.compare(c, P.intersect(c.rays), P.occluded(c.rays), rh, ro, f"{c.name} oracle BVH vs brute force") == 0
        hits += int((rh[0] != MISS).sum())
        misses += int((rh[0] == MISS).sum())
        # occluded is the existence of what intersect minimises, except at a sphere hit with t <= 0 < tfar
        assert ((rh[0] != MISS) <= (ro != 0)).all()
    print(fam, "hits", hits, "misses", misses)
    assert hits >= 100 and misses >= 100


def test_tiny_counts():
    cases = A.family("tiny")
    assert len(cases) == 3 * len(A.COUNTS)
    for c in cases:
        n = int(c.name.lstrip("tiny_trsphmix"))
        assert c.num_tris + c.num_spheres == n
        if "_sph" in c.name:
            assert len(c.scene["positions"]) == 0 and len(c.scene["tri_geom_first"]) == 1
        if n == 0:
            rh, ro = _ref("tiny", cases.index(c))
            assert (rh[0] == MISS).all() and np.isinf(rh[2]).all() and not ro.any()
        elif n >= 2:
            rh, _ = _ref("tiny", cases.index(c))
            assert (rh[0] != MISS).sum() >= 50 and (rh[0] == MISS).sum() >= 50


def test_equal_keys_and_zero_extents():
    by = {c.name: c for c in A.family("equal")}
    for k in A.TIE_KS:
        for kind in ("tris", "spheres", "concentric"):
            keys = A.morton_keys(by[f"equal_{kind}{k}"].scene)
            assert len(keys) == k and (keys == keys[0]).all()
            ext = np.ptp(A.box_centres(by[f"equal_{kind}{k}"].scene), axis=0)
            assert (ext == 0).all()
    for name, zero_axes in (("equal_flat1", [2]), ("equal_flat2", [1, 2]), ("equal_flat3", [0, 1, 2])):
        ext = np.ptp(A.box_centres(by[name].scene), axis=0)
        assert [a for a in range(3) if ext[a] == 0] == zero_axes, (name, ext)
    keys = A.morton_keys(by["equal_flat3"].scene)
    assert len(keys) == 40 and (keys == keys[0]).all()
    keys = A.morton_keys(by["equal_flat1"].scene)
    assert len(np.unique(keys)) < len(keys)  # the two triangles of a cell share a box


def test_degenerate_counts():
    for c in A.family("degenerate"):
        ng = A.stored_normals(c.scene)
        zero = int((ng == 0).all(axis=1).sum())
        print(c.name, "stored normals exactly zero:", zero, "constructed:", c.ndeg)
        assert zero == c.ndeg if c.ndeg is not None else 7 <= zero <= 10
        assert c.all_deg == (zero == c.num_tris + c.num_spheres)
    c = A.family("degenerate")[2]
    rh, ro = _ref("degenerate", 2)
    assert (rh[0] == MISS).all() and not ro.any()
    for c in A.family("staging"):
        if c.ndeg:
            assert int((A.stored_normals(c.scene) == 0).all(axis=1).sum()) == c.ndeg == 8


def test_axis_rays():
    cases = A.family("axis")
    for c in cases:
        d = c.rays[:, 3:6]
        zeros = d == 0.0
        assert zeros.sum() > 200
        assert np.signbit(d[zeros]).all() == c.name.endswith("neg") and np.signbit(d[zeros]).any() == c.name.endswith("neg")
    k = [c.name for c in cases].index("axis_grid_pos")
    rh, _ = _ref("axis", k)
    n = cases[k].meta["lattice"]
    assert n == 2 * 169 and (rh[0][:n] != MISS).all()  # every lattice ray, down and up, hits the grid
    assert (rh[2][:169] == 3.0).all() and (rh[2][169:n] == 2.0).all()
    assert (rh[0][n:n + 26] == MISS).all()  # in the plane, and parallel above it
    assert [c.name for c in cases] == ["axis_grid_pos", "axis_box_pos", "axis_grid_neg", "axis_box_neg"]
    for pos, neg in ((0, 2), (1, 3)):
        a, b = _ref("axis", pos), _ref("axis", neg)
        assert a[0][2].tobytes() == b[0][2].tobytes() and a[1].tobytes() == b[1].tobytes()  # the sign of a zero changes nothing


def test_oracle_is_scale_invariant():
    cases = A.family("scale")
    (g0, p0, t0, n0), o0 = _ref("scale", 0)
    assert cases[0].meta["k"] == 0 and (g0 != MISS).sum() > 5000
    for k, c in enumerate(cases[1:], start=1):
        (g, p, t, _), o = _ref("scale", k)
        f = f32(2.0) ** f32(c.meta["k"])
        assert (g == g0).all() and (p == p0).all() and (o == o0).all()
        assert (t / f).astype(f32).tobytes() == t0.tobytes()


def test_offset_scenes_keep_hits():
    for k, c in enumerate(A.family("offset")):
        rh, _ = _ref("offset", k)
        assert (rh[0] != MISS).sum() > 5000 and (rh[0] == MISS).sum() > 1000
        assert np.abs(c.scene["positions"]).min() >= 2.0 ** int(c.name.split("_")[1]) - 16


def test_deep_tree_structure():
    c = A.family("deep")[0]
    keys = A.morton_keys(c.scene)
    ncl, ring = c.meta["clusters"], A.DEEP_CLUSTER
    assert c.num_tris == 2 + ncl * ring and ncl == 63
    ck = keys[2:].reshape(ncl, ring)
    for j in range(ncl):  # every more significant bit 0, bit j (from the top, bit 62) 1: the chain
        assert (ck[j] >> np.uint64(62 - j) == 1).all(), j
    assert keys[0] == 0 and keys[1] == (1 << 63) - 1
    (g, p, t, _), occ = _ref("deep", 0)
    assert g[0] == MISS and not occ[0]  # the axis touches no triangle
    n = c.meta["levels"]
    assert n == 3 * ncl
    for part in (slice(1, 1 + n), slice(1 + n, 1 + 2 * n)):
        assert (g[part] == 0).all() and ((p[part].astype(int) - 2) // ring == np.repeat(np.arange(ncl), 3)).all()
        assert ((p[part].astype(int) - 2) % ring < A.DEEP_RING).all()  # a ring triangle, not the spar
    # ... and nothing else: without cluster j its rays hit nothing
    idx = c.scene["indices"]
    for j in range(ncl):
        keep = np.ones(len(idx), bool)
        keep[2 + j * ring:2 + (j + 1) * ring] = False
        sc = A.make_scene(c.scene["positions"], idx[keep], np.zeros((0, 4)))
        rr = np.concatenate([c.rays[1 + 3 * j:4 + 3 * j], c.rays[1 + n + 3 * j:4 + n + 3 * j]])
        assert (oracle.Prepared(sc, bvh=False).intersect(rr)[0] == MISS).all(), j
    # the spars' boxes are nested, and each contains every smaller cluster
    tri = c.scene["positions"][c.scene["indices"].astype(np.int64)][2:].reshape(ncl, ring, 3, 3)
    for j in range(ncl - 1):
        lo, hi = tri[j, -1].min(axis=0), tri[j, -1].max(axis=0)
        assert (lo < tri[j + 1:].min(axis=(0, 1, 2))).all() and (tri[j + 1:].max(axis=(0, 1, 2)) < hi).all(), j
    # the axis passes through every cluster's box
    w = A.DEEP_W
    for j in range(ncl):
        b, a = divmod(j, 3)
        x = A.DEEP_S[a] * 2.0 ** -b * w
        v = c.scene["positions"][6 + 3 * ring * j:6 + 3 * ring * (j + 1)]
        assert (v.min(axis=0) < x).all() and (x < v.max(axis=0)).all()


def test_staging_counts_straddle_the_threshold():
    lim = A.header_constant("kLdsSceneBytes")
    assert lim == 48 * 1024
    t, d = A.staging_counts()
    cases = A.family("staging")
    assert [c.num_tris for c in cases] == [t - 1, t, t + 1, d + 7, d + 8, d + 9]
    assert A.staged_bytes(t, t, 0, t) <= lim < A.staged_bytes(t + 1, t + 1, 0, t + 1)
    for c in cases[3:]:
        n = c.num_tris - 8
        assert A.staged_bytes(n + 8, n + 8, 0, n + 8) > lim  # over NP: not small
    assert A.staged_bytes(d, d + 8, 0, d) <= lim < A.staged_bytes(d + 1, d + 9, 0, d + 1)  # over N: flips at d


def test_interval_ends():
    c = A.family("interval")[0]
    (g, p, t, _), occ = _ref("interval", 0)
    sp, t0 = c.meta["spans"], c.meta["t0"]
    assert len(t0) == 300 and (t0 > 0).all()
    assert (t[sp["tfar+"]] == t0).all() and (t[sp["tnear+"]] != t0).all()
    # (at the ends themselves the products aden * tfar round: they are pinned on the exact rays below)
    for tag in ("tfar<tnear", "tfar=0", "d=0"):
        assert (g[sp[tag]] == MISS).all() and np.isinf(t[sp[tag]]).all() and not occ[sp[tag]].any(), tag
    for k in (-10, 10):
        s = t[sp[f"d*2^{k}"]] * f32(2.0) ** f32(k)
        assert np.abs(s / t0 - 1).max() < 1e-5
    h = c.meta["exact_h"]
    assert len(h) >= 50
    assert (t[sp["exact tfar="]] == h).all() and occ[sp["exact tfar="]].all()      # tfar == t: accepted
    assert (g[sp["exact tfar-"]] == MISS).all() and not occ[sp["exact tfar-"]].any()  # just short: a miss
    assert (t[sp["exact tnear-"]] == h).all()                                      # tnear just below t: accepted
    assert (t[sp["exact tnear="]] != h).all()                                      # tnear == t: rejected


def test_indexing_scene():
    c = A.family("indexing")[0]
    first = c.scene["tri_geom_first"]
    assert list(first) == [0, 5, 5, 12, 12] and c.num_spheres == 3
    used = np.unique(c.scene["indices"])
    assert len(used) == 36 and len(c.scene["positions"]) == 54
    assert len(set(c.scene["geom_material"].tolist())) == 7
    (g, p, _, _), _ = _ref("indexing", 0)
    seen = set(g[g != MISS].tolist())
    assert seen == {0, 2, 4, 5, 6}  # never an empty geometry; the spheres follow the four triangle geometries
    assert p[g == 0].max() == 4 and p[g == 2].max() == 6 and (p[(g >= 4) & (g != MISS)] == 0).all()


def test_sphere_rays():
    c = A.family("spheres")[0]
    assert (c.scene["spheres"][:, 3] == 0).sum() == 1
    for k in (1, 2):  # the points: every parallel ray hits exactly, at the nearest centre on its line
        pc = A.family("spheres")[k]
        (pg, _, pt, _), po = _ref("spheres", k)
        n = 2 * pc.meta["parallel"]
        assert (pc.scene["spheres"][:, 3] == 0).all() and (pg[:n] != MISS).all() and po[:n].all()
        assert set(pt[:n].tolist()) <= {1.0, 2.0, 3.0} and (pt[:n] == 3.0).sum() >= n // 3
    (g, _, t, _), _ = _ref("spheres", 0)
    per = 8 + 8 + 8 + 3 + 8  # rays per sphere: inside, on the surface outwards / inwards, tangents
    inside = np.concatenate([np.arange(8) + per * s for s in range(8)])
    assert (g[inside] != MISS).all() and (t[inside] > 0).all()  # from inside a sphere its far root is hit
    tangent = np.concatenate([np.arange(24, per) + per * s for s in range(8)])
    print("tangent rays that hit:", int((g[tangent] != MISS).sum()), "of", len(tangent))
    assert 0 < (g[tangent] != MISS).sum() < len(tangent)
