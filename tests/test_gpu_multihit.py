"""GPU tests of multi-hit ray queries: sptr_query_multi_hit / sptr_multi_hit_info (k_rayquery_multi,
kernels_query.h; the list of csrc/hit_list.h) through Renderer.query_multi_hit / multi_hit_info and sptr_cli.

Scenes are tests/refit_common.py's: default_emitter (an LDS-staged BVH2 with leaf ranges; the glass cube and the
spheres give real multi-hit lists) and the 30x70 sphere mesh with set_bvh_width(4) (the quantised BVH4 walked from
L2).  Rays are tests/multihit_common.py's 20 492.  The yardstick is tests/multihit_ref.py: per primitive the
oracle's brute force on a scene of that one primitive, sorted by (t, geom, prim) and cut at K; no tree, no device.

Rule (_compare): count and every slot of geom, prim, t and Ng are bit-equal to the reference, filled tail
included; uv is within query_common.check_barycentrics' bound for triangle slots and exactly 0 for sphere slots
and the tail.  A ray may differ only if one of its first K + 1 reference candidates is marginal in float64
(tests/test_multihit_cpu.py counts them: none in the query scenes' rays), and at most refit_common.CAP of the rays
may.  The expected number is 0.

One context per scene serves the module; the tests that change a context's scene make their own."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import adversarial_common as A
import multihit_common as M
import multihit_ref as MR
import query_common as Q
import refit_common as R
import sptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MISS = 0xFFFFFFFF
INVALID, NO_SCENE = -1, -3
FIELDS = ("geom", "prim", "t", "ng", "uv")
COLS = {"count": 0, "geom": 1, "prim": 1, "t": 1, "ng": 3, "uv": 2}
NP_DTYPE = {"count": np.uint32, "geom": np.uint32, "prim": np.uint32, "t": np.float32, "ng": np.float32, "uv": np.float32}


def _flat(sc):
    return sptr.FlatScene(sc["positions"], sc["indices"], sc["tri_geom_first"], sc["spheres"], sc["geom_material"])


def _context(cfg, dynamic=False):
    name, p0, p1, width = cfg
    r = sptr.Renderer(0)
    r.set_bvh_width(width)
    r.set_dynamic(dynamic)
    flat = sptr.builtin_scene(name, p0, p1)
    r.upload_scene(flat)
    r.set_materials(sptr.preset_materials(with_light=(name == "default_emitter")))
    r.set_lights(sptr.default_lights())
    r.set_environment(None)
    lay = r.scene_layout()
    assert (lay["lds_bytes"] != 0) == (width == 0) and lay["bvh_width"] == (4 if width else 2)
    return r, flat


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module", params=R.SCENES, ids=R.SCENE_IDS)
def scene(request, renderer):
    """(config, context, oracle scene dict, rays, rays on the device, the reference lists)."""
    sc, rays, ref = M.scene_reference(request.param[0])
    r, flat = _context(request.param)
    assert np.array_equal(flat.positions, sc["positions"]) and np.array_equal(flat.spheres, sc["spheres"])
    yield request.param, r, sc, rays, _dev(rays), ref
    r.close()


@pytest.fixture(scope="module")
def mesh(renderer):
    r, flat = _context(R.SCENES[1])
    yield r, flat
    r.close()


def _np(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _differing(got, want):
    """Per ray: count or any slot of geom, prim, t, ng differs in bits from the reference."""
    d = got["count"] != want["count"]
    for k in ("geom", "prim", "t", "ng"):
        d |= (got[k].view(np.uint32) != want[k].view(np.uint32)).reshape(len(d), -1).any(axis=1)
    return d


def _compare(got, sc, rays, ref, K, what):
    """The module docstring's rule; returns the number of differing rays."""
    n = len(rays)
    want = MR.cut(ref, K)
    assert got["count"].shape == (n,) and got["t"].shape == (n, K) and got["ng"].shape == (n, K, 3)
    assert got["uv"].shape == (n, K, 2) and got["geom"].dtype == np.uint32 and got["count"].dtype == np.uint32
    diff = _differing(got, want)
    flagged = MR.marginal_rays(sc, rays, ref, K)
    print(f"{what}: {n} rays, {int(want['count'].sum())} reference hits (up to {int(want['count'].max(initial=0))} per ray); "
          f"{int(diff.sum())} rays differ, {int((diff & ~flagged).sum())} of them without a marginal candidate "
          f"({int(flagged.sum())} rays hold one)")
    for q in np.flatnonzero(diff & ~flagged)[:4]:
        print(f"  ray {q} {rays[q]}: count {got['count'][q]} vs {want['count'][q]}\n   t {got['t'][q]}\n   vs {want['t'][q]}\n"
              f"   ids {got['geom'][q]} {got['prim'][q]}\n   vs  {want['geom'][q]} {want['prim'][q]}")
    assert not (diff & ~flagged).any(), what
    assert diff.sum() <= R.CAP * n, what
    # barycentrics: triangle slots by the float64 bound, every other slot exactly zero
    ntg = len(sc["tri_geom_first"]) - 1
    ok = ~diff
    tri = (got["geom"] < ntg) & ok[:, None]
    if tri.any():
        ray, slot = np.nonzero(tri)
        idx = sc["tri_geom_first"].astype(np.int64)[got["geom"][ray, slot]] + got["prim"][ray, slot].astype(np.int64)
        Q.check_barycentrics(got["uv"][ray, slot, 0], got["uv"][ray, slot, 1], sc["positions"], sc["indices"], rays[ray], idx, what)
    rest = ~tri & ok[:, None]
    assert (got["uv"].view(np.uint32)[rest] == 0).all(), what
    return int(diff.sum())


@pytest.mark.parametrize("K", M.KS)
def test_equals_the_reference(scene, K):
    cfg, r, sc, rays, rays_dev, ref = scene
    for path, arg in (("host", rays), ("device", rays_dev)):
        got = r.query_multi_hit(arg, K)
        assert isinstance(got["t"], np.ndarray if path == "host" else torch.Tensor)
        assert set(got) == {"count", *FIELDS}
        assert _compare(_np(got), sc, rays, ref, K, f"{cfg[0]} K={K} ({path})") == 0
        info = r.multi_hit_info()
        assert info["list_capacity"] == (4 if K <= 4 else 8 if K <= 8 else 16)
        assert info["lds_bytes"] >= 12 * 1024 + 2048 * info["list_capacity"]
    if K == M.KS[-1]:
        print(cfg[0], "multi_hit_info", info)


def test_k1_against_the_existing_query(scene):
    cfg, r, sc, rays, rays_dev, ref = scene
    one = _np(r.query_multi_hit(rays_dev, 1))
    old = _np(r.query_rays(rays_dev))
    assert (one["t"][:, 0].view(np.uint32) == old["t"].view(np.uint32)).all()  # every ray, bit for bit
    assert ((one["count"] == 1) == (old["geom"] != MISS)).all()
    clear = ~MR.tie_at(ref, 0)
    assert clear.sum() > 0.9 * len(rays)
    assert (one["geom"][clear, 0] == old["geom"][clear]).all() and (one["prim"][clear, 0] == old["prim"][clear]).all()
    assert (one["ng"][clear, 0].view(np.uint32) == old["ng"][clear].view(np.uint32)).all()
    assert (one["uv"][clear, 0].view(np.uint32) == old["uv"][clear].view(np.uint32)).all()


def test_prefix_property(scene):
    """Pruning by the K-th distance loses nothing: K = 4 is the first 4 slots of K = 16."""
    cfg, r, sc, rays, rays_dev, ref = scene
    a, b = _np(r.query_multi_hit(rays_dev, 4)), _np(r.query_multi_hit(rays_dev, 16))
    assert (a["count"] == np.minimum(b["count"], 4)).all()
    for k in FIELDS:
        assert a[k].tobytes() == np.ascontiguousarray(b[k][:, :4]).tobytes(), k
    for K in (2, 8):  # (within one capacity, and the middle one)
        c = _np(r.query_multi_hit(rays_dev, K))
        for k in FIELDS:
            assert c[k].tobytes() == np.ascontiguousarray(b[k][:, :K]).tobytes(), (K, k)


@pytest.mark.parametrize("K", (3, 16))
def test_order_cannot_matter(scene, K):
    cfg, r, sc, rays, rays_dev, ref = scene
    n0, q0 = r.multi_hit_info()["queries"], r.query_info()["queries"]
    for path, arg in (("host", rays), ("device", rays_dev)):
        plain = _np(r.query_multi_hit(arg, K, sort=False))
        info = r.multi_hit_info()
        assert info["sorted"] == 0 and info["ms_sort"] == 0.0 and info["ms_trace"] > 0.0
        ordered = _np(r.query_multi_hit(arg, K, sort=True))
        info = r.multi_hit_info()
        print(cfg[0], path, K, info)
        assert info["sorted"] == 1 and info["ms_sort"] > 0.0 and info["ms_trace"] > 0.0
        _same_bytes(ordered, plain, f"{cfg[0]} {path} sorted vs unsorted")
    assert r.multi_hit_info()["queries"] == n0 + 4 and r.query_info()["queries"] == q0


# ------------------------------------------------------------------------------------- ties and duplicates
_adv = {}


def _adversarial_context(width, split):
    """One context at a time for the adversarial cases (they come grouped by configuration)."""
    if (width, split) not in _adv:
        for r in _adv.values():
            r.close()
        _adv.clear()
        r = sptr.Renderer(0)
        r.set_bvh_width(width)
        r.set_split_refs(split)
        _adv[(width, split)] = r
    return _adv[(width, split)]


@pytest.fixture(scope="module", autouse=True)
def _close_adversarial(renderer):
    yield
    for r in _adv.values():
        r.close()
    _adv.clear()


def _run_case(fam, k, width, split=0):
    case, ref = M.case_reference(fam, k)
    r = _adversarial_context(width, split)
    r.upload_scene(_flat(case.scene))
    got = _np(r.query_multi_hit(_dev(case.rays), 16))
    _compare(got, case.scene, case.rays, ref, 16, f"{case.name} width={width} split={split}")
    assert _np(r.query_multi_hit(case.rays, 3, sort=True))["t"].tobytes() == np.ascontiguousarray(got["t"][:, :3]).tobytes()
    return case, ref, got, r


@pytest.mark.parametrize("width", (0, 4))
@pytest.mark.parametrize("k", range(9))
def test_equal_keys(k, width):
    case, ref, got, _ = _run_case("equal", k, width)
    kk, kind = A.TIE_KS[k // 3], k % 3
    hit = got["count"] > 0
    assert hit.sum() > 100
    key = (got["geom"].astype(np.uint64) << np.uint64(32)) | got["prim"].astype(np.uint64)
    if kind == 0:  # coincident triangles: min(K, 16) hits at one t, ids ascending, no repeat
        assert (got["count"][hit] == min(kk, 16)).all()
        assert (got["t"][hit, :min(kk, 16)] == got["t"][hit, :1]).all()
        assert (got["prim"][hit, :min(kk, 16)] == np.arange(min(kk, 16))).all() and (got["geom"][hit, :min(kk, 16)] == 0).all()
    elif kind == 1:  # identical spheres: ties among the entries, then among the exits
        live = key[hit]
        assert ((live[:, 1:] > live[:, :-1]) | (got["t"][hit, 1:] > got["t"][hit, :-1]) | (got["geom"][hit, 1:] == MISS)).all()
    else:  # concentric spheres seen from outside (the grid rays): entries from the outermost inwards, then exits
        full = got["count"] == min(2 * kk, 16)
        full[4096:] = False
        assert full.sum() > 100
        prim, geom = got["prim"][full], got["geom"][full]
        assert (prim[:, 1:] >= prim[:, :-1]).all() and (prim[:, 0] == 0).all() and (geom[:, 0] == kk - 1).all()
        entry = prim == 0
        assert (geom[entry] == (kk - 1 - np.arange(geom.shape[1]))[None, :].repeat(len(geom), 0)[entry]).all()
        if kk == 2:
            assert (prim == [0, 0, 1, 1] + [MISS] * 12).all() and (geom == [1, 0, 0, 1] + [MISS] * 12).all()


@pytest.mark.parametrize("width", (0, 4))
@pytest.mark.parametrize("fam,k", [c for c in M.ADVERSARIAL if c[0] in ("spheres", "interval", "tiny")],
                         ids=lambda v: str(v))
def test_spheres_intervals_and_tiny_trees(fam, k, width):
    case, ref, got, _ = _run_case(fam, k, width)
    if case.name == "spheres":  # origins inside: one hit, the exit reported as the first (prim 0)
        for own in range(8):  # (35 rays per sphere, the first 8 from 0.3 r off its centre)
            for q in range(own * 35, own * 35 + 8):
                g = list(got["geom"][q, :got["count"][q]])
                assert g.count(own) == 1 and got["prim"][q, g.index(own)] == 0, (own, q)


def test_split_references_give_one_hit_per_triangle():
    case, ref, got, r = _run_case("staging", 2, 4, split=8)
    lay = r.scene_layout()
    print("staging with split references:", lay["num_prim_refs"], "references for", case.num_tris, "triangles")
    assert lay["num_prim_refs"] > case.num_tris and lay["bvh_width"] == 4
    key = np.where(got["geom"] != MISS, (got["geom"].astype(np.uint64) << np.uint64(32)) | got["prim"].astype(np.uint64),
                   np.arange(16, dtype=np.uint64)[None, :] + (np.uint64(MISS) << np.uint64(32)))
    srt = np.sort(key, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()  # no triangle twice in any list


# ------------------------------------------------------------------------------------- shapes
SHAPE_NS = (0, 1, 63, 64, 65, 257)
BIG = 600001  # more rays than any resident grid has threads


@pytest.fixture(scope="module")
def shape_rays(mesh):
    """600 001 rays from default_rng(11) over refit_common.rays' boxes, and one K = 3 result for all of them."""
    rng = np.random.default_rng(11)
    o = rng.uniform([-6.0, 0.0, -6.0], [6.0, 5.0, 8.0], (BIG, 3))
    tg = rng.uniform([-3.0, 0.0, -3.0], [3.0, 3.0, 5.0], (BIG, 3))
    d = tg - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rr = np.zeros((BIG, 8), np.float32)
    rr[:, 0:3] = o
    rr[:, 3:6] = d
    rr[:, 7] = np.inf
    rr.setflags(write=False)
    dev = _dev(rr)
    big = _np(mesh[0].query_multi_hit(dev, 3, sort=False))
    assert (big["count"] == 3).sum() > 10000
    return rr, dev, big


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
@pytest.mark.parametrize("n", SHAPE_NS)
def test_shapes_where_indexing_can_break(mesh, shape_rays, n, sort):
    r = mesh[0]
    rr, dev, big = shape_rays
    want = {k: v[:n] for k, v in big.items()}  # (a ray's result does not depend on its batch)
    for path, arg in (("host", rr[:n]), ("device", dev[:n])):
        got = _np(r.query_multi_hit(arg, 3, sort=sort))
        assert got["count"].shape == (n,) and got["ng"].shape == (n, 3, 3)
        _same_bytes(got, want, f"n={n} {path} sort={sort}")
        if n:
            assert r.multi_hit_info()["sorted"] == int(sort)


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
def test_more_rays_than_a_resident_grid(mesh, shape_rays, sort):
    r = mesh[0]
    rr, dev, big = shape_rays
    two = _np(r.query_multi_hit(dev, 2, sort=sort))
    assert (two["count"] == np.minimum(big["count"], 2)).all()
    for k in FIELDS:
        assert two[k].tobytes() == np.ascontiguousarray(big[k][:, :2]).tobytes(), k
    # and against the closest-hit query, whose walk is another
    old = _np(r.query_rays(dev, sort=sort, fields=("t",)))
    assert (two["t"][:, 0].view(np.uint32) == old["t"].view(np.uint32)).all()


# ------------------------------------------------------------------------------------- NULL outputs
GUARD = 64  # elements on either side of an output


def _guarded(names, n, K):
    views, whole = {}, {}
    for k in names:
        shape = (n,) if k == "count" else (n, K) if COLS[k] == 1 else (n, K, COLS[k])
        m = int(np.prod(shape))
        big = torch.from_numpy(np.full(m + 2 * GUARD, 123456789, NP_DTYPE[k])).to("cuda:0")
        whole[k] = big
        views[k] = big[GUARD:GUARD + m].view(shape)
    torch.cuda.synchronize()
    return views, whole


def _guards_intact(whole):
    for k, big in whole.items():
        a = big.cpu().numpy()
        sentinel = a.dtype.type(123456789)
        assert (a[:GUARD] == sentinel).all() and (a[-GUARD:] == sentinel).all(), k


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
def test_null_outputs_and_guard_pages(scene, sort):
    cfg, r, sc, rays, rays_dev, ref = scene
    n, K = len(rays), 5
    views, whole = _guarded(("count",) + FIELDS, n, K)
    full = r.query_multi_hit(rays_dev, K, sort=sort, out=views)
    assert all(full[k].data_ptr() == views[k].data_ptr() for k in full)
    _guards_intact(whole)
    full = _np(full)
    _same_bytes(full, _np(r.query_multi_hit(rays_dev, K, sort=sort)), f"{cfg[0]} caller-allocated vs library-allocated")
    subsets = [c for m in range(len(FIELDS)) for c in itertools.combinations(FIELDS, m)]  # every proper subset
    assert len(subsets) == 31
    for names in subsets:
        views, whole = _guarded(("count",) + names, n, K)
        part = r.query_multi_hit(rays_dev, K, sort=sort, fields=names, out=views)
        assert set(part) == {"count", *names}
        _guards_intact(whole)
        _same_bytes(_np(part), {k: full[k] for k in ("count",) + names}, f"{cfg[0]} only {names}")
    for names in (("t",), ("geom", "uv"), ()):
        _same_bytes(r.query_multi_hit(rays, K, sort=sort, fields=names), {k: full[k] for k in ("count",) + names},
                    f"{cfg[0]} only {names}, host path")


@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_after_a_refit(cfg, renderer):
    _, rays, _ = M.scene_reference(cfg[0])
    rays_dev = _dev(rays)
    r, flat = _context(cfg, dynamic=True)
    before = _np(r.query_multi_hit(rays_dev, 4))
    pos, sph = R.deform(flat.positions, flat.spheres, 1)
    r.update_geometry(pos, sph)
    assert r.refit_info()["refits"] == 1
    fresh = sptr.Renderer(0)
    fresh.set_bvh_width(cfg[3])
    fresh.upload_scene(sptr.FlatScene(pos, flat.indices, flat.tri_geom_first, sph, flat.geom_material))
    for K in (4, 16):
        for sort in (False, True):
            _same_bytes(_np(r.query_multi_hit(rays_dev, K, sort=sort)), _np(fresh.query_multi_hit(rays_dev, K)),
                        f"{cfg[0]} refitted vs fresh, K={K} sort={sort}")
    after = _np(r.query_multi_hit(rays_dev, 4))
    assert (after["t"].view(np.uint32) != before["t"].view(np.uint32)).any(axis=1).mean() >= 0.2  # (the deformation matters)
    fresh.close()
    r.close()


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
def test_async_on_a_torch_stream(scene, sort):
    cfg, r, sc, rays, rays_dev, ref = scene
    want4, want16 = _np(r.query_multi_hit(rays_dev, 4, sort=sort)), _np(r.query_multi_hit(rays_dev, 16, sort=sort))
    want_old = _np(r.query_rays(rays_dev, sort=sort))
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(stream):
        got4 = r.query_multi_hit(rays_dev, 4, sort=sort, stream=stream.cuda_stream)
        old = r.query_rays(rays_dev, sort=sort, stream=stream.cuda_stream)  # (same stream: shared scratch)
        got16 = r.query_multi_hit(rays_dev, 16, sort=sort, stream=stream.cuda_stream)
    stream.synchronize()
    _same_bytes(_np(got4), want4, f"{cfg[0]} enqueued vs synchronous, K=4")
    _same_bytes(_np(got16), want16, f"{cfg[0]} enqueued vs synchronous, K=16")
    _same_bytes(_np(old), want_old, f"{cfg[0]} enqueued closest-hit between them")
    info = r.multi_hit_info()
    assert info["sorted"] == int(sort) and info["ms_trace"] > 0.0 and info["list_capacity"] == 16


# ------------------------------------------------------------------------------------- errors
def _raw(r, rays=None, n=0, flags=0, max_hits=1, pad=0, reserved=(0, 0, 0, 0), stream=None, **outs):
    q = sptr.MultiHitQuery()
    q.rays, q.n, q.flags, q.max_hits, q.pad = rays, n, flags, max_hits, pad
    for i, v in enumerate(reserved):
        q.reserved[i] = v
    for k, v in outs.items():
        setattr(q, k, v)
    return r._L.sptr_query_multi_hit(r._h, C.byref(q), C.c_void_p(stream) if stream else None)


def _renders_golden(r):
    g = np.load(os.path.join(GOLD, "radiance.npz"), allow_pickle=False)
    cam = sptr.camera_lookat(aspect=64 / 48)
    r.render(cam, 64, 48, spp=1, max_depth=6)
    rgb, acc = r.read_rgb8(), r.read_accum()
    frac = float((rgb == g["default_emitter_d6_rgb"]).all(axis=2).mean())
    rel = float(np.abs(acc - g["default_emitter_d6_accum"]).sum() / np.abs(g["default_emitter_d6_accum"]).sum())
    assert frac >= 0.995 and rel <= 5e-3, (frac, rel)  # (tests/test_gpu_golden.py's criteria for this frame)
    return rgb.tobytes(), acc.tobytes()


def test_errors_leave_the_context_usable(renderer):
    _, rays, _ = M.scene_reference("default_emitter")
    rays_dev = _dev(rays)
    n, K = len(rays), 4
    host = rays.ctypes.data
    out = {k: np.zeros(n * K * max(COLS[k], 1) if k != "count" else n, NP_DTYPE[k]) for k in ("count",) + FIELDS}
    ptr = {k: v.ctypes.data for k, v in out.items()}
    r = sptr.Renderer(0)
    assert _raw(r, host, n, 0, K, **ptr) == NO_SCENE
    with pytest.raises(sptr.SptrError, match="rc=-3:"):
        r.query_multi_hit(rays, K)
    r.close()
    r, _ = _context(R.SCENES[0])
    before = _renders_golden(r)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    shifted = torch.zeros(n * 8 + 4, dtype=torch.float32, device="cuda:0")[1:1 + n * 8]  # 4 bytes off 16-byte alignment
    assert shifted.data_ptr() % 16 == 4
    dcount = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    cases = {  # what is wrong: (sptr_last_error's text, the arguments)
        "any-hit flag": (b"query_multi_hit: SPTR_QUERY_ANY_HIT or unknown flags",
                         dict(rays=host, n=n, flags=sptr.SPTR_QUERY_ANY_HIT, max_hits=K, **ptr)),
        "unknown flag": (b"query_multi_hit: SPTR_QUERY_ANY_HIT or unknown flags",
                         dict(rays=host, n=n, flags=16, max_hits=K, **ptr)),
        "both sort flags": (b"query_multi_hit: SPTR_QUERY_SORT and SPTR_QUERY_NO_SORT exclude each other",
                            dict(rays=host, n=n, flags=sptr.SPTR_QUERY_SORT | sptr.SPTR_QUERY_NO_SORT, max_hits=K, **ptr)),
        "max_hits 0": (b"query_multi_hit: max_hits must be 1 .. SPTR_MULTI_HIT_MAX",
                       dict(rays=host, n=n, max_hits=0, **ptr)),
        "max_hits 17": (b"query_multi_hit: max_hits must be 1 .. SPTR_MULTI_HIT_MAX",
                        dict(rays=host, n=n, max_hits=17, **ptr)),
        "more than 2^28 rays": (b"query_multi_hit: more than 2^28 rays or hit slots",
                                dict(rays=host, n=(1 << 28) + 1, max_hits=1, **ptr)),
        "more than 2^28 slots": (b"query_multi_hit: more than 2^28 rays or hit slots",
                                 dict(rays=host, n=(1 << 24) + 1, max_hits=16, **ptr)),
        "NULL rays": (b"query_multi_hit: no rays",
                      dict(rays=None, n=n, max_hits=K, **ptr)),
        "NULL count": (b"query_multi_hit: the count output is required",
                       dict(rays=host, n=n, max_hits=K, **{k: v for k, v in ptr.items() if k != "count"})),
        "pad": (b"query_multi_hit: pad and reserved must be 0",
                dict(rays=host, n=n, max_hits=K, pad=1, **ptr)),
        "reserved": (b"query_multi_hit: pad and reserved must be 0",
                     dict(rays=host, n=n, max_hits=K, reserved=(0, 0, 0, 1), **ptr)),
        "host pointers on a stream": (b"query_multi_hit: host pointers cannot be enqueued on a stream",
                                      dict(rays=host, n=n, max_hits=K, stream=stream.cuda_stream, **ptr)),
        "misaligned device rays": (b"query_multi_hit: the device ray buffer must be 16-byte aligned",
                                   dict(rays=shifted.data_ptr(), n=n, flags=sptr.SPTR_QUERY_DEVICE_PTRS, max_hits=K,
                                        count=dcount.data_ptr())),
    }
    for what, (message, kw) in cases.items():
        assert _raw(r, **kw) == INVALID, what
        assert r._L.sptr_last_error(r._h) == message, what
        assert _renders_golden(r) == before, what  # the same bytes as before the refused call
    # (a lane context is the library's own and has no handle a caller could pass)
    with pytest.raises(sptr.SptrError):
        r.query_multi_hit(rays, K, stream=stream.cuda_stream)
    with pytest.raises(sptr.SptrError, match="rc=-1:"):
        r.query_multi_hit(shifted.view(n, 8), K)
    with pytest.raises(sptr.SptrError, match="rc=-1:"):
        r.query_multi_hit(rays, 17)
    with pytest.raises(sptr.SptrError):
        r.query_multi_hit(rays, K, fields=("colour",))
    assert all(not v.any() for v in out.values()) and not dcount.any()  # (no refused call wrote anything)
    assert _raw(r, None, 0, 0, K) == 0 and r.multi_hit_info()["queries"] == 0  # n == 0: OK, nothing launched
    assert r.multi_hit_info()["list_capacity"] == 0
    got = r.query_multi_hit(rays, K)  # and the context still answers
    assert (got["count"] > 1).sum() > 1000
    r.close()


def test_cli_multi_hit(tmp_path):
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"
    res = subprocess.run([exe, "--scene", "default_emitter", "--w", str(R.W), "--h", str(R.H), "--spp", "1", "--json",
                          "--query-centre-rays", "--multi-hit", "4", "--out", str(tmp_path / "img.ppm")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    _, rays, ref = M.scene_reference("default_emitter")
    count = MR.cut(ref, 4)["count"][:R.W * R.H]  # the pixel-centre rays come first
    mh = info["query"]["multi_hit"]
    print("sptr_cli --multi-hit 4:", info["query"])
    assert mh["k"] == 4 and mh["hits"] == int(count.sum())
    assert len(mh["count_hist"]) == 5 and sum(mh["count_hist"]) == R.W * R.H
    assert mh["count_hist"] == np.bincount(count, minlength=5).tolist()
    assert info["query"]["hits"] == R.W * R.H - mh["count_hist"][0]
    bad = subprocess.run([exe, "--scene", "default_emitter", "--multi-hit", "4", "--out", str(tmp_path / "x.ppm")],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
