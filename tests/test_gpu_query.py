"""GPU tests of ray queries on caller buffers: sptr_query_rays / sptr_query_info (k_rayquery, k_ray_keys,
kernels_query.h) through Renderer.query_rays / query_info, HipBackend::queryRays and sptr_cli.

Scenes and rays are tests/refit_common.py's: default_emitter (an LDS-staged BVH2 with leaf ranges) and the
30x70 sphere mesh with set_bvh_width(4) (treelets, the quantised BVH4 walked from L2), 20 492 rays.  The
yardstick is Renderer.intersect / occluded (sptr_intersect / sptr_occluded, k_query) on the same context, by
refit_common's rule: every ray bit-equal in geomID, primID, t and Ng, at most 1e-4 of them naming another
primitive at a bit-equal t (tests/test_refit_cpu.py: these rays hold no such ties, so 0 is expected).
Barycentrics are checked by tests/query_common.py's bound (pinned on the CPU by tests/test_query_cpu.py).

One context per scene serves the module; the tests that change a context's scene make their own."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import query_common as Q
import refit_common as R
import sptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MISS = 0xFFFFFFFF
INVALID, NO_SCENE = -1, -3
CLOSEST = ("geom", "prim", "t", "ng", "uv")
COLS = {"geom": 1, "prim": 1, "t": 1, "ng": 3, "uv": 2, "occluded": 1}
DTYPE = {"geom": torch.uint32, "prim": torch.uint32, "t": torch.float32, "ng": torch.float32, "uv": torch.float32,
         "occluded": torch.uint8}
NP_DTYPE = {"geom": np.uint32, "prim": np.uint32, "t": np.float32, "ng": np.float32, "uv": np.float32,
            "occluded": np.uint8}
SHAPE_NS =(0, 1, 63, 64, 65, 257, 600001)  # 600 001: more rays than any resident grid has threads


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


@pytest.fixture(scope="module")
def rays():
    return R.rays(sptr.camera_lookat(aspect=R.W / R.H).as_array())


@pytest.fixture(scope="module")
def rays_dev(rays):
    t = torch.from_numpy(rays.copy()).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module", params=R.SCENES, ids=R.SCENE_IDS)
def scene(request, rays):
    """(config, context, flat scene, Renderer.intersect's and Renderer.occluded's results on the rays)."""
    r, flat = _context(request.param)
    hits, occ = r.intersect(rays), r.occluded(rays)
    assert (hits[0] != MISS).sum() > 1000 and 1000 < occ.sum() < len(occ)
    yield request.param, r, flat, hits, occ
    r.close()


@pytest.fixture(scope="module")
def mesh(rays):
    r, flat = _context(R.SCENES[1])
    yield r, flat
    r.close()


def _np(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _hits(res):
    return res["geom"], res["prim"], res["t"], res["ng"]


def _same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_equals_the_yardstick(scene, rays, rays_dev):
    cfg, r, _, hits, occ = scene
    for path, arg in (("host", rays), ("device", rays_dev)):
        got = r.query_rays(arg)
        assert isinstance(got["t"], np.ndarray if path == "host" else torch.Tensor)
        got = _np(got)
        assert set(got) == set(CLOSEST) and got["uv"].shape == (len(rays), 2) and got["ng"].shape == (len(rays), 3)
        assert R.compare_hits(_hits(got), hits, f"{cfg[0]} query_rays ({path}) vs intersect") == 0
        any_hit = _np(r.query_rays(arg, any_hit=True))
        assert set(any_hit) == {"occluded"} and any_hit["occluded"].dtype == np.uint8
        assert R.compare_occluded(any_hit["occluded"], occ, f"{cfg[0]} query_rays any_hit ({path}) vs occluded") == 0
    assert "uv" not in r.query_rays(rays, uv=False)


def test_order_cannot_matter(scene, rays, rays_dev):
    cfg, r, _, _, _ = scene
    n0 = r.query_info()["queries"]
    for path, arg in (("host", rays), ("device", rays_dev)):
        for any_hit in (False, True):
            plain = _np(r.query_rays(arg, any_hit=any_hit, sort=False))
            info = r.query_info()
            assert info["sorted"] == 0 and info["ms_sort"] == 0.0 and info["ms_trace"] > 0.0
            ordered = _np(r.query_rays(arg, any_hit=any_hit, sort=True))
            info = r.query_info()
            print(cfg[0], path, "any_hit" if any_hit else "closest", info)
            assert info["sorted"] == 1 and info["ms_sort"] > 0.0 and info["ms_trace"] > 0.0
            _same_bytes(ordered, plain, f"{cfg[0]} {path} sorted vs unsorted")
    assert r.query_info()["queries"] == n0 + 8


@pytest.fixture(scope="module")
def shape_rays(mesh):
    """600 001 rays from default_rng(11) over refit_common.rays' boxes, and Renderer.intersect's results."""
    n = max(SHAPE_NS)
    rng = np.random.default_rng(11)
    o = rng.uniform([-6.0, 0.0, -6.0], [6.0, 5.0, 8.0], (n, 3))
    tg = rng.uniform([-3.0, 0.0, -3.0], [3.0, 3.0, 5.0], (n, 3))
    d = tg - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rr = np.zeros((n, 8), np.float32)
    rr[:, 0:3] = o
    rr[:, 3:6] = d
    rr[:, 7] = np.inf
    rr.setflags(write=False)
    dev = torch.from_numpy(rr.copy()).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return rr, dev, mesh[0].intersect(rr)


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
@pytest.mark.parametrize("n", SHAPE_NS)
def test_shapes_where_indexing_can_break(mesh, shape_rays, n, sort):
    r = mesh[0]
    rr, dev, ref = shape_rays
    want = tuple(a[:n] for a in ref)  # (a ray's result does not depend on its batch)
    for path, arg in (("host", rr[:n]), ("device", dev[:n])):
        got = _np(r.query_rays(arg, sort=sort))
        assert all(len(got[k]) == n for k in CLOSEST)
        if n:
            R.compare_hits(_hits(got), want, f"n={n} {path} sort={sort}")
            assert r.query_info()["sorted"] == int(sort)
        occ = _np(r.query_rays(arg, any_hit=True, sort=sort))["occluded"]
        assert occ.shape == (n,)
        # tfar is inf: a ray is occluded exactly when it has a closest hit
        assert R.compare_occluded(occ, (want[0] != MISS).astype(np.uint8), f"n={n} {path} any_hit sort={sort}") <= 1e-4 * n


GUARD = 64  # elements on either side of an output


def _guarded(names, n):
    """Outputs of n rays inside larger device tensors filled with a sentinel: ({name: view}, {name: whole})."""
    views, whole = {}, {}
    for k in names:
        m = n * COLS[k]
        dt = NP_DTYPE[k]
        big = torch.from_numpy(np.full(m + 2 * GUARD, 0x5A if dt == np.uint8 else 123456789, dt)).to("cuda:0")
        assert big.dtype == DTYPE[k]
        whole[k] = big
        views[k] = big[GUARD:GUARD + m].view((n, COLS[k]) if COLS[k] > 1 else (n,))
    torch.cuda.synchronize()
    return views, whole


def _guards_intact(whole):
    for k, big in whole.items():
        a = big.cpu().numpy()
        sentinel = a.dtype.type(0x5A if a.dtype == np.uint8 else 123456789)
        assert (a[:GUARD] == sentinel).all() and (a[-GUARD:] == sentinel).all(), k


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
def test_null_outputs_and_guard_pages(scene, rays_dev, sort):
    cfg, r, _, _, _ = scene
    n = rays_dev.shape[0]
    views, whole = _guarded(CLOSEST, n)
    full = r.query_rays(rays_dev, sort=sort, out=views)
    assert all(full[k].data_ptr() == views[k].data_ptr() for k in CLOSEST)
    _guards_intact(whole)
    full = _np(full)
    _same_bytes(full, _np(r.query_rays(rays_dev, sort=sort)), f"{cfg[0]} caller-allocated vs library-allocated outputs")
    for names in (("t",), ("geom", "uv")):
        views, whole = _guarded(names, n)
        part = r.query_rays(rays_dev, sort=sort, fields=names, out=views)
        assert set(part) == set(names)
        _guards_intact(whole)
        _same_bytes(_np(part), {k: full[k] for k in names}, f"{cfg[0]} only {names}")
        _same_bytes(r.query_rays(rays_dev.cpu().numpy(), sort=sort, fields=names), {k: full[k] for k in names},
                    f"{cfg[0]} only {names}, host path")
    views, whole = _guarded(("occluded",), n)
    r.query_rays(rays_dev, any_hit=True, sort=sort, out=views)
    _guards_intact(whole)


def test_barycentrics(scene, rays, rays_dev):
    cfg, r, flat, _, _ = scene
    got = _np(r.query_rays(rays_dev))
    mask, tri = Q.triangle_hits(flat.tri_geom_first, got["geom"], got["prim"])
    assert mask.sum() > 500
    Q.check_barycentrics(got["uv"][mask, 0], got["uv"][mask, 1], flat.positions, flat.indices, rays[mask], tri,
                         f"{cfg[0]} device")
    # spheres and misses: exactly zero (the reference's sphere callbacks set no u or v)
    assert (got["geom"] == MISS).sum() > 0
    assert not got["uv"][~mask].any() and (got["uv"][~mask].view(np.uint32) == 0).all()
    if cfg[0] == "default_emitter":
        sph = (got["geom"] != MISS) & ~mask
        assert sph.sum() > 1000 and (got["prim"][sph] == 0).all()
    # the float32 hit point, by the header's convention, against o + t d
    u, v = got["uv"][mask, 0].astype(np.float64), got["uv"][mask, 1].astype(np.float64)
    p = flat.positions.astype(np.float64)
    i = flat.indices.astype(np.int64)[tri]
    point = (1.0 - u - v)[:, None] * p[i[:, 0]] + u[:, None] * p[i[:, 1]] + v[:, None] * p[i[:, 2]]
    rr = rays[mask].astype(np.float64)
    gap = np.linalg.norm(point - (rr[:, 0:3] + got["t"][mask].astype(np.float64)[:, None] * rr[:, 3:6]), axis=1)
    print(f"{cfg[0]}: worst |(1-u-v) v0 + u v1 + v v2 - (o + t d)| = {gap.max():.2e}")
    assert gap.max() <= 2e-5  # (as tests/test_query_cpu.py)


@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_after_a_refit(cfg, rays, rays_dev):
    r, flat = _context(cfg, dynamic=True)
    before = _np(r.query_rays(rays_dev))
    r.update_geometry(*R.deform(flat.positions, flat.spheres, 1))
    want = r.intersect(rays)
    for sort in (False, True):
        got = _np(r.query_rays(rays_dev, sort=sort))
        assert R.compare_hits(_hits(got), want, f"{cfg[0]} after a refit, sort={sort}") == 0
    assert (got["t"].view(np.uint32) != before["t"].view(np.uint32)).mean() >= 0.2  # (the deformation matters)
    moved_positions, _ = R.deform(flat.positions, flat.spheres, 1)
    mask, tri = Q.triangle_hits(flat.tri_geom_first, got["geom"], got["prim"])
    Q.check_barycentrics(got["uv"][mask, 0], got["uv"][mask, 1], moved_positions, flat.indices, rays[mask], tri,
                         f"{cfg[0]} after a refit")
    R.compare_occluded(_np(r.query_rays(rays_dev, any_hit=True))["occluded"], r.occluded(rays), f"{cfg[0]} after a refit")
    r.close()


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
def test_async_on_a_torch_stream(scene, rays_dev, sort):
    cfg, r, _, _, _ = scene
    want = _np(r.query_rays(rays_dev, sort=sort))
    want_occ = _np(r.query_rays(rays_dev, any_hit=True, sort=sort))
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(stream):
        got = r.query_rays(rays_dev, sort=sort, stream=stream.cuda_stream)
        occ = r.query_rays(rays_dev, any_hit=True, sort=sort, stream=stream.cuda_stream)  # (same stream: shared scratch)
    stream.synchronize()
    _same_bytes(_np(got), want, f"{cfg[0]} enqueued vs synchronous")
    _same_bytes(_np(occ), want_occ, f"{cfg[0]} enqueued any_hit vs synchronous")
    info = r.query_info()
    assert info["sorted"] == int(sort) and info["ms_trace"] > 0.0


def _raw(r, rays=None, n=0, flags=0, stream=None, **outs):
    q = sptr.RayQuery()
    q.rays, q.n, q.flags = rays, n, flags
    for k, v in outs.items():
        setattr(q, k, v)
    return r._L.sptr_query_rays(r._h, C.byref(q), C.c_void_p(stream) if stream else None)


def _renders_golden(r):
    g = np.load(os.path.join(GOLD, "radiance.npz"), allow_pickle=False)
    cam = sptr.camera_lookat(aspect=64 / 48)
    r.render(cam, 64, 48, spp=1, max_depth=6)
    rgb, acc = r.read_rgb8(), r.read_accum()
    frac = float((rgb == g["default_emitter_d6_rgb"]).all(axis=2).mean())
    rel = float(np.abs(acc - g["default_emitter_d6_accum"]).sum() / np.abs(g["default_emitter_d6_accum"]).sum())
    assert frac >= 0.995 and rel <= 5e-3, (frac, rel)  # (tests/test_gpu_golden.py's criteria for this frame)


def test_errors_leave_the_context_usable(rays, rays_dev):
    n = len(rays)
    host = rays.ctypes.data
    out = {k: np.zeros(n * COLS[k], np.uint32 if k in ("geom", "prim") else np.float32) for k in CLOSEST}
    ptr = {k: v.ctypes.data for k, v in out.items()}
    occ = np.zeros(n, np.uint8)
    r = sptr.Renderer(0)
    assert _raw(r, host, n, 0, **ptr) == NO_SCENE
    assert _raw(r, host, n, sptr.SPTR_QUERY_ANY_HIT, occluded=occ.ctypes.data) == NO_SCENE
    with pytest.raises(sptr.SptrError, match="rc=-3:"):
        r.query_rays(rays)
    r.close()
    r, _ = _context(R.SCENES[0])
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    shifted = torch.zeros(n * 8 + 4, dtype=torch.float32, device="cuda:0")[1:1 + n * 8]  # 4 bytes off 16-byte alignment
    assert shifted.data_ptr() % 16 == 4
    cases = {  # what is wrong: (sptr_last_error's text, the arguments)
        "both sort flags": (b"query_rays: SPTR_QUERY_SORT and SPTR_QUERY_NO_SORT exclude each other",
                            dict(rays=host, n=n, flags=sptr.SPTR_QUERY_SORT | sptr.SPTR_QUERY_NO_SORT, **ptr)),
        "more than 2^28 rays": (b"query_rays: more than 2^28 rays",
                                dict(rays=host, n=(1 << 28) + 1, flags=0, **ptr)),
        "NULL rays": (b"query_rays: no rays",
                      dict(rays=None, n=n, flags=0, **ptr)),
        "any-hit without occluded": (b"query_rays: SPTR_QUERY_ANY_HIT needs the occluded output",
                                     dict(rays=host, n=n, flags=sptr.SPTR_QUERY_ANY_HIT, **ptr)),
        "any-hit without occluded, n = 0": (b"query_rays: SPTR_QUERY_ANY_HIT needs the occluded output",
                                            dict(rays=None, n=0, flags=sptr.SPTR_QUERY_ANY_HIT)),
        "host pointers on a stream": (b"query_rays: host pointers cannot be enqueued on a stream",
                                      dict(rays=host, n=n, flags=0, stream=stream.cuda_stream, **ptr)),
        "misaligned device rays": (b"query_rays: the device ray buffer must be 16-byte aligned",
                                   dict(rays=shifted.data_ptr(), n=n, flags=sptr.SPTR_QUERY_DEVICE_PTRS,
                                        t=rays_dev.data_ptr())),
        "unknown flag": (b"query_rays: unknown flags",
                         dict(rays=host, n=n, flags=16, **ptr)),
    }
    for what, (message, kw) in cases.items():
        assert _raw(r, **kw) == INVALID, what
        assert r._L.sptr_last_error(r._h) == message, what
        _renders_golden(r)
    with pytest.raises(sptr.SptrError):
        r.query_rays(rays, stream=stream.cuda_stream)
    with pytest.raises(sptr.SptrError, match="rc=-1:"):
        r.query_rays(shifted.view(n, 8))
    with pytest.raises(sptr.SptrError):
        r.query_rays(rays, fields=("colour",))
    assert all(not v.any() for v in out.values())  # (no refused call wrote anything)
    assert _raw(r, None, 0, 0) == 0 and r.query_info()["queries"] == 0  # n == 0: OK, nothing launched
    got = r.query_rays(rays)  # and the context still answers
    assert (got["geom"] != MISS).sum() > 1000
    r.close()


def test_cli_query_centre_rays(tmp_path):
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"
    res = subprocess.run([exe, "--scene", "default", "--w", str(R.W), "--h", str(R.H), "--spp", "1", "--json",
                          "--query-centre-rays", "--out", str(tmp_path / "img.ppm")], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    r = sptr.Renderer(0)
    flat = sptr.setup_default(r, "default")
    r.render(sptr.camera_lookat(aspect=R.W / R.H), R.W, R.H, spp=1)
    ids = r.read_aov(sptr.SPTR_AOV_ID)
    r.close()
    hits = int((ids[..., 0] != MISS).sum())
    tri = int((ids[..., 0] < len(flat.tri_geom_first) - 1).sum())
    print("sptr_cli --query-centre-rays:", info["query"], "AOV hits", hits, "triangle hits", tri)
    assert info["query"] == {"rays": R.W * R.H, "hits": hits, "tri_hits": tri}
    assert 0 < tri < hits < R.W * R.H
