"""GPU tests of signed distance queries: sptr_set_signed_distance / sptr_query_signed_distance / sptr_signed_info /
sptr_read_pseudonormals (kernels_signed.hip; the definition of csrc/pseudonormal.h) through Renderer and sptr_cli.

Scenes: signed_common's small meshes (an LDS-staged BVH2 each) and tests/refit_common.py's two: default_emitter (staged
BVH2) and the 30x70 sphere mesh with set_bvh_width(4).  The yardsticks are the host twins sptr_host_pseudonormals and
sptr_host_query_signed_distance: the same header, a stable sort and brute force, no tree, no device.

Rule everywhere (_same_bytes): every output of every point, and every table entry, is bit-equal to the twin's, nothing
excluded; the expected number of differing rows is 0.  A 2048-point subset of the sphere mesh and the star's 1024
points are also held to the float64 reference under the CPU test's rule (signed_common.check_signs).
Which rows that rule compares is decided by the float64 reference alone (signed_ref.reference_cos), never by the
device's output; test_signed_cpu.py's docstring has the one row of the sphere mesh where that matters."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import adversarial_common as A
import points_common as P
import refit_common as R
import signed_common as S
import sptr
import transform_common as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MISS = 0xFFFFFFFF
INVALID, NO_SCENE = -1, -3
FIELDS = S.FIELDS
COLS = {"geom": 1, "prim": 1, "dist2": 1, "dist": 1, "point": 3, "uv": 2, "ng": 3, "signed_dist": 1, "normal": 3, "feature": 1}
NP_DTYPE = {k: (np.uint32 if k in ("geom", "prim", "feature") else np.float32) for k in FIELDS}
SIGNED_ONLY = ("signed_dist", "normal", "feature")


def _width(name):
    return 4 if name == "sphere_mesh" else 0


def _context(name, flat=None, signed=True, dynamic=False, transforms=False, split=0):
    r = sptr.Renderer(0)
    r.set_bvh_width(_width(name))
    if split:
        r.set_split_refs(split)
    r.set_dynamic(dynamic, transforms=transforms)
    if signed:
        r.set_signed_distance(True)
    flat = P.flat(S.scene(name)) if flat is None else flat
    r.upload_scene(flat)
    r.set_materials(sptr.preset_materials(with_light=(name == "default_emitter")))
    r.set_lights(sptr.default_lights())
    r.set_environment(None)
    return r, flat


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


def _np(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _same_bytes(got, want, what):
    """Bit equality of every output of every row; prints the number of differing rows first."""
    assert got.keys() == want.keys(), what
    n = len(next(iter(want.values()))) if want else 0
    diff = np.zeros(n, bool)
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        if n:
            diff |= (got[k].view(np.uint32) != want[k].view(np.uint32)).reshape(n, -1).any(axis=1)
    print(f"{what}: {int(diff.sum())} of {n} rows differ")
    for q in np.flatnonzero(diff)[:4]:
        print(f"  row {q}: " + "; ".join(f"{k} {got[k][q]} vs {want[k][q]}" for k in got))
    assert not diff.any(), what


def _tables_equal(r, flat, what):
    tw = sptr.host_pseudonormals(flat)
    got = r.read_pseudonormals()
    info = r.signed_info()
    print(what, "signed_info", info)
    assert info["valid"] == 1 and info["num_tris"] == len(flat.indices) and info["table_bytes"] == 108 * len(flat.indices)
    for k in sptr._SIGNED_COUNTS:
        assert info[k] == tw[k], (what, k, info[k], tw[k])
    _same_bytes(got, {"nv": tw["nv"], "ne": tw["ne"]}, f"{what} tables")
    return info


@pytest.fixture(scope="module", params=S.ALL_NAMES)
def scene(request, renderer):
    """(name, context, flat scene, points, points on the device, the twin's answers)."""
    name = request.param
    r, flat = _context(name)
    pts = S.all_points(name)
    yield name, r, flat, pts, _dev(pts), S.twin(name)
    r.close()


@pytest.fixture(scope="module")
def mesh(renderer):
    r, flat = _context("sphere_mesh")
    yield r, flat
    r.close()


def test_tables_equal_the_twin(scene):
    name, r, flat, pts, pts_dev, tw = scene
    info = _tables_equal(r, flat, name)
    assert info["builds"] == 1 and info["ms_build"] > 0.0
    lay = r.scene_layout()
    assert (lay["lds_bytes"] != 0) == (name != "sphere_mesh")
    if name in S.MESH_NAMES:
        for k, v in S.meshes()[name][1].items():
            assert info[k] == v, (name, k)


def test_tables_with_split_references(renderer):
    r, flat = _context("sphere_mesh", split=4)
    _tables_equal(r, flat, "sphere_mesh with split references")
    pts = S.all_points("sphere_mesh")
    _same_bytes(_np(r.query_signed_distance(_dev(pts))), S.twin("sphere_mesh"), "sphere_mesh with split references")
    r.close()


def test_equals_the_twin(scene):
    name, r, flat, pts, pts_dev, tw = scene
    for path, arg in (("host", pts), ("device", pts_dev)):
        got = r.query_signed_distance(arg)
        assert isinstance(got["signed_dist"], np.ndarray if path == "host" else torch.Tensor)
        assert set(got) == set(FIELDS)
        _same_bytes(_np(got), tw, f"{name} ({path})")
    info = r.signed_info()
    assert info["ms_sign"] > 0.0 and info["builds"] == 1
    _same_bytes(_np(r.query_signed_distance(pts_dev, flip_triangles=True)), S.twin(name, True), f"{name} flipped")
    hits = tw["geom"] != MISS
    ntg = len(flat.tri_geom_first) - 1
    tri = hits & (tw["geom"] < ntg)
    fl = S.twin(name, True)["signed_dist"]
    assert (np.signbit(fl[tri]) != np.signbit(tw["signed_dist"][tri])).all()
    assert fl[~tri].tobytes() == tw["signed_dist"][~tri].tobytes()


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
def test_order_cannot_matter(scene, sort):
    name, r, flat, pts, pts_dev, tw = scene
    if name not in S.QUERY_SCENES and name != "star":
        return
    _same_bytes(_np(r.query_signed_distance(pts_dev, sort=sort)), tw, f"{name} sort={sort}")
    _same_bytes(r.query_signed_distance(pts, sort=sort), tw, f"{name} sort={sort}, host path")
    assert r.point_query_info()["sorted"] == int(sort)


@pytest.mark.parametrize("name", ("sphere_mesh", "star"))
def test_subset_against_float64(name, renderer):
    """Box and (for the sphere mesh the first 512 rows of) near against signed_ref under signed_common's rule."""
    r, flat = _context(name)
    try:
        failures = []
        for which, rows in (("box", slice(None)), ("near", slice(0, 512))):
            p = S.point_sets(name)[which][rows]
            got = _np(r.query_signed_distance(_dev(p)))
            try:
                S.check_signs(name, which, got, "device", rows=rows)
            except AssertionError as e:
                failures.append(str(e))
        assert not failures, failures
    finally:
        r.close()


# ------------------------------------------------------------------------------------- shapes
SHAPE_NS = (0, 1, 63, 64, 65, 257)
BIG = 600001  # more points than any resident grid has threads


@pytest.fixture(scope="module")
def shape_points(mesh):
    """600 001 points from default_rng(12) over the mesh scene's bounds grown by half, with radii inf, 0.5 and 0.05 in
    turn, and the twin's answers for the first 4096 and the last 4096."""
    sc = P.query_scene("sphere_mesh")
    c, _, lo, hi = A.bounds(sc)
    half = 0.5 * (hi - lo)
    pp = np.zeros((BIG, 4), np.float32)
    pp[:, :3] = np.random.default_rng(12).uniform(c - 1.5 * half, c + 1.5 * half, (BIG, 3))
    pp[:, 3] = np.tile(np.array([np.inf, 0.5, 0.05], np.float32), BIG // 3 + 1)[:BIG]
    pp.setflags(write=False)
    dev = _dev(pp)
    big = _np(mesh[0].query_signed_distance(dev, sort=False))
    head = sptr.host_query_signed_distance(mesh[1], pp[:4096])
    tail = sptr.host_query_signed_distance(mesh[1], pp[-4096:])
    _same_bytes({k: v[:4096] for k, v in big.items()}, head, "600 001 points, the first 4096")
    _same_bytes({k: v[-4096:] for k, v in big.items()}, tail, "600 001 points, the last 4096")
    assert 1000 < (head["feature"] == MISS).sum() < 3500
    return pp, dev, big


@pytest.mark.parametrize("sort", (False, True), ids=("unsorted", "sorted"))
@pytest.mark.parametrize("n", SHAPE_NS)
def test_shapes_where_indexing_can_break(mesh, shape_points, n, sort):
    r = mesh[0]
    pp, dev, big = shape_points
    want = {k: v[:n] for k, v in big.items()}  # (a point's result does not depend on its batch)
    for path, arg in (("host", pp[:n]), ("device", dev[:n])):
        got = _np(r.query_signed_distance(arg, sort=sort))
        assert got["signed_dist"].shape == (n,) and got["normal"].shape == (n, 3) and got["feature"].shape == (n,)
        _same_bytes(got, want, f"n={n} {path} sort={sort}")


def test_more_points_than_a_resident_grid_sorted(mesh, shape_points):
    pp, dev, big = shape_points
    _same_bytes(_np(mesh[0].query_signed_distance(dev, sort=True)), big, "600 001 points, sorted vs unsorted")


# ------------------------------------------------------------------------------------- NULL outputs
GUARD = 64  # elements on either side of an output


def _guarded(names, n):
    views, whole = {}, {}
    for k in names:
        shape = (n,) if COLS[k] == 1 else (n, COLS[k])
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


def test_null_outputs_and_guards(scene):
    name, r, flat, pts, pts_dev, tw = scene
    if name not in S.QUERY_SCENES and name != "star":
        return
    n = len(pts)
    subsets = [FIELDS] + [(k,) for k in SIGNED_ONLY] + [SIGNED_ONLY, ("geom", "signed_dist"), ("prim", "feature"),
                                                        ("dist", "point", "normal"), ()]
    for names in subsets:  # (without geom or prim the ids go into the query's scratch)
        views, whole = _guarded(names, n)
        part = r.query_signed_distance(pts_dev, fields=names, out=views)
        assert set(part) == set(names) and all(part[k].data_ptr() == views[k].data_ptr() for k in part)
        _guards_intact(whole)
        _same_bytes(_np(part), {k: tw[k] for k in names}, f"{name} only {names}")
    for names in (("signed_dist",), ("feature", "uv"), ("normal",), ()):
        _same_bytes(r.query_signed_distance(pts, fields=names), {k: tw[k] for k in names}, f"{name} only {names}, host path")


# ------------------------------------------------------------------------------------- moved scenes
@pytest.mark.parametrize("name", S.QUERY_SCENES)
def test_after_update_geometry(name, renderer):
    pts = S.all_points(name)
    pts_dev = _dev(pts)
    r, flat = _context(name, dynamic=True)
    before = _np(r.query_signed_distance(pts_dev))
    assert r.signed_info()["builds"] == 1
    pos, sph = R.deform(flat.positions, flat.spheres, 1)
    r.update_geometry(pos, sph)
    assert r.signed_info()["builds"] == 2
    moved = sptr.FlatScene(pos, flat.indices, flat.tri_geom_first, sph, flat.geom_material)
    want = sptr.host_query_signed_distance(moved, pts)
    _tables_equal(r, moved, f"{name} after update_geometry")
    fresh, _ = _context(name, flat=moved)
    _same_bytes(_np(fresh.query_signed_distance(pts_dev)), want, f"{name} fresh upload of the moved scene vs the twin")
    _same_bytes(fresh.read_pseudonormals(), r.read_pseudonormals(), f"{name} refitted tables vs a fresh upload's")
    for sort in (False, True):
        _same_bytes(_np(r.query_signed_distance(pts_dev, sort=sort)), want, f"{name} refitted vs the twin, sort={sort}")
    assert (want["signed_dist"].view(np.uint32) != before["signed_dist"].view(np.uint32)).mean() >= 0.2
    r.update_geometry(None, sph)  # spheres alone: the triangles' tables are rebuilt from the kept corners
    assert r.signed_info()["builds"] == 3
    _same_bytes(_np(r.query_signed_distance(pts_dev)), want, f"{name} after a sphere-only update")
    fresh.close()
    r.close()


@pytest.mark.parametrize("name", S.QUERY_SCENES)
def test_after_update_transforms(name, renderer):
    pts = S.all_points(name)
    pts_dev = _dev(pts)
    sc = S.scene(name)
    r, flat = _context(name, transforms=True)
    before = _np(r.query_signed_distance(pts_dev))
    mats = X.matrices((0.0,), 1)
    pos = X.transform_geometries(sc, mats)
    sph = R.deform(flat.positions, flat.spheres, 1)[1]
    r.update_transforms(mats, sph)
    assert r.signed_info()["builds"] == 2
    moved = sptr.FlatScene(pos, flat.indices, flat.tri_geom_first, sph, flat.geom_material)
    want = sptr.host_query_signed_distance(moved, pts)
    _tables_equal(r, moved, f"{name} after update_transforms")
    fresh, _ = _context(name, flat=moved)
    _same_bytes(_np(fresh.query_signed_distance(pts_dev)), want, f"{name} fresh upload of the transformed scene vs the twin")
    _same_bytes(_np(r.query_signed_distance(pts_dev)), want, f"{name} transformed vs the twin")
    _same_bytes(_np(r.query_signed_distance(pts_dev, sort=True)), want, f"{name} transformed vs the twin, sorted")
    assert (want["signed_dist"].view(np.uint32) != before["signed_dist"].view(np.uint32)).mean() >= 0.2
    fresh.close()
    r.close()


# ------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize("name", S.QUERY_SCENES)
def test_async_on_a_torch_stream(name, renderer):
    r, flat = _context(name)
    pts = S.all_points(name)
    pts_dev, tw = _dev(pts), S.twin(name)
    rays_dev = _dev(R.rays(sptr.camera_lookat(aspect=R.W / R.H).as_array()))
    want_rays = _np(r.query_rays(rays_dev))
    want_points = _np(r.query_points(pts_dev))
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(stream):
        old = r.query_rays(rays_dev, stream=stream.cuda_stream)  # (same stream: shared scratch)
        got = r.query_signed_distance(pts_dev, fields=SIGNED_ONLY, stream=stream.cuda_stream)  # (ids in scratch)
        plain = r.query_points(pts_dev, stream=stream.cuda_stream)
        full = r.query_signed_distance(pts_dev, stream=stream.cuda_stream)
    stream.synchronize()
    _same_bytes(_np(got), {k: tw[k] for k in SIGNED_ONLY}, f"{name} enqueued between a ray query and a point query")
    _same_bytes(_np(full), tw, f"{name} enqueued after the point query")
    for a, b in ((_np(old), want_rays), (_np(plain), want_points)):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert r.signed_info()["ms_sign"] > 0.0
    r.close()


def test_a_context_without_the_option_answers_as_before(renderer):
    """query_points of a context that never set the option: the twin's bytes, and the bytes of a context that did."""
    for name in S.QUERY_SCENES:
        pts = S.all_points(name)
        plain, _ = _context(name, signed=False)
        info = plain.signed_info()
        assert info["valid"] == 0 and info["builds"] == 0 and info["table_bytes"] == 0
        got = plain.query_points(pts)
        _same_bytes(got, P.twin(name), f"{name} without the option")
        with_opt, _ = _context(name)
        _same_bytes(with_opt.query_points(pts), got, f"{name} with the option, query_points")
        plain.close()
        with_opt.close()


# ------------------------------------------------------------------------------------- errors
def _raw(r, points=None, n=0, flags=0, reserved=(0, 0, 0, 0), reserved2=(0, 0, 0, 0), stream=None, **outs):
    q = sptr.SignedQuery()
    q.q.points, q.q.n, q.q.flags = points, n, flags
    for i, v in enumerate(reserved):
        q.q.reserved[i] = v
    for i, v in enumerate(reserved2):
        q.reserved[i] = v
    for k, v in outs.items():
        sptr._signed_query_set(q, k, v)
    return r._L.sptr_query_signed_distance(r._h, C.byref(q), C.c_void_p(stream) if stream else None)


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
    pts = S.all_points("default_emitter")
    n = len(pts)
    host = pts.ctypes.data
    out = {k: np.zeros(n * COLS[k], NP_DTYPE[k]) for k in FIELDS}
    ptr = {k: v.ctypes.data for k, v in out.items()}
    r = sptr.Renderer(0)
    assert _raw(r, host, n, 0, **ptr) == NO_SCENE
    r.close()
    # no set_signed_distance before the upload
    r, _ = _context("default_emitter", signed=False)
    before = _renders_golden(r)
    assert _raw(r, host, n, 0, **ptr) == INVALID and b"set_signed_distance" in r._L.sptr_last_error(r._h)
    with pytest.raises(sptr.SptrError, match="rc=-1:"):
        r.query_signed_distance(pts)
    with pytest.raises(sptr.SptrError, match="rc=-1:"):
        r.read_pseudonormals()
    assert _renders_golden(r) == before
    # the option set after the upload changes nothing until the next upload
    r.set_signed_distance(True)
    assert _raw(r, host, n, 0, **ptr) == INVALID
    assert _renders_golden(r) == before
    r.close()
    r, _ = _context("default_emitter")
    before = _renders_golden(r)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    shifted = torch.zeros(n * 4 + 4, dtype=torch.float32, device="cuda:0")[1:1 + n * 4]  # 4 bytes off 16-byte alignment
    good = torch.zeros(n * 4, dtype=torch.float32, device="cuda:0")
    dsd = torch.zeros(n + 1, dtype=torch.float32, device="cuda:0")
    dbytes = dsd.view(torch.uint8)[2:2 + 4 * n]  # 2 bytes off 4-byte alignment
    assert shifted.data_ptr() % 16 == 4 and dbytes.data_ptr() % 4 == 2
    DEV = sptr.SPTR_QUERY_DEVICE_PTRS
    cases = {  # what is wrong: (sptr_last_error's text, the arguments)
        "any-hit flag": (b"query_signed_distance: SPTR_QUERY_ANY_HIT or unknown flags",
                         dict(points=host, n=n, flags=sptr.SPTR_QUERY_ANY_HIT, **ptr)),
        "unknown flag": (b"query_signed_distance: SPTR_QUERY_ANY_HIT or unknown flags",
                         dict(points=host, n=n, flags=64, **ptr)),
        "both sort flags": (b"query_signed_distance: SPTR_QUERY_SORT and SPTR_QUERY_NO_SORT exclude each other",
                            dict(points=host, n=n, flags=sptr.SPTR_QUERY_SORT | sptr.SPTR_QUERY_NO_SORT, **ptr)),
        "more than 2^28 points": (b"query_signed_distance: more than 2^28 points",
                                  dict(points=host, n=(1 << 28) + 1, **ptr)),
        "NULL points": (b"query_signed_distance: no points",
                        dict(points=None, n=n, **ptr)),
        "reserved of the point query": (b"query_signed_distance: reserved must be 0",
                                        dict(points=host, n=n, reserved=(0, 1, 0, 0), **ptr)),
        "reserved": (b"query_signed_distance: reserved must be 0",
                     dict(points=host, n=n, reserved2=(0, 0, 0, 1), **ptr)),
        "host pointers on a stream": (b"query_signed_distance: host pointers cannot be enqueued on a stream",
                                      dict(points=host, n=n, stream=stream.cuda_stream, **ptr)),
        "misaligned device points": (b"query_signed_distance: the device point buffer must be 16-byte aligned, the outputs 4-byte aligned",
                                     dict(points=shifted.data_ptr(), n=n, flags=DEV, signed_dist=dsd.data_ptr())),
        "misaligned device output": (b"query_signed_distance: the device point buffer must be 16-byte aligned, the outputs 4-byte aligned",
                                     dict(points=good.data_ptr(), n=n, flags=DEV, signed_dist=dbytes.data_ptr())),
    }
    for what, (message, kw) in cases.items():
        assert _raw(r, **kw) == INVALID, what
        assert r._L.sptr_last_error(r._h) == message, what
        assert _renders_golden(r) == before, what  # the same bytes as before the refused call
    # (a lane context is the library's own and has no handle a caller could pass)
    with pytest.raises(sptr.SptrError):
        r.query_signed_distance(pts, stream=stream.cuda_stream)
    with pytest.raises(sptr.SptrError):
        r.query_signed_distance(pts, fields=("colour",))
    assert all(not v.any() for v in out.values()) and not dsd.any()  # (no refused call wrote anything)
    queries = r.point_query_info()["queries"]
    assert _raw(r, None, 0, 0) == 0 and r.point_query_info()["queries"] == queries  # n == 0: OK, nothing launched
    _same_bytes(r.query_signed_distance(pts), S.twin("default_emitter"), "after the refused calls")
    assert _renders_golden(r) == before
    r.close()


def test_cli_signed_grid(tmp_path):
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"
    N = 16
    sc = P.query_scene("default_emitter")
    pos, s = sc["positions"].astype(np.float64), sc["spheres"].astype(np.float64)
    lo = np.minimum(pos.min(axis=0), (s[:, :3] - s[:, 3:4]).min(axis=0))
    hi = np.maximum(pos.max(axis=0), (s[:, :3] + s[:, 3:4]).max(axis=0))
    c, h = (lo + hi) / 2.0, (hi - lo) / 2.0
    ax = [((c[a] - 1.1 * h[a]) + (2.2 * h[a]) * ((np.arange(N) + 0.5) / N)).astype(np.float32) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), z.ravel(), np.full(N ** 3, np.inf, np.float32)], axis=1).astype(np.float32)
    tables = sptr.host_pseudonormals(P.flat(sc))
    for flip in (False, True):
        res = subprocess.run([exe, "--scene", "default_emitter", "--w", "64", "--h", "48", "--spp", "1", "--json",
                              "--query-points-grid", str(N), "--signed"] + (["--flip"] if flip else [])
                             + ["--out", str(tmp_path / "img.ppm")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        info = json.loads(res.stdout.strip().splitlines()[-1])["signed"]
        print(f"sptr_cli --query-points-grid 16 --signed{' --flip' if flip else ''}:", info)
        tw = sptr.host_query_signed_distance(P.flat(sc), pts, flip_triangles=flip)
        miss = tw["feature"] == MISS
        neg = np.signbit(tw["signed_dist"]) & ~miss
        assert info["flip"] == int(flip) and info["missed"] == int(miss.sum()) == 0
        assert info["negative"] == int(neg.sum()) and info["positive"] == N ** 3 - int(neg.sum())
        assert 0 < info["negative"] < N ** 3
        for k in sptr._SIGNED_COUNTS:
            assert info[k] == tables[k], k
