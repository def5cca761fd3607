"""GPU tests of per-geometry transforms on the device: sptr_set_dynamic(SPTR_DYNAMIC_TRANSFORMS),
sptr_set_rest_positions, sptr_update_transforms (k_refit_slots<true>, kernels_refit.hip) and sptr_tree_cost
(k_tree_cost).  DESIGN.md 6c, "Transforms".

Scenes, matrices, the float32 restatement of the per-vertex arithmetic and the expected world positions are
tests/transform_common.py's (checked on the CPU oracle by tests/test_transform_cpu.py); rays and the comparison
rules are tests/refit_common.py's.  Every test creates its own contexts and closes them; at most two are alive
at once.

What is compared with what:
  - against a fresh upload of the expected world positions, the tree differs (the upload's topology against the
    moved scene's), so queries go through compare_hits / compare_occluded: at most 1e-4 of the rays may name
    another primitive, at a bit-equal distance;
  - against sptr_update_geometry(expected positions) on a context that uploaded the same scene, the tree is the
    same and the device must have computed the same vertices: 0 differing rays, byte-equal images, equal
    traversal counters (which only agree if every box, BVH2 and quantised, is the same bit for bit).
The lane-context error of sptr_update_transforms is not reachable through a Renderer (a lane context is internal
to its parent) and is not tested here."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import refit_common as R
import sptr
import transform_common as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = R.W, R.H
INVALID, NO_SCENE = "rc=-1:", "rc=-3:"
COUNTERS = ("node_visits", "tri_tests", "sphere_tests", "shadow_node_visits")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _flat(scene, pos=None, sph=None):
    return sptr.FlatScene(scene["positions"] if pos is None else pos, scene["indices"], scene["tri_geom_first"],
                          scene["spheres"] if sph is None else sph, scene["geom_material"])


def _context(cfg, flat, dynamic=False, transforms=False, split_refs=0):
    _, name, _, _, width, _ = cfg
    r = sptr.Renderer(0)
    r.set_bvh_width(width)
    if split_refs:
        r.set_split_refs(split_refs)
    r.set_dynamic(dynamic, transforms=transforms)
    r.upload_scene(flat)
    r.set_materials(sptr.preset_materials(with_light=(name == "default_emitter")))
    r.set_lights(sptr.default_lights())
    r.set_environment(None)
    lay = r.scene_layout()
    assert (lay["lds_bytes"] != 0) == (width == 0) and lay["bvh_width"] == (4 if width else 2)
    return r


@pytest.fixture(scope="module")
def cam():
    return sptr.camera_lookat(aspect=W / H)


@pytest.fixture(scope="module")
def rays(cam):
    return R.rays(cam.as_array())


@pytest.fixture(scope="module", params=X.SCENES, ids=X.SCENE_IDS)
def data(request):
    """The composite scene, and per step k its matrices and expected (positions, spheres): computed once."""
    cfg = request.param
    _, name, p0, p1, _, shifts = cfg
    b = sptr.builtin_scene(name, p0, p1)
    scene = X.compose({"positions": b.positions, "indices": b.indices, "tri_geom_first": b.tri_geom_first,
                       "spheres": b.spheres, "geom_material": b.geom_material}, shifts)
    return {"cfg": cfg, "tag": cfg[0], "scene": scene, "mats": {k: X.matrices(shifts, k) for k in (0, 1, 2)},
            "exp": {k: X.expected(scene, shifts, k) for k in (0, 1, 2)}}


def _queries(r, rays):
    return r.intersect(rays), r.occluded(rays)


def _same_queries(a, b, what):
    R.compare_hits(a[0], b[0], what)
    R.compare_occluded(a[1], b[1], what)


def _exact_queries(a, b, what=""):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(_bits(x), _bits(y)), what
    assert np.array_equal(a[1], b[1]), what


def _render(r, cam, **kw):
    st = r.render(cam, W, H, spp=4, **kw)
    return r.read_accum(), r.read_rgb8(), st


def _state(r, rays, cam):
    """Queries, a 4-spp image and the traversal counters of the scene as it stands."""
    q = _queries(r, rays)
    img = _render(r, cam)
    cnt = _render(r, cam, flags=sptr.SPTR_FRAME_COUNT_VISITS)[2]
    return q, img, {k: getattr(cnt, k) for k in COUNTERS}


def _exact_state(a, b, what):
    _exact_queries(a[0], b[0], what)
    assert np.array_equal(_bits(a[1][0]), _bits(b[1][0])), what
    assert np.array_equal(a[1][1], b[1][1]), what
    print(what, a[2], b[2])
    assert a[2] == b[2], what
    assert a[2]["node_visits"] > 0 and a[2]["shadow_node_visits"] > 0


# ------------------------------------------------------------------ 1. against a fresh upload of the moved scene
def test_transforms_equal_fresh_upload(data, rays):
    cfg, scene = data["cfg"], data["scene"]
    dyn = _context(cfg, _flat(scene), transforms=True)
    before = dyn.intersect(rays)
    for k in (1, 2):  # 2 after 1: each call starts from the rest pose, transforms do not accumulate
        pos, sph = data["exp"][k]
        dyn.update_transforms(data["mats"][k], sph)
        fresh = _context(cfg, _flat(scene, pos, sph))
        got = _queries(dyn, rays)
        _same_queries(got, _queries(fresh, rays), f"{data['tag']} k={k} transforms vs fresh upload")
        fresh.close()
        changed = (got[0][0] != before[0]) | (got[0][1] != before[1]) | (_bits(got[0][2]) != _bits(before[2]))
        assert changed.mean() >= 0.2  # (the step matters: tests/test_transform_cpu.py)
    assert dyn.refit_info()["refits"] == 2
    dyn.close()


# ------------------------------------------------------------------ 2. against update_geometry on the same tree
def test_transforms_equal_update_geometry_bit_for_bit(data, rays, cam):
    cfg, scene = data["cfg"], data["scene"]
    a = _context(cfg, _flat(scene), transforms=True)
    b = _context(cfg, _flat(scene), transforms=True)
    for k in (1, 2):
        pos, sph = data["exp"][k]
        a.update_transforms(data["mats"][k], sph)
        b.update_geometry(pos, sph)
        _exact_state(_state(a, rays, cam), _state(b, rays, cam), f"{data['tag']} k={k} update_transforms vs update_geometry")
    # a later update_geometry leaves the rest pose alone: the next transform starts from it again
    a.update_geometry(*data["exp"][2])
    a.update_transforms(data["mats"][1], data["exp"][1][1])
    b.update_geometry(*data["exp"][1])
    _exact_queries(_queries(a, rays), _queries(b, rays), "rest pose after update_geometry")
    a.close()
    b.close()


# ------------------------------------------------------------------ 3. identity, there and back
def test_identity_and_there_and_back(data, rays, cam):
    cfg, scene = data["cfg"], data["scene"]
    dyn = _context(cfg, _flat(scene), transforms=True)
    ref = _state(dyn, rays, cam)
    assert np.array_equal(_bits(data["mats"][0]), _bits(X.identity(3)))
    dyn.update_transforms(X.identity(3), scene["spheres"])
    _exact_state(_state(dyn, rays, cam), ref, f"{data['tag']}: identity matrices vs the upload")
    dyn.update_transforms(data["mats"][2], data["exp"][2][1])
    assert not np.array_equal(_bits(dyn.intersect(rays)[2]), _bits(ref[0][0][2]))
    dyn.update_transforms(X.identity(3), scene["spheres"])
    _exact_state(_state(dyn, rays, cam), ref, f"{data['tag']}: k=2 and back to the identity")
    dyn.close()


# ------------------------------------------------------------------ 4. object-space rest pose + instance matrices
def test_rest_positions_with_instance_matrices(data, rays):
    """The caller's use: upload the flattening, set the object-space vertices as the rest pose, send the instances'
    matrices.  Object space: each copy's vertices relative to its own centre; instance matrix of step k:
    M_k(g) T(c_g), composed in float64.  The flattening is transform_common.transform_point's, which equals the host
    layer's Flatten bit for bit (tests/test_transform_cpu.py)."""
    cfg, scene = data["cfg"], data["scene"]
    shifts = cfg[5]
    first, idx = scene["tri_geom_first"], scene["indices"]
    obj = scene["positions"].copy()
    inst = {k: np.zeros((3, 4, 4), np.float32) for k in (0, 1, 2)}
    for g, dx in enumerate(shifts):
        c = X.CENTRE + np.array([dx, 0.0, 0.0])
        v = np.unique(idx[first[g]:first[g + 1]])
        obj[v] = (obj[v].astype(np.float64) - c).astype(np.float32)
        T = np.eye(4)
        T[:3, 3] = c
        for k in inst:
            inst[k][g] = (data["mats"][k][g].astype(np.float64).T @ T).T.astype(np.float32)
    flatten = {k: X.transform_geometries(scene, inst[k], rest=obj) for k in inst}
    dyn = _context(cfg, _flat(scene, flatten[0]), transforms=True)
    upload = _queries(dyn, rays)
    dyn.set_rest_positions(obj)
    _exact_queries(_queries(dyn, rays), upload, "set_rest_positions alone changes nothing")
    for k in (1, 2):
        sph = data["exp"][k][1]
        dyn.update_transforms(inst[k], sph)
        fresh = _context(cfg, _flat(scene, flatten[k], sph))
        _same_queries(_queries(dyn, rays), _queries(fresh, rays), f"{data['tag']} k={k} rest pose + instance matrices vs Flatten")
        fresh.close()
    # the step-0 matrices give the uploaded flattening back, bit for bit
    dyn.update_transforms(inst[0], scene["spheres"])
    _exact_queries(_queries(dyn, rays), upload, "instance matrices of step 0")
    # through a device pointer too
    t = torch.from_numpy(obj).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    dyn.set_rest_positions(t, device=True)
    dyn.update_transforms(inst[0])
    _exact_queries(_queries(dyn, rays), upload, "rest pose by device pointer")
    with pytest.raises(sptr.SptrError, match=INVALID):
        dyn.set_rest_positions(obj[:-1])
    dyn.close()


# ------------------------------------------------------------------ 5. other paths
def test_lanes_and_launch_modes_see_the_transform(data, cam):
    cfg, scene = data["cfg"], data["scene"]
    pos, sph = data["exp"][1]
    ref = None
    variants = [("launch mode 0", 0, 0), ("launch mode 3", 3, 0)]
    if cfg[4] == 0:  # LDS-staged: the second pixel lane holds a copy of the scene, refitted from the same rest pose
        variants += [("one lane", 0, 1), ("two lanes", 0, 2)]
    for what, mode, lanes in variants:
        dyn = _context(cfg, _flat(scene), transforms=True)
        dyn.set_launch_mode(mode)
        dyn.set_pixel_lanes(lanes)
        for _ in range(3):  # the shape repeated: a stale captured graph or cull mask would show after the update
            still = _render(dyn, cam)
        dyn.update_transforms(data["mats"][1], sph)
        for _ in range(3):
            img = _render(dyn, cam)
        if lanes:
            assert dyn.pixel_lanes_info()["active"] == (lanes == 2)
        if mode == 3:
            assert dyn.graph_info()["captures"] >= 2
        assert float((img[1] == still[1]).all(axis=2).mean()) < 0.999  # (the image did change)
        if ref is None:
            plain = _context(cfg, _flat(scene), dynamic=True)
            plain.update_geometry(pos, sph)
            ref = _render(plain, cam)
            plain.close()
        assert np.array_equal(_bits(img[0]), _bits(ref[0])) and np.array_equal(img[1], ref[1]), f"{data['tag']} {what}"
        dyn.close()


def test_partial_calls_and_device_pointers(data, rays):
    cfg, scene = data["cfg"], data["scene"]
    pos, sph = data["exp"][1]
    a = _context(cfg, _flat(scene), transforms=True)
    b = _context(cfg, _flat(scene), dynamic=True)
    a.update_transforms(xforms=data["mats"][1])  # triangles only
    b.update_geometry(positions=pos)
    _exact_queries(_queries(a, rays), _queries(b, rays), f"{data['tag']} matrices only")
    a.update_transforms(spheres=sph)  # spheres only: the triangles keep their records
    b.update_geometry(spheres=sph)
    host = _queries(a, rays)
    _exact_queries(host, _queries(b, rays), f"{data['tag']} then spheres only")
    info = a.refit_info()
    assert info["refits"] == 2 and info["ms_wall"] > 0.0 and info["ms_device"] > 0.0
    b.close()
    a.update_transforms(X.identity(3), scene["spheres"])
    tm = torch.from_numpy(data["mats"][1].copy()).to("cuda:0").contiguous()
    ts = torch.from_numpy(sph.copy()).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    a.update_transforms(tm, ts, device=True)
    _exact_queries(_queries(a, rays), host, f"{data['tag']} device pointers")
    assert a.refit_info()["refits"] == 4
    a.close()


def test_errors():
    lds, wide = X.SCENES
    b = sptr.builtin_scene(lds[1])
    scene = X.compose({"positions": b.positions, "indices": b.indices, "tri_geom_first": b.tri_geom_first,
                       "spheres": b.spheres, "geom_material": b.geom_material}, lds[5])
    eye, sph = X.identity(3), scene["spheres"]
    r = sptr.Renderer(0)
    for call in (lambda: r.update_transforms(eye, sph), lambda: r.set_rest_positions(scene["positions"]), lambda: r.tree_cost()):
        with pytest.raises(sptr.SptrError, match=NO_SCENE):
            call()
    r.close()
    dyn = _context(lds, _flat(scene), transforms=True)
    bad = eye.copy()
    bad[1, 3, 0] = np.nan
    inf = eye.copy()
    inf[2, 0, 0] = np.inf
    for what, call in (("matrix count", lambda: dyn.update_transforms(eye[:2], sph)),
                       ("sphere count", lambda: dyn.update_transforms(eye, sph[:-1])),
                       ("both NULL", lambda: dyn.update_transforms(None, None)),
                       ("NaN entry", lambda: dyn.update_transforms(bad, sph)),
                       ("infinite entry", lambda: dyn.update_transforms(inf)),
                       ("rest count", lambda: dyn.set_rest_positions(scene["positions"][:-1]))):
        with pytest.raises(sptr.SptrError, match=INVALID):
            call()
    for flags in (2, 0x80000000):  # unknown flags, through the C ABI
        h = np.ascontiguousarray(eye)
        assert dyn._L.sptr_update_transforms(dyn._h, h.ctypes.data, 3, None, 0, flags) == -1
        p = np.ascontiguousarray(scene["positions"])
        assert dyn._L.sptr_set_rest_positions(dyn._h, p.ctypes.data, len(p), flags) == -1
    assert dyn.refit_info()["refits"] == 0  # (no refused call refitted anything)
    nan_row3 = eye.copy()
    nan_row3[:, :, 3] = 7.0  # row 3 is ignored
    before = dyn.intersect(R.rays(sptr.camera_lookat(aspect=W / H).as_array())[:512])
    dyn.update_transforms(nan_row3)
    after = dyn.intersect(R.rays(sptr.camera_lookat(aspect=W / H).as_array())[:512])
    for x, y in zip(before, after):
        assert np.array_equal(_bits(x), _bits(y))
    dyn.close()
    # split references are neither refitted nor transformed
    m = sptr.builtin_scene(wide[1], wide[2], wide[3])
    mesh = X.compose({"positions": m.positions, "indices": m.indices, "tri_geom_first": m.tri_geom_first,
                      "spheres": m.spheres, "geom_material": m.geom_material}, wide[5])
    split = _context(wide, _flat(mesh), transforms=True, split_refs=4)
    lay = split.scene_layout()
    assert lay["num_prim_refs"] > lay["num_tris"] + lay["num_spheres"]
    with pytest.raises(sptr.SptrError, match=INVALID):
        split.update_transforms(eye, mesh["spheres"])
    with pytest.raises(sptr.SptrError, match=INVALID):
        split.set_rest_positions(mesh["positions"])
    assert split.tree_cost()["cost"] > 0.0  # (the figure itself needs no dynamic upload)
    split.close()


def test_plain_dynamic_upload_refuses_transforms_and_still_refits(data, rays):
    cfg, scene = data["cfg"], data["scene"]
    pos, sph = data["exp"][1]
    plain = _context(cfg, _flat(scene), dynamic=True)
    with pytest.raises(sptr.SptrError, match=INVALID):
        plain.update_transforms(data["mats"][1], sph)
    with pytest.raises(sptr.SptrError, match=INVALID):
        plain.set_rest_positions(scene["positions"])
    tc = plain.tree_cost()
    assert tc["cost_at_upload"] == 0.0 and tc["root_area_at_upload"] == 0.0 and tc["cost"] > 0.0 and tc["root_area"] > 0.0
    plain.update_geometry(pos, sph)
    fresh = _context(cfg, _flat(scene, pos, sph))
    _same_queries(_queries(plain, rays), _queries(fresh, rays), f"{data['tag']} set_dynamic(1): refit as before")
    assert plain.refit_info()["refits"] == 1
    fresh.close()
    # the bit is read by the next upload, and cleared by the one after
    plain.set_dynamic(True, transforms=True)
    plain.upload_scene(_flat(scene))
    plain.update_transforms(data["mats"][1], sph)
    plain.set_dynamic(True)
    plain.upload_scene(_flat(scene))
    with pytest.raises(sptr.SptrError, match=INVALID):
        plain.update_transforms(data["mats"][1], sph)
    plain.close()


# ------------------------------------------------------------------ 6. motion vectors
def test_motion_vectors_follow_a_transform(data, cam):
    """render, update, render with the denoiser, its history and the motion path on: once through
    update_geometry(expected positions), once through update_transforms, the scene uploaded again in between.  The
    history snapshots triangle records, so the two must give the same bits.  Two pixel lanes on the LDS scene."""
    cfg, scene = data["cfg"], data["scene"]
    pos, sph = data["exp"][1]
    r = sptr.Renderer(0)
    r.set_bvh_width(cfg[4])
    r.set_dynamic(True, transforms=True)
    out = []
    for path in ("geometry", "transforms"):
        r.upload_scene(_flat(scene))
        r.set_materials(sptr.preset_materials(with_light=(cfg[1] == "default_emitter")))
        r.set_lights(sptr.default_lights())
        r.set_environment(None)
        r.set_pixel_lanes(2 if cfg[4] == 0 else 0)
        r.set_denoise(3)
        r.set_denoise_history(4)
        r.set_history_motion(True)
        r.render(cam, W, H, spp=1)
        if path == "geometry":
            r.update_geometry(pos, sph)
        else:
            r.update_transforms(data["mats"][1], sph)
        r.set_seed_offset(1)
        r.render(cam, W, H, spp=1)
        info, minfo = r.history_info(), r.motion_info()
        assert info["carried"] and info["reprojected"] > 0 and minfo["used"] and minfo["snapshots"] == 1
        if cfg[4] == 0:
            assert r.pixel_lanes_info()["active"]
        out.append((r.read_history(), r.read_motion(), r.read_denoised(), info["reprojected"]))
        r.set_seed_offset(0)
        r.set_history_motion(False)
    r.close()
    g, t = out
    print(f"{data['tag']}: {g[3]} pixels took history through update_geometry, {t[3]} through update_transforms")
    for x, y in zip(g[:3], t[:3]):
        assert np.array_equal(_bits(x), _bits(y))
    assert g[3] == t[3]
    assert np.isfinite(g[1]).any()


# ------------------------------------------------------------------ 7. the tree cost
def test_tree_cost(data):
    cfg, scene = data["cfg"], data["scene"]
    dyn = _context(cfg, _flat(scene), transforms=True)
    up = dyn.tree_cost()
    print(f"{data['tag']}: tree cost {up}")
    assert up["cost"] > 0.0 and up["root_area"] > 0.0
    assert up["cost"] == up["cost_at_upload"] and up["root_area"] == up["root_area_at_upload"]  # right after the upload
    assert dyn.tree_cost() == up  # the same tree, the same bits
    dyn.update_transforms(data["mats"][2], data["exp"][2][1])
    moved = dyn.tree_cost()
    assert moved["cost"] != up["cost"] and moved["cost_at_upload"] == up["cost"]
    dyn.update_transforms(X.identity(3), scene["spheres"])
    assert dyn.tree_cost() == up  # there and back
    # the whole scene scaled by exactly 2 about the origin: every extent doubles exactly, every area is 4 times
    two = np.tile(np.diag(np.array([2.0, 2.0, 2.0, 1.0], np.float32)), (3, 1, 1))
    dyn.update_transforms(two, scene["spheres"] * np.float32(2.0))
    big = dyn.tree_cost()
    assert big["cost"] == 4.0 * up["cost"] and big["root_area"] == 4.0 * up["root_area"]
    # the three geometries moved apart: some counted box holds two of them and grows
    apart = X.identity(3).copy()
    for g in range(3):
        apart[g, 3, :3] = 40.0 * np.array([np.cos(2.0 * np.pi * g / 3.0), 0.0, np.sin(2.0 * np.pi * g / 3.0)])
    dyn.update_transforms(apart, scene["spheres"])
    far = dyn.tree_cost()
    print(f"{data['tag']}: geometries moved apart by 40: cost ratio {far['cost'] / up['cost']:.3f}, "
          f"root area ratio {far['root_area'] / up['root_area']:.3f}")
    assert far["cost"] > 1.01 * up["cost"]
    dyn.close()


# ------------------------------------------------------------------ 8. the upper layers
def test_cli_animate_rigid(tmp_path):
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"

    def run(*extra):
        res = subprocess.run([exe, "--scene", "default_emitter", "--w", str(W), "--h", str(H), "--spp", "2", "--animate", "3",
                              "--json", "--out", str(tmp_path / "a.ppm"), *extra], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        return json.loads(res.stdout.strip().splitlines()[-1])

    rigid, plain = run("--rigid"), run()
    print({k: rigid[k] for k in ("refits", "transform_updates", "tree_cost", "tree_cost_at_build", "root_area", "ms_refit_wall")})
    assert rigid["rigid"] == 1 and rigid["refits"] == 2 and rigid["transform_updates"] == 2
    assert rigid["tree_cost"] > 0.0 and rigid["tree_cost_at_build"] > 0.0 and rigid["root_area_at_build"] > 0.0
    assert rigid["tree_cost"] != rigid["tree_cost_at_build"]  # (the instances and the spheres did move)
    assert plain["rigid"] == 0 and plain["refits"] == 2 and plain["transform_updates"] == 0
    assert plain["tree_cost"] > 0.0 and plain["tree_cost_at_build"] == 0.0
