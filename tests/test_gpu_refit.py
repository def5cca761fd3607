"""GPU tests of dynamic scenes: sptr_set_dynamic, sptr_update_geometry (the in-place BVH refit,
kernels_refit.hip) and sptr_refit_info.

Scenes, deformation, rays and the comparison rule are tests/refit_common.py's (checked on the CPU oracle by
tests/test_refit_cpu.py).  Every test creates its own contexts: one uploaded dynamic and refitted, and fresh
ones that upload the moved scene.  The expected difference is none: the refit recomputes the triangle
records and re-quantises the wide nodes with the build's own device functions, so only the tree topology
(the upload's, not the moved scene's) differs from a fresh build, and topology does not change a closest
hit unless two primitives lie at one distance.

Images are compared by the project's criteria (>= 99.9 % identical RGB8 pixels, relative L1 <= 1e-3 on the
accumulation); where the two contexts hold the same tree (there and back, dynamic against non-dynamic)
byte-identical images and equal traversal counters are required: the counters only agree if every box,
BVH2 and quantised, is the same bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import refit_common as R
import sptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = R.W, R.H
INVALID, NO_SCENE = "rc=-1:", "rc=-3:"


def _flat(cfg, k=0):
    name, p0, p1, _ = cfg
    s = sptr.builtin_scene(name, p0, p1)
    s.positions, s.spheres = R.deform(s.positions, s.spheres, k)
    return s


def _context(cfg, flat, dynamic, split_refs=0):
    name, _, _, width = cfg
    r = sptr.Renderer(0)
    r.set_bvh_width(width)
    if split_refs:
        r.set_split_refs(split_refs)
    r.set_dynamic(dynamic)
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


def _queries(r, rays):
    return r.intersect(rays), r.occluded(rays)


def _same_queries(a, b, what):
    R.compare_hits(a[0], b[0], what)
    R.compare_occluded(a[1], b[1], what)


def _exact_queries(a, b):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(a[1], b[1])


def _render(r, cam, **kw):
    st = r.render(cam, W, H, spp=4, **kw)
    return r.read_accum(), r.read_rgb8(), st


def _same_image(a, b, what):
    same = float((a[1] == b[1]).all(axis=2).mean())
    rel = float(np.abs(a[0] - b[0]).sum() / max(1e-12, np.abs(b[0]).sum()))
    print(f"{what}: identical RGB8 pixels {same:.5f}, relative L1 of the accumulation {rel:.2e}")
    assert same >= 0.999 and rel <= 1e-3


@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_refit_equals_fresh_build(cfg, rays):
    base = _flat(cfg)
    dyn = _context(cfg, base, True)
    before = dyn.intersect(rays)
    for k in (1, 2):  # 2 on top of 1: the second refit starts from refitted boxes
        moved = _flat(cfg, k)
        dyn.update_geometry(moved.positions, moved.spheres)
        fresh = _context(cfg, moved, False)
        got = _queries(dyn, rays)
        _same_queries(got, _queries(fresh, rays), f"{cfg[0]} k={k} refit vs fresh build")
        fresh.close()
        changed = (got[0][0] != before[0]) | (got[0][1] != before[1]) | (got[0][2].view(np.uint32) != before[2].view(np.uint32))
        assert changed.mean() >= 0.2  # (the deformation matters: tests/test_refit_cpu.py)
    assert dyn.refit_info()["refits"] == 2
    dyn.close()


@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_there_and_back(cfg, rays, cam):
    base = _flat(cfg)
    plain = _context(cfg, base, False)
    dyn = _context(cfg, base, True)
    ref_q = _queries(plain, rays)
    ref_img = _render(plain, cam)
    ref_cnt = _render(plain, cam, flags=sptr.SPTR_FRAME_COUNT_VISITS)[2]
    counters = ("node_visits", "tri_tests", "sphere_tests", "shadow_node_visits")
    assert ref_cnt.node_visits > 0 and ref_cnt.shadow_node_visits > 0

    def check(what):
        _exact_queries(_queries(dyn, rays), ref_q)
        img = _render(dyn, cam)
        assert np.array_equal(img[0].view(np.uint32), ref_img[0].view(np.uint32)), what
        assert np.array_equal(img[1], ref_img[1]), what
        cnt = _render(dyn, cam, flags=sptr.SPTR_FRAME_COUNT_VISITS)[2]
        print(what, {k: (getattr(cnt, k), getattr(ref_cnt, k)) for k in counters})
        for k in counters:
            assert getattr(cnt, k) == getattr(ref_cnt, k), (what, k)

    check(f"{cfg[0]}: dynamic upload vs ordinary upload")
    assert dyn.scene_layout() == plain.scene_layout() and dyn.scene_info()["depth"] == plain.scene_info()["depth"]
    moved = _flat(cfg, 2)
    dyn.update_geometry(moved.positions, moved.spheres)
    assert not np.array_equal(dyn.intersect(rays)[2].view(np.uint32), ref_q[0][2].view(np.uint32))
    dyn.update_geometry(base.positions, base.spheres)
    check(f"{cfg[0]}: deformed and back")
    plain.close()
    dyn.close()


@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_render_after_refit(cfg, cam):
    moved = _flat(cfg, 1)
    fresh = _context(cfg, moved, False)
    ref = _render(fresh, cam)
    dyn = _context(cfg, _flat(cfg), True)
    still = _render(dyn, cam)
    dyn.update_geometry(moved.positions, moved.spheres)
    img = _render(dyn, cam)
    _same_image(img, ref, f"{cfg[0]} k=1 render after refit vs fresh build")
    assert float((img[1] == still[1]).all(axis=2).mean()) < 0.999  # (the image did change)
    if cfg[3] == 0:  # LDS-staged: the second pixel lane holds a copy of the scene, refitted too
        fresh.set_pixel_lanes(2)
        ref2 = _render(fresh, cam)
        assert fresh.pixel_lanes_info()["active"]
        lanes = _context(cfg, _flat(cfg), True)
        lanes.set_pixel_lanes(2)
        _render(lanes, cam)
        assert lanes.pixel_lanes_info()["active"]
        lanes.update_geometry(moved.positions, moved.spheres)
        _same_image(_render(lanes, cam), ref2, f"{cfg[0]} k=1 two pixel lanes after refit vs fresh build")
        assert lanes.pixel_lanes_info()["active"]
        lanes.close()
    fresh.close()
    dyn.close()


@pytest.mark.parametrize("mode", (0, 3))
@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_launch_modes_see_the_refit(cfg, mode, cam):
    """The shape three times, an update, three times again: a stale captured graph or cull mask shows."""
    moved = _flat(cfg, 1)
    fresh = _context(cfg, moved, False)
    fresh.set_launch_mode(mode)
    ref = None
    for _ in range(3):
        ref = _render(fresh, cam)
    dyn = _context(cfg, _flat(cfg), True)
    dyn.set_launch_mode(mode)
    for _ in range(3):
        _render(dyn, cam)
    dyn.update_geometry(moved.positions, moved.spheres)
    for i in range(3):
        _same_image(_render(dyn, cam), ref, f"{cfg[0]} launch mode {mode} call {i} after the update")
    if mode == 3:
        assert dyn.graph_info()["captures"] >= 2  # one graph before the update, another after
    fresh.close()
    dyn.close()


def test_denoiser_recomputes_aovs_after_update(cam):
    cfg = R.SCENES[0]
    dyn = _context(cfg, _flat(cfg), True)
    dyn.set_denoise(2)
    dyn.render(cam, W, H, spp=1)
    dyn.render(cam, W, H, spp=1, frame_begin=2)
    assert dyn.denoise_info()["aov_passes"] == 1  # a still camera: cached
    moved = _flat(cfg, 1)
    dyn.update_geometry(moved.positions, moved.spheres)
    dyn.render(cam, W, H, spp=1)
    assert dyn.denoise_info()["aov_passes"] == 2
    fresh = _context(cfg, moved, False)
    fresh.set_denoise(2)
    fresh.render(cam, W, H, spp=1)
    assert np.array_equal(dyn.read_aov(sptr.SPTR_AOV_ID), fresh.read_aov(sptr.SPTR_AOV_ID))
    fresh.close()
    dyn.close()


@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_partial_updates_and_device_pointers(cfg, rays):
    base, moved = _flat(cfg), _flat(cfg, 1)
    dyn = _context(cfg, base, True)
    dyn.update_geometry(positions=moved.positions)
    half = sptr.FlatScene(moved.positions, base.indices, base.tri_geom_first, base.spheres, base.geom_material)
    fresh = _context(cfg, half, False)
    _same_queries(_queries(dyn, rays), _queries(fresh, rays), f"{cfg[0]} positions only")
    fresh.close()
    dyn.update_geometry(spheres=moved.spheres)
    fresh = _context(cfg, moved, False)
    host_path = _queries(dyn, rays)
    _same_queries(host_path, _queries(fresh, rays), f"{cfg[0]} then spheres only")
    fresh.close()
    info = dyn.refit_info()
    assert info["refits"] == 2 and info["ms_wall"] > 0.0 and info["ms_device"] > 0.0
    dyn.close()
    # the same update in one call through device pointers
    dev = _context(cfg, base, True)
    tp = torch.from_numpy(moved.positions).to("cuda:0").contiguous()
    ts = torch.from_numpy(moved.spheres).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    dev.update_geometry(tp, ts, device=True)
    _exact_queries(_queries(dev, rays), host_path)
    assert dev.refit_info()["refits"] == 1
    dev.close()


def test_errors_and_refit_info():
    lds, mesh = R.SCENES
    moved = _flat(lds, 1)
    r = sptr.Renderer(0)
    with pytest.raises(sptr.SptrError, match=NO_SCENE):
        r.update_geometry(moved.positions, moved.spheres)
    r.close()
    plain = _context(lds, _flat(lds), False)
    with pytest.raises(sptr.SptrError, match=INVALID):
        plain.update_geometry(moved.positions, moved.spheres)
    assert plain.refit_info()["refits"] == 0
    plain.close()
    dyn = _context(lds, _flat(lds), True)
    with pytest.raises(sptr.SptrError, match=INVALID):
        dyn.update_geometry(moved.positions[:-1], moved.spheres)
    with pytest.raises(sptr.SptrError, match=INVALID):
        dyn.update_geometry(moved.positions, moved.spheres[:-1])
    with pytest.raises(sptr.SptrError, match=INVALID):
        dyn.update_geometry(None, None)
    assert dyn.refit_info() == {"refits": 0, "ms_wall": 0.0, "ms_device": 0.0, "excluded_prims": 0}
    dyn.update_geometry(moved.positions, moved.spheres)
    assert dyn.refit_info()["refits"] == 1
    dyn.upload_scene(_flat(lds))  # an upload starts the count again
    assert dyn.refit_info()["refits"] == 0
    dyn.set_dynamic(False)
    dyn.upload_scene(_flat(lds))
    with pytest.raises(sptr.SptrError, match=INVALID):
        dyn.update_geometry(moved.positions, moved.spheres)
    dyn.close()
    # split references are not refitted
    base = _flat(mesh)
    split = _context(mesh, base, True, split_refs=4)
    lay = split.scene_layout()
    assert lay["num_prim_refs"] > lay["num_tris"] + lay["num_spheres"]
    with pytest.raises(sptr.SptrError, match=INVALID):
        split.update_geometry(base.positions, base.spheres)
    split.close()
    # triangles exactly degenerate at upload stay out of the tree: the mesh's pole rings
    dyn = _context(mesh, base, True)
    info, scene = dyn.refit_info(), dyn.scene_info()
    print("sphere mesh: excluded_prims", info["excluded_prims"], scene)
    assert info["excluded_prims"] == scene["prims"] - (scene["nodes"] + 1) and info["excluded_prims"] > 0
    m2 = _flat(mesh, 2)
    dyn.update_geometry(m2.positions, m2.spheres)
    assert dyn.refit_info()["excluded_prims"] == info["excluded_prims"]
    dyn.close()


def _ppm(path):
    with open(path, "rb") as f:
        parts = f.read().split(b"\n", 3)
    return np.frombuffer(parts[3], np.uint8).reshape(H, W, 3)


def test_cli_animate(tmp_path):
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"
    base = [exe, "--scene", "default_emitter", "--w", str(W), "--h", str(H), "--spp", "2", "--json"]
    out, info = {}, {}
    for tag, extra in (("refit", []), ("rebuild", ["--rebuild"]), ("still", [])):
        out[tag] = tmp_path / f"{tag}.ppm"
        args = base + ["--out", str(out[tag])] + (["--animate", "4"] + extra if tag != "still" else [])
        res = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        info[tag] = json.loads(res.stdout.strip().splitlines()[-1])
    print({k: {f: v[f] for f in ("refits", "ms_refit_wall", "ms_refit_device", "ms_build")} for k, v in info.items()})
    assert info["refit"]["refits"] == 3 and info["rebuild"]["refits"] == 0 and info["still"]["refits"] == 0
    assert info["refit"]["ms_refit_wall"] > 0.0 and info["refit"]["ms_refit_device"] > 0.0 and info["refit"]["ms_build"] == 0.0
    assert info["rebuild"]["ms_build"] > 0.0 and info["rebuild"]["ms_refit_wall"] == 0.0
    a, b = _ppm(out["refit"]), _ppm(out["rebuild"])
    same = float((a == b).all(axis=2).mean())
    print(f"sptr_cli --animate 4: refit vs rebuild, identical pixels {same:.5f}")
    assert same >= 0.999
    assert float((a == _ppm(out["still"])).all(axis=2).mean()) < 0.999  # (the spheres did move)
    # refits are not tied to the wavefront path
    res = subprocess.run(base + ["--out", str(tmp_path / "pt.ppm"), "--animate", "2", "--integrator", "pathtracer"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1])["refits"] == 1
