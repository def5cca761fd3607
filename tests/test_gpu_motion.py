"""GPU tests of the motion vectors (sptr_set_history_motion, sptr_read_motion, sptr_motion_info, SPTR_AOV_UV):
DESIGN.md §6h.

Configurations as tests/test_gpu_refit.py: 150x82 (ragged 32x8 blocks and 32x32 tiles on both edges) of
default_emitter (12 triangles and 9 spheres, the BVH2 staged in LDS) and of the 30x70 sphere mesh with
set_bvh_width(4) (the wide walk from L2), each uploaded after set_dynamic(True).  Geometry k is
refit_common.deform(positions, spheres, 0.3 k): the steps whose inputs tests/test_motion_cpu.py checks on the CPU.

A pass that reads its carry through a snapshot is compared bit for bit with the numpy restatement
(tests/motion_ref.py) fed the GPU's own accumulation, AOV planes (the barycentric plane among them) and carried
history, and the coordinates the test itself handed to update_geometry; a pass that does not is
tests/temporal_ref.py's.  Zero differing pixels are required."""
import json
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import motion_ref as M
import refit_common as R
import sptr
import temporal_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = R.W, R.H
ITER = 3
MAX_HISTORY = 4
STEP = 0.3
FLOOR_TAKEN = 0.9  # of the hit pixels take history on the last step (tests/test_motion_cpu.py, on the oracle)
TARGET = (0.0, 1.0, 0.0)
POSITIONS = [(0.0, 3.0, 8.0), (0.41869, 3.0, 7.98904)]  # the default camera and one 3 degrees on its orbit


def _reset(r):
    r.set_history_motion(False)
    r.set_seed_offset(0)
    r.set_denoise_history(0)
    r.set_denoise(0)
    r.set_pixel_lanes(0)
    r.set_launch_mode(0)
    r.set_bvh_width(0)
    r.set_dynamic(False)


@pytest.fixture(scope="module", params=R.SCENES, ids=R.SCENE_IDS)
def cfg(request, renderer):
    name, p0, p1, width = request.param
    _reset(renderer)
    renderer.set_bvh_width(width)
    renderer.set_dynamic(True)
    flat = sptr.setup_default(renderer, name, p0, p1)
    cams = [sptr.camera_lookat(pos=p, target=TARGET, aspect=W / H) for p in POSITIONS]
    renderer.render(cams[0], W, H, spp=4)  # the wave buffers at their largest size of this module (a growth drops the history)
    geo = [R.deform(flat.positions, flat.spheres, STEP * k) for k in range(4)]
    for g in geo:
        for a in g:
            a.setflags(write=False)
    yield {"name": name, "flat": flat, "cams": cams, "geo": geo, "topo": (flat.indices, flat.tri_geom_first),
           "lds": width == 0, "tri_geoms": len(flat.tri_geom_first) - 1}
    _reset(renderer)
    sptr.setup_default(renderer, "default")  # (the session's renderer holds a scene uploaded without set_dynamic again)


def _begin(r, cfg, motion=True):
    """Geometry 0, the denoiser and the history on, nothing carried."""
    r.set_history_motion(False)
    r.update_geometry(*cfg["geo"][0])
    r.set_denoise(ITER)
    r.set_denoise_history(MAX_HISTORY)
    r.set_history_motion(motion)
    r.set_seed_offset(0)


def _end(r):
    r.set_history_motion(False)
    r.set_denoise_history(0)
    r.set_denoise(0)
    r.set_seed_offset(0)


def _read_aovs(r):
    nz = np.concatenate([r.read_aov(sptr.SPTR_AOV_NORMAL), r.read_aov(sptr.SPTR_AOV_DEPTH)[..., None]], axis=-1)
    return nz, r.read_aov(sptr.SPTR_AOV_ALBEDO), r.read_aov(sptr.SPTR_AOV_ID)


def _state(r):
    nz, albedo, ids = _read_aovs(r)
    s = {"acc": r.read_accum(), "nz": nz, "albedo": albedo, "ids": ids, "uv": r.read_aov(sptr.SPTR_AOV_UV),
         "den": r.read_denoised(), "hist": r.read_history(), "info": r.history_info(), "minfo": r.motion_info()}
    s["motion"] = r.read_motion() if s["minfo"]["used"] else None
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _differing(a, b):
    """Finite pixels of b that differ from a in any bit (the non-finite ones must be non-finite in both)."""
    fin = np.isfinite(b).all(axis=-1)
    assert np.array_equal(fin, np.isfinite(a).all(axis=-1))
    return int((_bits(a)[fin] != _bits(b)[fin]).any(axis=-1).sum()), int(fin.sum())


def _same_motion(got, want):
    """Bit-equal where the restatement is a number, NaN exactly where it is NaN."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _sequence(r, cfg, plan, check=True):
    """plan: per pass (updates, camera index); updates: (positions or None, spheres or None) pairs handed to
    update_geometry before the pass.  Every pass restarts the accumulation with one frame, seeded with offset i,
    so each is the next one's carry.  Every pass is compared with
    the restatement of the path it must take: through the geometry its carry saw when the geometry changed
    since, tests/temporal_ref.py's otherwise.  Returns the passes' states."""
    cur = cfg["geo"][0]
    carry, seen, out = None, None, []
    for i, (updates, ci) in enumerate(plan):
        for pos, sph in updates:
            r.update_geometry(pos, sph)
            cur = (cur[0] if pos is None else pos, cur[1] if sph is None else sph)
        cam = cfg["cams"][ci]
        r.set_seed_offset(i)
        r.render(cam, W, H, spp=1)
        s = _state(r)
        out.append(s)
        moved = carry is not None and (seen[0] is not cur[0] or seen[1] is not cur[1])
        if check:
            ca = cam.as_array()
            if moved:
                den, hist, cnt, motion = M.denoise(s["acc"], 1, s["nz"], s["albedo"], s["ids"], s["uv"], ca, carry, MAX_HISTORY,
                                                   ITER, cfg["topo"], seen, cur)
            else:
                den, hist, cnt = T.denoise(s["acc"], 1, s["nz"], s["albedo"], s["ids"], ca, carry, MAX_HISTORY, ITER)
            bad_h, fin = _differing(s["hist"], hist)
            bad_d, _ = _differing(s["den"], den)
            hits = int((s["nz"][..., 3] >= 0).sum())
            print(f"{cfg['name']} pass {i}: history {bad_h}, filtered {bad_d} of {fin} finite pixels differ from the restatement; "
                  f"{s['info']['reprojected']} of {hits} hits took history (restatement {cnt}), motion path {s['minfo']['used']}, "
                  f"{s['info']['ms_reproject']:.4f} ms")
            assert bad_h == 0 and bad_d == 0
            assert s["info"]["reprojected"] == cnt and s["info"]["carried"] == (carry is not None)
            assert s["minfo"]["used"] == moved
            if moved:
                assert _same_motion(s["motion"], motion)
                assert np.isnan(s["motion"][s["nz"][..., 3] < 0]).all()
        carry = {"hist": s["hist"], "nz": s["nz"], "ids": s["ids"], "cam": cam.as_array()}
        seen = cur
    return out


def _plan_of_steps(cfg):
    """Move, then restart: steps 1 and 2 under the standing camera, step 3 seen from the other one."""
    g = cfg["geo"]
    return [([], 0), ([g[1]], 0), ([g[2]], 0), ([g[3]], 1)]


# ---------------------------------------------------------------------------------------- 1. the barycentric plane
def test_aov_uv_equals_query_rays(cfg, renderer):
    r = renderer
    _begin(r, cfg, motion=False)
    r.set_denoise(0)
    r.update_geometry(*cfg["geo"][1])
    cam = cfg["cams"][0]
    r.render(cam, W, H, spp=1)
    nz, albedo, ids = _read_aovs(r)
    passes = r.denoise_info()["aov_passes"]
    uv = r.read_aov(sptr.SPTR_AOV_UV)
    assert uv.shape == (H, W, 2) and uv.dtype == np.float32
    assert r.denoise_info()["aov_passes"] == passes + 1  # the cached planes lacked it: computed again
    q = r.query_rays(D.pixel_centre_rays(cam.as_array(), W, H))
    assert np.array_equal(_bits(uv), _bits(q["uv"].reshape(H, W, 2)))
    assert np.array_equal(ids[..., 0], q["geom"].reshape(H, W))
    tri = ids[..., 0] < cfg["tri_geoms"]
    assert tri.sum() > 100 and (~tri & (ids[..., 0] != D.MISS)).sum() > 0  # (both kinds are in view)
    assert (uv[tri] != 0).any() and (_bits(uv)[~tri] == 0).all()  # a sphere hit or a miss: 0, 0
    again = _read_aovs(r)
    for a, b in zip((nz, albedo, ids), again):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(r.read_aov(sptr.SPTR_AOV_UV)), _bits(uv))
    assert r.denoise_info()["aov_passes"] == passes + 1  # (and now they are cached with it)
    _end(r)


# ---------------------------------------------------------------------------------------- 2. move, then restart
def test_moves_are_bit_equal_to_the_restatement(cfg, renderer):
    _begin(renderer, cfg)
    before = renderer.motion_info()["snapshots"]
    out = _sequence(renderer, cfg, _plan_of_steps(cfg))
    _end(renderer)
    last = out[-1]
    hits = int((last["nz"][..., 3] >= 0).sum())
    assert last["info"]["reprojected"] >= FLOOR_TAKEN * hits
    with np.errstate(invalid="ignore"):
        speed = np.sqrt((last["motion"].astype(np.float64) ** 2).sum(axis=-1))
    assert (speed > 0.5).sum() > 0.6 * hits  # (and the image did move)
    assert out[-1]["minfo"]["snapshots"] == before + 3


# ---------------------------------------------------------------------------------------- 3. two refits between passes
def test_two_refits_between_passes_keep_the_older_geometry(cfg, renderer):
    g = cfg["geo"]
    _begin(renderer, cfg)
    before = renderer.motion_info()["snapshots"]
    out = _sequence(renderer, cfg, [([], 0), ([g[1], g[2]], 0), ([g[3]], 0)])
    _end(renderer)
    assert out[1]["minfo"]["snapshots"] == before + 1  # the second refit kept the snapshot of geometry 0
    assert out[2]["minfo"]["snapshots"] == before + 2
    assert out[1]["info"]["reprojected"] > 0 and out[2]["info"]["reprojected"] > 0


# ---------------------------------------------------------------------------------------- 4. partial updates
def test_partial_updates(cfg, renderer):
    g = cfg["geo"]
    _begin(renderer, cfg)
    out = _sequence(renderer, cfg, [([], 0), ([(g[1][0], None)], 0), ([(None, g[2][1])], 0)])
    _end(renderer)
    assert all(s["minfo"]["used"] and s["info"]["reprojected"] > 0 for s in out[1:])


# ---------------------------------------------------------------------------------------- 5. off: as before
def test_motion_off_a_refit_still_drops_the_carry(cfg, renderer):
    r = renderer
    _begin(r, cfg, motion=False)
    cam = cfg["cams"][0]
    r.render(cam, W, H, spp=1)
    r.render(cam, W, H, spp=1)
    assert r.history_info()["carried"]
    r.update_geometry(*cfg["geo"][1])
    r.render(cam, W, H, spp=1)
    info = r.history_info()
    _end(r)
    assert not info["carried"] and info["reprojected"] == 0


# ---------------------------------------------------------------------------------------- 6. what still drops the carry
def test_the_carry_is_dropped_by_every_other_state_change(cfg, renderer):
    r = renderer
    a = cfg["cams"][0]
    g = cfg["geo"]
    name = cfg["name"]

    def after(between):
        _begin(r, cfg)
        r.render(a, W, H, spp=1)
        r.update_geometry(*g[1])
        between()
        r.render(a, W, H, spp=1)
        return r.history_info(), r.motion_info()

    info, minfo = after(lambda: None)
    assert info["carried"] and minfo["used"] and info["reprojected"] > 0  # (without any of them the carry is read)
    for what, between in (("upload", lambda: r.upload_scene(cfg["flat"])),
                          ("materials", lambda: r.set_materials(sptr.preset_materials(with_light=(name == "default_emitter")))),
                          ("size", lambda: r.render(a, 64, 48, spp=1)),
                          ("setter", lambda: r.set_history_motion(True))):
        info, minfo = after(between)
        print(f"{name}: after {what}: carried {info['carried']}, motion path {minfo['used']}")
        assert not info["carried"] and not minfo["used"] and info["reprojected"] == 0
        with pytest.raises(sptr.SptrError):
            r.read_motion()
    # a continuation after a refit: its carry (pass 0, geometry 0) has no snapshot any more (it holds geometry 1)
    _begin(r, cfg)
    r.render(a, W, H, spp=1)
    r.update_geometry(*g[1])
    r.render(a, W, H, spp=1)
    assert r.motion_info()["used"]
    r.update_geometry(*g[2])
    r.render(a, W, H, spp=1, frame_begin=2)
    info, minfo = r.history_info(), r.motion_info()
    _end(r)
    assert not info["carried"] and not minfo["used"] and info["reprojected"] == 0


# ---------------------------------------------------------------------------------------- 7. no refit: the static path
def test_motion_on_without_a_refit_is_the_static_path(cfg, renderer):
    _begin(renderer, cfg)
    before = renderer.motion_info()["snapshots"]
    out = _sequence(renderer, cfg, [([], 0), ([], 1), ([], 0)])
    _end(renderer)
    assert not any(s["minfo"]["used"] for s in out) and out[1]["info"]["reprojected"] > 0
    assert all(s["minfo"]["snapshots"] == before for s in out)


# ---------------------------------------------------------------------------------------- 8. invariance
def test_results_do_not_depend_on_how_the_call_is_launched(cfg, renderer):
    r = renderer

    def sequence():
        _begin(r, cfg)
        s = _sequence(r, cfg, _plan_of_steps(cfg), check=False)[-1]
        return s

    base = sequence()
    others = []
    for mode in (1, 3):
        r.set_launch_mode(mode)
        others.append(sequence())
    r.set_launch_mode(0)
    for lanes in (1, 2):
        r.set_pixel_lanes(lanes)
        others.append(sequence())
        assert r.pixel_lanes_info()["active"] == (lanes == 2 and cfg["lds"])
    r.set_pixel_lanes(0)
    _end(r)
    assert base["minfo"]["used"] and base["info"]["reprojected"] > 0
    for o in others:
        assert np.array_equal(_bits(o["hist"]), _bits(base["hist"])) and np.array_equal(_bits(o["den"]), _bits(base["den"]))
        assert np.array_equal(_bits(o["motion"]), _bits(base["motion"]))
        assert o["info"]["reprojected"] == base["info"]["reprojected"] and o["minfo"]["used"]


# ---------------------------------------------------------------------------------------- 9. errors
def test_errors_and_the_golden_image_afterwards():
    """On a context of its own, so that "before any motion pass" holds."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "c1_default_256_4spp.npz"), allow_pickle=False)
    r = sptr.Renderer(0)
    try:
        r.set_history_motion(True)  # no scene yet: fine
        assert r.motion_info() == {"snapshots": 0, "ms_snapshot": 0.0, "used": False}
        r.set_dynamic(True)
        flat = sptr.setup_default(r, "default")
        cam = sptr.camera_lookat(aspect=W / H)
        r.set_denoise(ITER)
        r.set_denoise_history(MAX_HISTORY)
        r.width, r.height = W, H
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.read_motion()  # no pass yet
        r.render(cam, W, H, spp=1)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.read_motion()  # a pass, but not through a snapshot
        r.update_geometry(*R.deform(flat.positions, flat.spheres, STEP))
        r.render(cam, W, H, spp=1)
        mv = r.read_motion()
        assert mv.shape == (H, W, 2) and np.isfinite(mv).any() and np.isnan(mv).any()
        info = r.motion_info()
        assert info["snapshots"] == 1 and info["used"] and info["ms_snapshot"] > 0
        r.set_denoise(0)  # no pass: nothing to read
        r.render(cam, W, H, spp=1)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.read_motion()
        # everything off, the uploaded coordinates again: the golden image
        r.set_history_motion(False)
        r.set_denoise_history(0)
        r.update_geometry(flat.positions, flat.spheres)
        st = r.render(sptr.camera_lookat(aspect=1.0), 256, 256, spp=4)
        rgb, acc = r.read_rgb8(), r.read_accum()
        frac = float((rgb == g["rgb"]).all(axis=2).mean())
        m = np.isfinite(acc) & np.isfinite(g["accum"])
        rel = float(np.abs(acc[m] - g["accum"][m]).sum() / np.abs(g["accum"][m]).sum())
        print(f"golden C1 afterwards: identical RGB8 pixels {frac:.5f}, relative L1 {rel:.2e}")
        assert (~m).sum() <= 3 and frac >= 0.999 and rel <= 1e-3 and st.samples == 256 * 256 * 4
    finally:
        r.close()


# ---------------------------------------------------------------------------------------- 10. the upper layers
def test_cli_motion(tmp_path):
    """sptr_cli --animate K --denoise N --history --motion: HipBackend::Settings::motion through update()."""
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"

    def run(*extra):
        res = subprocess.run([exe, "--scene", "default_emitter", "--w", str(W), "--h", str(H), "--spp", "2", "--animate", "4",
                              "--denoise", str(ITER), "--history", "--json", "--out", str(tmp_path / "a.ppm"), *extra],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        return json.loads(res.stdout.strip().splitlines()[-1])

    on, off = run("--motion"), run()
    print(f"--motion: reprojected {on['reprojected']:.1f} per frame, {on['snapshots']} snapshots of {on['ms_snapshot']:.4f} ms; "
          f"without: reprojected {off['reprojected']:.1f}")
    assert on["motion"] == 1 and on["reprojected"] > 0 and on["snapshots"] == 3 and on["refits"] == 3
    assert off["motion"] == 0 and off["reprojected"] == 0 and off["snapshots"] == 0
