"""GPU: continue_path and the emission line (csrc/kernels_wavefront.hip) in the kernels they are inlined into,
against the float64 path model tests/scatter_ref.py, within the model's bound and no more (tests/
test_scatter_ref_cpu.py holds the float32 oracle to half of it on the CPU and rejects fifteen wrong variants).

  a. the ray path: render_rays with seeds as the paths' rng states and samples = 1, max_depth 1, 2, 3, 6 and tail
     depths 0, 1, 2, 6, every ray set of scatter_common on its scene staged and unstaged (k_shade with k_trace /
     k_trace_dyn, and k_tail); the closest-hit count is the model's segment count and no shadow ray is traced;
  b. the render path: one sample per pixel at 96 x 64 with the states of primary_rays, at the sites of
     test_gpu_env.ROOM_SITES (k_bounce01 + k_bounce, the tail from 1 and from 2, the chain, launch modes 1 and 2,
     unstaged BVH4 and BVH2), each confirmed by its stat, with a black light where the fused kernels need one.

The radiance is exactly 0 where the model's path uses up max_depth without emission or environment, and never
non-finite.  The model flags at most 1 % of any set as fragile; only those rays are excused.  Where the bound is not
derived (a sphere hit from a computed origin) it is 4 x what the oracle needs on the CPU for the same set, not
below 16 eps; nothing comes from the GPU's output.  Not covered here (held by variant equality and the oracle):
k_shade_trace (batches above 21 M paths), k_trace_pm, k_strag, and the PATHTRACER and OPTIX integrators.  Worst
error / bound ratios are printed as `SCATTER_MEASURE` lines (profiles/scatter_measurements.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library, as tests/conftest.py's renderer fixture does

import env_common as E
import residue
import scatter_common as SC
import scatter_ref as R
import sptr
from test_gpu_env import BLACK_LIGHT, ROOM_SITES

pytestmark = pytest.mark.gpu
MAX_FRAGILE = 0.01
ENV_IDS = [f"{kind}{S}" for S, kind, _ in SC.ENVS]
DEPTHS = (1, 2, 3, SC.MAX_DEPTH)
TAILS = (0, 1, 2, 6)


@pytest.fixture()
def clean(renderer):
    """The session's context with every setting these tests touch back at its default afterwards."""
    yield renderer
    renderer.set_tail_depth(0)
    renderer.set_launch_mode(0)
    renderer.set_bounce_chain(0)
    renderer.set_bvh_width(0)
    renderer.set_environment(None)
    renderer.set_lights(sptr.default_lights())


def _upload(r, scene_name, staged, light, width=0):
    sc = SC.scene(scene_name)
    f = SC.flat_scene(sc, SC.SCENES[scene_name][1 if staged else 2])
    r.set_bvh_width(width)
    r.upload_scene(sptr.FlatScene(f["positions"], f["indices"], f["tri_geom_first"], f["spheres"], f["geom_material"]))
    mats = []
    for row in sc["materials"]:
        m = sptr.Material()
        m.albedo[:] = [float(v) for v in row[0:3]]
        m.metallic, m.roughness, m.ior, m.type = float(row[3]), float(row[4]), float(row[8]), 0
        m.emission[:] = [float(v) for v in row[5:8]]
        mats.append(m)
    assert np.array_equal(sptr.materials_as_array(mats), sc["materials"])  # float32 in, float32 out
    r.set_materials(mats)
    if light:
        t, v, c, i = BLACK_LIGHT
        r.set_lights([sptr.Light(t, (C.c_float * 3)(*v), (C.c_float * 3)(*c), i)])
    else:
        r.set_lights([])
    lay = r.scene_layout()
    assert (lay["lds_bytes"] != 0) == staged, lay
    return lay


def _check(what, got, res, oracle_got, depth, worst):
    """The kernels against the bound, no margin; returns the record for the log."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    keep = ~res["fragile"]
    assert (~keep).mean() <= MAX_FRAGILE, (what, float((~keep).mean()))
    r = R.ratio(got, res)
    ro = R.ratio(oracle_got, res)
    k = int(np.argmax(np.where(keep, r, -1.0)))
    rec = {"what": what, "n": len(r), "fragile": int((~keep).sum()), "underived": int((keep & res["underived"]).sum()),
           "gpu_worst_ratio": round(float(r[k]), 4), "oracle_worst_ratio": round(float(ro[keep].max()), 4)}
    if r[k] > worst.get("gpu_worst_ratio", -1.0):
        worst.update(rec)
    assert r[k] <= 1.0, (rec, int(k), got[k], res["value"][k], res["tol"][k], res["kind"][k].tolist())
    ended = keep & (res["segments"] == depth) & (res["value"] == 0).all(axis=1) & (res["env_scale"] == 0).all(axis=1)
    assert (got[ended] == 0).all(), what
    return rec


# ------------------------------------------------------------------------------------------ a. the ray path
@pytest.mark.parametrize("staged", [True, False], ids=["staged", "unstaged"])
@pytest.mark.parametrize("name", SC.SET_NAMES)
def test_paths_through_the_ray_path(clean, name, staged):
    """k_trace / k_trace_dyn and k_shade at bounces 1 to 5, and k_tail from bounce 1 and 2."""
    r = clean
    rs = SC.ray_set(name)
    _upload(r, rs.scene_name, staged, light=False)
    rays = rs.rays()
    worst = {}
    for e, (S, kind, state) in enumerate(SC.ENVS):
        r.set_environment(E.env_map(kind, S), *state)
        for depth in DEPTHS:
            res = rs.bound(e, depth)
            assert not res["fragile"].any()  # (the set was drawn without them)
            for tail in TAILS:
                r.set_tail_depth(tail)
                got = r.render_rays(rays, seeds=rs.states, samples=1, max_depth=depth)
                info = r.ray_render_info()
                # every segment the model predicts was traced, and no other: the branch sequences agree
                assert info["closest"] == int(res["segments"].sum()), (name, tail, depth, info)
                assert info["shadow"] == 0, info
                _check(f"rays {name} {'staged' if staged else 'unstaged'} {ENV_IDS[e]} depth={depth} tail={tail}", got, res,
                       rs.oracle(e, depth)[0], depth, worst)
    residue.log_parity(f"SCATTER_MEASURE gpu rays {name} {'staged' if staged else 'unstaged'}", worst)


# ------------------------------------------------------------------------------------------ b. the render path
_frame_models = {}


def _frame_model(r, scene_name, cam, e, depth):
    """The model on the GPU's own primary rays and rng states of the frame (shared by the sites)."""
    key = (scene_name, e, depth)
    if key not in _frame_models:
        rs = SC.ray_set("frame_" + scene_name)
        dirs, rng = r.primary_rays(cam, SC.FRAME_W, SC.FRAME_H, 1)
        S, kind, state = SC.ENVS[e]
        res = R.trace(SC.scene(scene_name), cam.as_array()[:3], dirs.reshape(-1, 3), rng.ravel(),
                      (E.env_map(kind, S), state[0], state[1]), depth, du_underived=rs.granted_du(e, depth)[0])
        _frame_models[key] = (res, rs.oracle(e, depth)[0])
    return _frame_models[key]


# test_gpu_env's sites and stat predicates.  The mirror room's paths end by bounce 3; these outlive bounce 4, where
# the automatic policy hands a small staged batch to the tail, so the one site that leaves the tail depth to that
# policy while its predicate wants no tail rays asks for no tail.
SITES = [(name, N, light, cfg if cfg or name != "k_bounce01 + k_bounce" else {"tail": SC.MAX_DEPTH}, reached)
         for name, N, light, cfg, reached in ROOM_SITES]
assert sum(cfg != old[3] for cfg, old in zip((s[3] for s in SITES), ROOM_SITES)) == 1


@pytest.mark.parametrize("scene_name", list(SC.SCENES))
@pytest.mark.parametrize("site", SITES, ids=[s[0] for s in SITES])
def test_paths_through_render(clean, site, scene_name):
    """One sample per pixel: each pixel's path is its primary ray's with the state primary_rays reports."""
    name, N, light, cfg, reached = site
    staged = N == E.ROOM_N_STAGED
    r = clean
    lay = _upload(r, scene_name, staged, light, cfg.get("width", 0))
    if "width" in cfg:
        assert lay["bvh_width"] == cfg["width"], lay
    r.set_tail_depth(cfg.get("tail", 0))
    r.set_bounce_chain(cfg.get("chain", 0))
    r.set_launch_mode(cfg.get("mode", 0))
    pos, target, fov = SC.RENDER_CAMERAS[scene_name]
    cam = sptr.camera_lookat(pos=pos, target=target, fov=fov, aspect=SC.FRAME_W / SC.FRAME_H)
    worst = {}
    for e, (S, kind, state) in enumerate(SC.ENVS):
        r.set_environment(E.env_map(kind, S), *state)
        for depth in (2, SC.MAX_DEPTH):
            res, oracle_got = _frame_model(r, scene_name, cam, e, depth)
            st = r.render(cam, SC.FRAME_W, SC.FRAME_H, spp=1, max_depth=depth)
            got = r.read_accum().reshape(-1, 3)
            if depth == SC.MAX_DEPTH:
                assert reached(st), (name, st.as_dict())
            nfrag = int(res["fragile"].sum())
            # every segment the model predicts was traced, and no other (a fragile path may differ by depth - 1)
            assert abs(int(st.rays_closest) - int(res["segments"].sum())) <= (depth - 1) * nfrag, (st.rays_closest, nfrag)
            assert (st.rays_shadow > 0) == light  # (the black light's shadow rays are traced; they add 0)
            _check(f"render {scene_name} [{name}] {ENV_IDS[e]} depth={depth}", got, res, oracle_got, depth, worst)
    residue.log_parity(f"SCATTER_MEASURE gpu render {scene_name} [{name}]", worst)
