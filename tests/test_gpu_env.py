"""GPU: the cubemap lookup env_color<true> (csrc/kernels_wavefront.hip) at its call sites against the float64
model tests/env_ref.py, within the model's derived error bound and no more (tests/test_env_ref_cpu.py holds the
float32 oracle to half of it on the CPU).

  a. direct misses through the ray path (k_trace's non-primary forms): every map, face size and environment state
     with direction sets A to E;
  b. the bounce-0 kernels through render: the pixels whose primary rays miss, against the sample-order sum of the
     model (k_sky in both of its forms, k_trace / k_trace_dyn primary, k_trace_wp, one and two pixel lanes);
  c. bounce >= 1 through the mirror room, where no random number enters a path: albedo^k * model(final direction),
     exactly 0 when the mirrors use up the depth (k_shade, k_trace, k_trace_dyn, k_tail through the ray path;
     k_bounce01, k_bounce, the chain and the tail through render);
  d. state changes (face size, intensity, clamp, back to the sky), also for the second pixel lane's context.

Every site is confirmed by a stat or info call.  Not covered here (held by their variant-equality and oracle
tests): k_trace_pm, which takes frames of millions of pixels; k_strag, which takes a scene beyond an XCD's L2;
k_pathtracer and k_optix, which tonemap before they accumulate.  Worst error / bound ratios are printed as
`ENV_MEASURE` lines (profiles/env_measurements.txt)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import env_common as E
import env_ref
import oracle
import sptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 150, 82
MISS = 0xFFFFFFFF
INVALID = -1


def _sky_ilp():
    """SPTR_SKY_ILP's default, read from the kernel source."""
    text = open(os.path.join(ROOT, "simple-path-tracer_amd", "csrc", "kernels_wavefront.hip")).read()
    return int(re.search(r"#define\s+SPTR_SKY_ILP\s+(\d+)", text).group(1))


SKY_ILP = _sky_ilp()
SPPS = (1, SKY_ILP + 1)
LANE_GROUP_SPP = 16 + SKY_ILP + 1  # lane groups (k_trace_wp, the sky split) take batches of 16 samples or more


@pytest.fixture()
def clean(renderer):
    """The session's context with every setting these tests touch back at its default afterwards."""
    yield renderer
    renderer.set_wave_paths(0)
    renderer.set_tail_depth(0)
    renderer.set_launch_mode(0)
    renderer.set_pixel_lanes(0)
    renderer.set_bounce_chain(0)
    renderer.set_sky_split(0, 0)
    renderer.set_seed_offset(0)
    renderer.set_bvh_width(0)
    renderer.set_environment(None)
    renderer.set_lights(sptr.default_lights())


def _flat(sc):
    return sptr.FlatScene(sc["positions"], sc["indices"], sc["tri_geom_first"], sc["spheres"], sc["geom_material"])


def _material(albedo, metallic, roughness):
    m = sptr.Material()
    m.albedo[:] = albedo
    m.metallic, m.roughness, m.ior, m.type = metallic, roughness, 1.0, 0
    m.emission[:] = (0.0, 0.0, 0.0)
    return m


def _rays(origin, dirs, tfar=0.0):
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    r = np.zeros((len(d), 8), np.float32)
    r[:, 0:3] = np.asarray(origin, np.float32)
    r[:, 3:6] = d
    r[:, 7] = tfar
    return r


def _report(what, r, extra="", oracle_ratio=None):
    """Prints the worst error / bound ratio of the GPU (and of the float32 oracle on the same directions); returns
    the index of the GPU's worst."""
    k = int(np.argmax(r))
    o = "" if oracle_ratio is None else f" oracle_worst_ratio={float(np.max(oracle_ratio)):.4f}"
    print(f"ENV_MEASURE gpu {what} n={len(r)} worst_ratio={float(r[k]):.4f}{o} {extra}")
    return k


def _ratio(got, val, tol):
    err = np.abs(np.asarray(got, np.float64) - val)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / tol).max(axis=1)
    return np.where(np.isnan(r), np.inf, r)


# ------------------------------------------------------------------------------------------ a. direct misses
@pytest.mark.parametrize("kind,S", [(kind, S) for kind in E.KINDS for S in E.SIZES])
def test_direct_misses_through_the_ray_path(clean, kind, S):
    r = clean
    r.upload_scene(_flat(E.far_scene()))
    r.set_materials([_material((0.5, 0.5, 0.5), 0.0, 0.5)])
    r.set_lights([])
    faces = E.env_map(kind, S)
    sets = E.direction_sets(S)
    dev = {name: torch.from_numpy(_rays(E.FAR_ORIGIN, d)).to("cuda:0") for name, (d, _) in sets.items()}
    worst = 0.0
    for state in E.STATES:
        r.set_environment(faces, *state)
        for name, (dirs, either) in sets.items():
            host = _rays(E.FAR_ORIGIN, dirs)
            for depth in (1, 6):
                for path in ("host", "device"):
                    got = r.render_rays(host if path == "host" else dev[name], max_depth=depth)
                    got = got.cpu().numpy() if path == "device" else got
                    info = r.ray_render_info()
                    assert info["closest"] == len(dirs) and info["shadow"] == 0, (name, depth, path, info)
                    ratio = env_ref.ratio(got, dirs, faces, state[0], state[1], either_face=either)
                    k = int(ratio.argmax())
                    if depth == 1 and path == "host":
                        o = env_ref.ratio(oracle.env(dirs, faces, *state), dirs, faces, state[0], state[1], either_face=either)
                        _report(f"direct {kind} S={S} state={state} set={name}", ratio, oracle_ratio=o)
                    if ratio[k] > 1.0:
                        print(f"{kind} S={S} state={state} set {name} depth {depth} ({path}): direction {dirs[k]} got {got[k]}",
                              "model", env_ref.lookup(dirs[k:k + 1], faces, *state)[0][0],
                              "(face, x, y) got", E.decode(got[k], S, state[0]) if kind == "coordinate" else "")
                    assert ratio[k] <= 1.0, (kind, S, state, name, depth, path, dirs[k], float(ratio[k]))
                    worst = max(worst, float(ratio[k]))
            if name == "E":  # interior texel centres: the texel itself
                d, face, gx, gy = E.dirs_texel_grid(S)
                m = (gx % 1 == 0) & (gy % 1 == 0) & (gx > 0) & (gx < S - 1) & (gy > 0) & (gy < S - 1)
                if m.any():
                    want = np.minimum(faces[face[m], gy[m].astype(int), gx[m].astype(int)].astype(np.float64), state[1]) * state[0]
                    tol = env_ref.lookup(d[m], faces, *state)[1]
                    assert (np.abs(got[m] - want) <= tol).all()
    print(f"ENV_MEASURE gpu direct {kind} S={S} worst_ratio={worst:.4f}")


# ------------------------------------------------------------------------------------------ b. bounce 0
def _site_envs():
    return [(S, kind, state, E.env_map(kind, S)) for S, kind, state in E.SITE_CONFIGS]


class _Frames:
    """Per scene: the primary rays of accumulation indices 1 .. n, which pixels miss with every sample, and the
    model's sample-order sums (value, bound) per environment."""

    def __init__(self, r, cam, nmax):
        self.dirs, self.miss = [], []
        o = cam.as_array()[:3]
        for acc in range(1, nmax + 1):
            d, _ = r.primary_rays(cam, W, H, acc)
            d = d.reshape(-1, 3)
            geom = r.query_rays(_rays(o, d, tfar=np.inf), fields=["geom"])["geom"]
            self.dirs.append(d)
            self.miss.append(geom == MISS)
        self.cache = {}

    def expect(self, key, faces, state, spp):
        if (key, spp) not in self.cache:
            val, tol, osum = np.zeros((W * H, 3)), np.zeros((W * H, 3)), np.zeros((W * H, 3), np.float32)
            for s in range(spp):
                v, t, _ = env_ref.lookup(self.dirs[s], faces, *state)
                val, tol = val + v, tol + t
                osum = osum + oracle.env(self.dirs[s], faces, *state)  # (the oracle's float32 sum, in sample order)
            self.cache[(key, spp)] = (val, tol, np.logical_and.reduce(self.miss[:spp]), osum)
        return self.cache[(key, spp)]


def _check_frame(r, frames, key, faces, state, spp, what):
    val, tol, miss, osum = frames.expect(key, faces, state, spp)
    got = r.read_accum().reshape(-1, 3)
    assert miss.sum() >= W * H // 10, (what, int(miss.sum()))
    ratio = _ratio(got[miss], val[miss], tol[miss])
    k = _report(f"bounce0 {what} spp={spp} S={faces.shape[1]}", ratio, f"miss_pixels={int(miss.sum())}",
                _ratio(osum[miss], val[miss], tol[miss]))
    assert ratio[k] <= 1.0, (what, spp, int(np.flatnonzero(miss)[k]), float(ratio[k]))


def test_bounce_0_staged_scene(clean):
    """k_sky's per-pixel form (the culled pixels) beside k_trace's primary form (the others), one and two pixel
    lanes, and k_trace alone without a cull mask."""
    r = clean
    sptr.setup_default(r, "default_emitter")
    assert r.scene_layout()["lds_bytes"] != 0
    cam = sptr.camera_lookat(aspect=W / H)
    frames = _Frames(r, cam, max(SPPS))
    for S, kind, state, faces in _site_envs():
        r.set_environment(faces, *state)
        for spp in SPPS:
            for lanes in (0, 1, 2):
                r.set_pixel_lanes(lanes)
                st = r.render(cam, W, H, spp=spp, max_depth=1)
                info = r.pixel_lanes_info()
                assert info["requested"] == lanes and info["active"] == (lanes == 2), info
                assert 0 < st.traced_primary < W * H * spp  # some pixels traced, the culled ones summed by k_sky
                assert st.rays_closest == W * H * spp
                _check_frame(r, frames, (S, kind), faces, state, spp, f"staged lanes={lanes}")
            r.set_pixel_lanes(0)
            st = r.render(cam, W, H, spp=spp, max_depth=1, flags=sptr.SPTR_FRAME_NO_CULL)
            assert st.traced_primary == W * H * spp  # no mask: every miss is k_trace's
            _check_frame(r, frames, (S, kind), faces, state, spp, "staged no cull")


def test_bounce_0_lane_groups_and_the_sky_split(clean):
    """Batches of 16 samples or more take lane groups (k_trace_wp); with the split on, the culled bulk is summed by
    k_sky's list form."""
    r = clean
    sptr.setup_default(r, "default_emitter")
    cam = sptr.camera_lookat(aspect=W / H)
    spp = LANE_GROUP_SPP
    frames = _Frames(r, cam, spp)
    for S, kind, state, faces in _site_envs():
        r.set_environment(faces, *state)
        for mode, threads in ((2, 1024), (1, 0)):
            r.set_sky_split(mode, threads)
            st = r.render(cam, W, H, spp=spp, max_depth=1)
            assert r.sky_split_info()["bulk_threads"] == (threads if mode == 2 else 0), r.sky_split_info()
            assert 0 < st.traced_primary < W * H * spp
            _check_frame(r, frames, (S, kind), faces, state, spp, f"lane groups split={'on' if mode == 2 else 'off'}")


def test_bounce_0_unstaged_scene(clean):
    """A scene too large to stage: k_trace_dyn (BVH4) and k_trace (BVH2) serve bounce 0."""
    r = clean
    cam = sptr.camera_lookat(aspect=W / H)
    for width in (0, 2):
        r.set_bvh_width(width)
        sptr.setup_default(r, "sphere_mesh", 40, 80)
        lay = r.scene_layout()
        assert lay["lds_bytes"] == 0 and lay["bvh_width"] == (4 if width == 0 else 2), lay
        frames = _Frames(r, cam, max(SPPS))
        for S, kind, state, faces in _site_envs():
            r.set_environment(faces, *state)
            for spp in SPPS:
                st = r.render(cam, W, H, spp=spp, max_depth=1)
                assert 0 < st.traced_primary <= W * H * spp
                _check_frame(r, frames, (S, kind), faces, state, spp, f"unstaged bvh{lay['bvh_width']}")


# ------------------------------------------------------------------------------------------ c. mirrors
BLACK_LIGHT = (0, (0.3, -1.0, 0.2), (0.0, 0.0, 0.0), 2.0)


def _room(r, N, light):
    r.upload_scene(_flat(E.room_scene(N)))
    r.set_materials([_material(E.MIRROR_ALBEDO, 1.0, 0.5)])
    if light:
        t, v, c, i = BLACK_LIGHT
        r.set_lights([sptr.Light(t, (C.c_float * 3)(*v), (C.c_float * 3)(*c), i)])
    else:
        r.set_lights([])
    lay = r.scene_layout()
    assert (lay["lds_bytes"] != 0) == (N == E.ROOM_N_STAGED), lay
    return lay


def _room_ratio(got, origin, dirs, faces, state, depth):
    """(the GPU's ratios, the oracle's on the model's final directions, k, drop)."""
    val, tol, k, drop = E.room_expectation(origin, dirs, faces, state[0], state[1], depth)
    return _ratio(got, val, tol), _ratio(E.room_oracle(origin, dirs, faces, state, depth), val, tol), k, drop


@pytest.mark.parametrize("N", [E.ROOM_N_STAGED, E.ROOM_N_UNSTAGED], ids=["staged", "unstaged"])
@pytest.mark.parametrize("light", [False, True], ids=["no_light", "black_light"])
def test_mirror_paths_through_the_ray_path(clean, N, light):
    """k_trace / k_trace_dyn and k_shade at bounces 1 to 3, and k_tail from bounce 1 and 2."""
    r = clean
    _room(r, N, light)
    dirs = E.room_rays()
    rays = _rays(E.ROOM_ORIGIN, dirs)
    for S, kind, state, faces in _site_envs():
        r.set_environment(faces, *state)
        for tail in (0, 1, 2, 6):
            r.set_tail_depth(tail)
            for depth in (1, 2, 3, 6):
                got = r.render_rays(rays, max_depth=depth)
                info = r.ray_render_info()
                ratio, oratio, k, drop = _room_ratio(got, E.ROOM_ORIGIN, dirs, faces, state, depth)
                assert drop.sum() == 0
                # every segment the model predicts was traced, and no other: the mirror sequences agree
                assert info["closest"] == int(np.minimum(k + 1, depth).sum()), (tail, depth, info)
                assert (info["shadow"] > 0) == light, info  # (the black light's shadow rays are traced; they add 0)
                j = _report(f"mirrors rays N={N} light={light} tail={tail} depth={depth} S={S}", ratio, oracle_ratio=oratio)
                assert ratio[j] <= 1.0, (tail, depth, dirs[j], int(k[j]), got[j], float(ratio[j]))
                assert (got[k >= depth] == 0).all()  # exactly 0, with the black light too


ROOM_CAMERA = dict(pos=E.ROOM_ORIGIN, target=(-3.0, 1.0, -3.0))
# (name, N, black light, settings, what the stats must show)
ROOM_SITES = [
    ("k_bounce01 + k_bounce", E.ROOM_N_STAGED, True, {}, lambda st: st.traced_fused > 0 and st.rays_tail == 0),
    ("k_bounce01, tail from 2", E.ROOM_N_STAGED, True, {"tail": 2}, lambda st: st.traced_fused > 0 and st.rays_tail > 0),
    ("chain", E.ROOM_N_STAGED, True, {"chain": 2}, lambda st: st.traced_fused > 0),
    ("tail from 1", E.ROOM_N_STAGED, True, {"tail": 1}, lambda st: st.rays_tail > 0 and st.traced_fused == 0),
    ("staged, no light: k_shade + k_trace", E.ROOM_N_STAGED, False, {"tail": 6},
     lambda st: st.traced_bounce > 0 and st.traced_fused == 0 and st.rays_tail == 0),
    ("launch mode 1", E.ROOM_N_STAGED, True, {"mode": 1}, lambda st: st.traced_fused > 0),
    ("launch mode 2", E.ROOM_N_STAGED, True, {"mode": 2}, lambda st: st.traced_fused > 0),
    ("unstaged: k_shade + k_trace_dyn", E.ROOM_N_UNSTAGED, True, {"tail": 6},
     lambda st: st.traced_bounce > 0 and all(st.traced_by_depth[d] > 0 for d in (1, 2, 3)) and st.rays_tail == 0),
    ("unstaged, no light: k_trace_dyn's own misses", E.ROOM_N_UNSTAGED, False, {"tail": 6},
     lambda st: st.traced_bounce > 0 and st.rays_tail == 0),
    ("unstaged, tail from 1", E.ROOM_N_UNSTAGED, False, {"tail": 1}, lambda st: st.rays_tail > 0),
    ("unstaged, tail from 2", E.ROOM_N_UNSTAGED, True, {"tail": 2}, lambda st: st.rays_tail > 0 and st.traced_bounce > 0),
    ("unstaged BVH2: k_shade + k_trace", E.ROOM_N_UNSTAGED, False, {"tail": 6, "width": 2},
     lambda st: st.traced_bounce > 0 and st.rays_tail == 0),
]


@pytest.mark.parametrize("site", ROOM_SITES, ids=[s[0] for s in ROOM_SITES])
def test_mirror_paths_through_render(clean, site):
    """A camera looking into the corner of the mirror room, one sample per pixel: each pixel's path is its primary
    ray's, so the frame is albedo^k * model(final direction) wherever the path keeps 1e-3 away from a border."""
    name, N, light, cfg, reached = site
    r = clean
    r.set_bvh_width(cfg.get("width", 0))
    lay = _room(r, N, light)
    if "width" in cfg:
        assert lay["bvh_width"] == cfg["width"], lay
    r.set_tail_depth(cfg.get("tail", 0))
    r.set_bounce_chain(cfg.get("chain", 0))
    r.set_launch_mode(cfg.get("mode", 0))
    cam = sptr.camera_lookat(aspect=W / H, **ROOM_CAMERA)
    origin = cam.as_array()[:3]
    dirs = r.primary_rays(cam, W, H, 1)[0].reshape(-1, 3)
    for S, kind, state, faces in _site_envs():
        r.set_environment(faces, *state)
        for depth in (2, 6):
            st = r.render(cam, W, H, spp=1, max_depth=depth)
            got = r.read_accum().reshape(-1, 3)
            ratio, oratio, k, drop = _room_ratio(got, origin, dirs, faces, state, depth)
            shares = np.bincount(k, minlength=4) / len(k)
            assert drop.mean() <= 0.01 and (shares[1:4] >= 0.05).all(), (float(drop.mean()), shares)
            if depth == 6:
                assert reached(st), (name, st.as_dict())
            # every segment the model predicts was traced, and no other (a dropped path may differ by its 3 bounces)
            assert abs(int(st.rays_closest) - int(np.minimum(k + 1, depth).sum())) <= 3 * int(drop.sum()), st.rays_closest
            assert (st.rays_shadow > 0) == light
            keep = ~drop
            j = _report(f"mirrors render [{name}] depth={depth} S={S}", ratio[keep], f"dropped={int(drop.sum())}", oratio[keep])
            assert ratio[keep][j] <= 1.0, (name, depth, int(np.flatnonzero(keep)[j]), float(ratio[keep][j]))
            assert (got[keep & (k >= depth)] == 0).all()


# ------------------------------------------------------------------------------------------ d. state changes
def _sky_rel_l1(got, dirs):
    want = oracle.env(dirs, None)
    return float(np.abs(got - want).sum() / np.abs(want).sum())


def test_state_changes_take_effect_on_the_next_call(clean):
    r = clean
    r.upload_scene(_flat(E.far_scene()))
    r.set_materials([_material((0.5, 0.5, 0.5), 0.0, 0.5)])
    r.set_lights([])
    dirs = E.dirs_uniform(5000, seed=9)
    rays = _rays(E.FAR_ORIGIN, dirs)
    steps = [("noise", 16, (0.8, 5.0)), ("noise", 3, (0.8, 5.0)), ("noise", 257, (0.8, 5.0)),
             ("noise", 257, (2.5, 0.75)), ("noise", 257, (1.0, 1e30)), ("coordinate", 257, (1.0, 1e30))]
    last = None
    for kind, S, state in steps:
        faces = E.env_map(kind, S)
        r.set_environment(faces, *state)
        got = r.render_rays(rays, max_depth=6)
        ratio = env_ref.ratio(got, dirs, faces, *state)
        k = _report(f"state change to {kind} S={S} state={state}", ratio,
                    oracle_ratio=env_ref.ratio(oracle.env(dirs, faces, *state), dirs, faces, *state))
        assert ratio[k] <= 1.0, (kind, S, state, float(ratio[k]))
        assert last is None or not np.array_equal(got, last)
        last = got
    r.set_environment(None)
    got = r.render_rays(rays, max_depth=6)
    rel = _sky_rel_l1(got, dirs)
    print(f"back to the sky: relative L1 to the oracle's sky {rel:.2e}")
    assert rel <= 1e-3  # tests/test_gpu_ray_render.py's bound for the sky through this path


def test_state_changes_reach_the_second_pixel_lane(clean):
    """Two pixel lanes in launch mode 3, as tests/test_gpu_parity.py::test_pixel_lanes_follow_shading_changes: the
    lane's launch graph is captured before each change, and the frame after it must show the new environment."""
    r = clean
    sptr.setup_default(r, "default_emitter")
    cam = sptr.camera_lookat(aspect=W / H)
    frames = _Frames(r, cam, 1)
    r.set_launch_mode(3)
    r.set_pixel_lanes(2)
    steps = [("noise", 16, (0.8, 5.0)), ("noise", 3, (0.8, 5.0)), ("coordinate", 257, (0.8, 5.0)),
             ("coordinate", 257, (2.5, 0.75)), ("coordinate", 257, (1.0, 1e30))]
    for kind, S, state in steps:
        faces = E.env_map(kind, S)
        r.set_environment(faces, *state)
        for _ in range(3):  # (a shape is captured on its second call and replayed on its third)
            r.render(cam, W, H, spp=1, max_depth=1)
        assert r.pixel_lanes_info()["active"]
        _check_frame(r, frames, (kind, S, state), faces, state, 1, f"two lanes after a change to {kind} S={S} {state}")
    r.set_environment(None)
    for _ in range(3):
        r.render(cam, W, H, spp=1, max_depth=1)
    assert r.pixel_lanes_info()["active"]
    miss = frames.miss[0]
    got = r.read_accum().reshape(-1, 3)[miss]
    rel = _sky_rel_l1(got, frames.dirs[0][miss])
    print(f"two lanes back to the sky: relative L1 {rel:.2e}")
    assert rel <= 1e-3


# ------------------------------------------------------------------------------------------ the face-size limit
def test_face_sizes_beyond_the_index_range_are_refused(clean):
    """6 S^2 must stay below 2^32 (S <= 26 754): a larger size is refused before faces is read (the buffer here holds
    one 2 x 2 map) and leaves the environment as it was."""
    r = clean
    r.upload_scene(_flat(E.far_scene()))
    r.set_materials([_material((0.5, 0.5, 0.5), 0.0, 0.5)])
    r.set_lights([])
    faces = E.env_map("noise", 3)
    r.set_environment(faces, 0.8, 5.0)
    dirs = E.dirs_uniform(2000, seed=10)
    rays = _rays(E.FAR_ORIGIN, dirs)
    before = r.render_rays(rays)
    small = np.ascontiguousarray(E.env_map("noise", 2))
    for size in (26755, 65536, 2 ** 31 - 1, 1, 0, -5):
        e = sptr.Environment()
        e.faces = small.ctypes.data_as(C.POINTER(C.c_float))
        e.size, e.intensity, e.max_clamp = size, 3.0, 1.0
        assert r._L.sptr_set_environment(r._h, C.byref(e)) == INVALID, size
        assert r._L.sptr_last_error(r._h), size
        assert np.array_equal(r.render_rays(rays), before), size
    with pytest.raises(sptr.SptrError, match="rc=-1:"):
        r.set_environment(np.zeros((6, 1, 1, 3), np.float32))
    assert env_ref.ratio(before, dirs, faces, 0.8, 5.0).max() <= 1.0
