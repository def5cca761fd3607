"""GPU tests of path-traced radiance for caller-supplied rays: sptr_render_rays / sptr_ray_render_info
(k_rays_inject, k_rays_gather, kernels_rays.h, and the integrator's chain entered at depth 0 through its
non-primary instantiations) through Renderer.render_rays / ray_render_info and sptr_cli --panorama.

The yardstick is the renderer itself: a ray with the origin, direction and rng state of a camera path must
return that path's radiance, so the primary rays of a frame (Renderer.primary_rays) through the ray path give
the frame's accumulation (read_accum).  "Equal" is equality of the uint32 bit patterns, non-finite values
included.  Frames are 150 x 82: ragged 32x32 tiles on both edges, 12 300 paths, several blocks."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import oracle
import sptr
import test_ray_render_cpu as RC
import workloads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
W, H = 150, 82
INVALID, NO_SCENE = -1, -3
SHAPE_NS = (0, 1, 63, 64, 65, 257, 600001)  # 600 001: more paths than any resident grid has threads


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _equal(got, want, what):
    got, want = _bits(got).reshape(-1), _bits(want).reshape(-1)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    print(f"{what}: {bad} of {got.size} words differ")
    assert bad == 0, what


def _rays(origin, dirs):
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    r = np.zeros((len(d), 8), np.float32)
    r[:, 0:3] = np.asarray(origin, np.float32)
    r[:, 3:6] = d
    return r


def _frame_rays(r, cam, acc):
    """(rays, rng) of the W x H frame with accumulation index acc, pixel y * W + x."""
    dirs, rng = r.primary_rays(cam, W, H, acc)
    return _rays(cam.as_array()[:3], dirs), rng.reshape(-1).copy()


def _frame(r, cam, depth, acc=1, spp=1):
    """read_accum of one call of spp frames whose seeds are those of accumulation index acc, acc + 1, ..."""
    r.set_seed_offset(acc - 1)
    try:
        r.render(cam, W, H, spp=spp, max_depth=depth)
        return r.read_accum().reshape(-1, 3)
    finally:
        r.set_seed_offset(0)


def _point_lights():
    sun = sptr.default_lights()[0]
    point = sptr.Light(1, (C.c_float * 3)(1.5, 4.0, 2.0), (C.c_float * 3)(1.0, 0.8, 0.6), 30.0)
    fill = sptr.Light(0, (C.c_float * 3)(0.6, -1.0, -0.2), (C.c_float * 3)(0.4, 0.5, 0.9), 0.7)
    return [sun, point, fill]


def _setup(r, name):
    """The five scenes of the frame test; returns the camera."""
    r.set_bvh_width(0)
    if name == "mesh":  # too large to be staged: walked as BVH4
        sptr.setup_default(r, "sphere_mesh", 40, 80)
        lay = r.scene_layout()
        assert lay["lds_bytes"] == 0 and lay["bvh_width"] == 4
    elif name == "chair":
        sptr.setup_default(r, "gltf:" + workloads.CHAIR, 7, 0, env_faces=workloads.hdr_env_faces(64))
    elif name == "lights":
        sptr.setup_default(r, "default")
        r.set_lights(_point_lights())
    else:
        sptr.setup_default(r, name)
        assert r.scene_layout()["lds_bytes"] != 0
    return sptr.camera_lookat(aspect=W / H)


@pytest.fixture()
def clean(renderer):
    """The session's context with every setting these tests touch back at its default afterwards."""
    yield renderer
    renderer.set_wave_paths(0)
    renderer.set_tail_depth(0)
    renderer.set_launch_mode(0)
    renderer.set_pixel_lanes(0)
    renderer.set_seed_offset(0)
    renderer.set_denoise_history(0)
    renderer.set_denoise(0)
    renderer.set_bvh_width(0)
    renderer.set_environment(None)
    renderer.set_lights(sptr.default_lights())


# ------------------------------------------------------------------------------- 1. a frame through the ray path
@pytest.mark.parametrize("scene", ["default", "default_emitter", "mesh", "chair", "lights"])
def test_a_frame_through_the_ray_path(clean, scene):
    """The depth-0 non-primary chain equals the primary one: at every pixel, depths 1, 2 and 6."""
    r = clean
    cam = _setup(r, scene)
    for depth, acc in ((1, 1), (2, 3), (6, 1)):
        rays, _ = _frame_rays(r, cam, acc)
        want = _frame(r, cam, depth, acc)
        got = r.render_rays(rays, frame_index=acc, max_depth=depth)
        info = r.ray_render_info()
        assert info["chunks"] == 1 and info["closest"] >= W * H and info["ms"] > 0.0
        assert np.isfinite(want).all() and (want > 0).any()
        _equal(got, want, f"{scene} depth {depth} acc {acc}: render_rays vs read_accum")
    if scene == "lights":
        assert info["shadow"] > W * H // 4  # (the lit hits queue tasks for three lights)


def test_a_frame_with_explicit_seeds(clean):
    r = clean
    cam = _setup(r, "default_emitter")
    rays, rng = _frame_rays(r, cam, 4)
    want = _frame(r, cam, 6, 4)
    _equal(r.render_rays(rays, seeds=rng, frame_index=9, max_depth=6), want, "seeds = primary_rays' rng")
    _equal(r.render_rays(rays, frame_index=4, max_depth=6), want, "no seeds, frame_index = acc")


def test_a_frame_after_a_two_lane_accumulation_and_an_upload(clean):
    """An upload after a two-lane accumulation leaves the pixel buffers without a layout until the next render:
    primary_rays and render_rays, which read no pixel, must work in that state (they divided by a tile count of
    zero), and a ray render between two-lane calls leaves them as they are."""
    r = clean
    cam = _setup(r, "default_emitter")
    r.set_pixel_lanes(2)
    r.render(cam, W, H, spp=4, max_depth=6)
    assert r.pixel_lanes_info()["active"]
    want4 = r.read_accum().reshape(-1, 3)
    _setup(r, "default_emitter")  # (the upload)
    rays, rng = _frame_rays(r, cam, 1)
    got = r.render_rays(rays, seeds=rng, max_depth=6)
    r.render(cam, W, H, spp=4, max_depth=6)
    assert r.pixel_lanes_info()["active"]
    _equal(r.read_accum().reshape(-1, 3), want4, "two-lane accumulation after an upload and a ray render")
    r.set_pixel_lanes(1)
    _equal(got, _frame(r, cam, 6, 1), "render_rays in the state an upload leaves after two lanes")


# ------------------------------------------------------------------------------- 2. accumulation
def test_accumulating_calls_equal_the_accumulation(clean):
    r = clean
    cam = _setup(r, "default_emitter")
    want = _frame(r, cam, 6, 1, spp=4)
    out = np.zeros((W * H, 3), np.float32)
    for acc in (1, 2, 3, 4):
        rays, _ = _frame_rays(r, cam, acc)
        r.render_rays(rays, frame_index=acc, max_depth=6, accumulate=True, out=out)
    _equal(out, want, "four accumulating calls vs the 4-frame read_accum")


# ------------------------------------------------------------------------------- 3. samples
@pytest.mark.parametrize("seeded", [False, True], ids=["index", "seeds"])
def test_samples_equal_accumulating_single_sample_calls(clean, seeded):
    r = clean
    cam = _setup(r, "default")
    rays, rng = _frame_rays(r, cam, 2)
    seeds = rng if seeded else None
    got = r.render_rays(rays, seeds=seeds, samples=5, frame_index=7, max_depth=6)
    out = np.zeros((W * H, 3), np.float32)
    for s in range(5):
        if seeded:  # the b = seeds[i] rule: the state a single-sample call takes as given
            state = RC.ray_rng(rng, len(rng), 5, 7, s)
            r.render_rays(rays, seeds=state, max_depth=6, accumulate=True, out=out)
        else:
            r.render_rays(rays, frame_index=7 + s, max_depth=6, accumulate=True, out=out)
    _equal(got, out, f"samples = 5 vs five accumulating calls ({'seeds' if seeded else 'ray index'})")
    assert not np.array_equal(_bits(got), _bits(r.render_rays(rays, seeds=seeds, samples=1, frame_index=7)))


# ------------------------------------------------------------------------------- 4. shape and order
@pytest.fixture(scope="module")
def shape_rays():
    """600 001 rays towards the scene from around it (default_rng(11)) with explicit seeds."""
    n = max(SHAPE_NS)
    g = np.random.default_rng(11)
    o = g.uniform([-6.0, 0.0, -6.0], [6.0, 5.0, 8.0], (n, 3))
    tg = g.uniform([-3.0, 0.0, -3.0], [3.0, 3.0, 5.0], (n, 3))
    d = tg - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rr = np.zeros((n, 8), np.float32)
    rr[:, 0:3] = o
    rr[:, 3:6] = d
    seeds = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return rr, seeds


def test_shapes_where_indexing_can_break(clean, shape_rays):
    r = clean
    _setup(r, "mesh")
    rr, seeds = shape_rays
    dev, dseeds = torch.from_numpy(rr).to("cuda:0"), torch.from_numpy(seeds.view(np.int32)).to("cuda:0")
    full = r.render_rays(dev, seeds=dseeds).cpu().numpy()
    print("chunks of the full batch in the wave capacity the session's context has:", r.ray_render_info()["chunks"])
    assert np.isfinite(full).all() and (full > 0).any(axis=1).mean() > 0.9
    nofull = r.render_rays(dev).cpu().numpy()  # (without seeds a ray's state is its index: a prefix is a prefix)
    for n in SHAPE_NS:
        for path in ("host", "device"):
            a = rr[:n] if path == "host" else dev[:n]
            s = seeds[:n] if path == "host" else dseeds[:n]
            got = r.render_rays(a, seeds=s)
            got = got.cpu().numpy() if path == "device" else got
            assert got.shape == (n, 3)
            _equal(got, full[:n], f"n = {n} ({path}), seeds")
            got = r.render_rays(a)
            got = got.cpu().numpy() if path == "device" else got
            _equal(got, nofull[:n], f"n = {n} ({path}), no seeds")
    # a permuted batch with explicit seeds gives the permuted result
    perm = np.random.default_rng(5).permutation(len(rr))
    got = r.render_rays(np.ascontiguousarray(rr[perm]), seeds=np.ascontiguousarray(seeds[perm]))
    _equal(got, full[perm], "permuted batch")


def test_chunks_and_tail_depth_cannot_matter(shape_rays):
    r = sptr.Renderer(0)
    try:
        _chunks_and_tail_depth(r, shape_rays)
    finally:
        r.close()


def _chunks_and_tail_depth(r, shape_rays):
    _setup(r, "default_emitter")
    n = 70001
    rr, seeds = shape_rays[0][:n], shape_rays[1][:n]
    # a context without wave buffers: the first call allocates a capacity that holds the whole batch
    want3 = r.render_rays(rr, seeds=seeds, samples=3, frame_index=2, max_depth=6)
    assert r.ray_render_info()["chunks"] == 1
    want1 = r.render_rays(rr, seeds=seeds, max_depth=6)
    assert r.ray_render_info()["chunks"] == 1
    r.set_wave_paths(20000)  # at least three chunks of whole rays
    _equal(r.render_rays(rr, seeds=seeds, max_depth=6), want1, "4 chunks vs unsplit")
    assert r.ray_render_info()["chunks"] == 4
    _equal(r.render_rays(rr, seeds=seeds, samples=3, frame_index=2, max_depth=6), want3, "11 chunks of 3 samples vs unsplit")
    assert r.ray_render_info()["chunks"] == 11  # 6 666 rays of 3 samples each
    # a capacity below one ray's samples: the sample range is split too, into contiguous ranges in order
    m = 300
    r.set_wave_paths(2)
    for accumulate in (False, True):
        base = np.full((m, 3), 0.25, np.float32)
        ref = base.copy() + want3[:m] if accumulate else want3[:m]
        got = r.render_rays(rr[:m], seeds=seeds[:m], samples=3, frame_index=2, max_depth=6, accumulate=accumulate,
                            out=base.copy())
        assert r.ray_render_info()["chunks"] == 2 * m
        _equal(got, ref, f"sample range split (accumulate={accumulate}) vs unsplit")
    r.set_wave_paths(0)
    for tail in (1, 2, 3, 5, 32):
        r.set_tail_depth(tail)
        _equal(r.render_rays(rr, seeds=seeds, max_depth=6), want1, f"tail depth {tail}")
    r.set_tail_depth(0)
    c0, s0 = r.ray_render_info()["closest"], r.ray_render_info()["shadow"]
    r.set_tail_depth(2)
    r.render_rays(rr, seeds=seeds, max_depth=6)
    info = r.ray_render_info()
    assert (info["closest"], info["shadow"]) == (c0, s0)  # (the query counts do not depend on it either)


def test_two_cameras_interleaved(clean):
    r = clean
    _setup(r, "default_emitter")
    cams = (sptr.camera_lookat(aspect=W / H), sptr.camera_lookat(pos=(3.0, 2.0, 6.0), target=(0.0, 1.0, 0.0), aspect=W / H))
    rays, rngs, frames = [], [], []
    for cam, acc in zip(cams, (1, 6)):
        a, b = _frame_rays(r, cam, acc)
        rays.append(a)
        rngs.append(b)
        frames.append(_frame(r, cam, 6, acc))
    both = np.empty((2 * W * H, 8), np.float32)
    both[0::2], both[1::2] = rays
    seeds = np.empty(2 * W * H, np.uint32)
    seeds[0::2], seeds[1::2] = rngs
    got = r.render_rays(both, seeds=seeds, max_depth=6)
    _equal(got[0::2], frames[0], "interleaved batch, camera 0")
    _equal(got[1::2], frames[1], "interleaved batch, camera 1")


# ------------------------------------------------------------------------------- 5. misses
@pytest.mark.parametrize("env", ["sky", "cubemap"])
def test_rays_that_leave_the_scene_return_the_environment(clean, env):
    r = clean
    faces = workloads.hdr_env_faces(64) if env == "cubemap" else None
    sptr.setup_default(r, "default", env_faces=faces)
    g = np.random.default_rng(3)
    d = g.normal(size=(20000, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.05  # upwards from above the scene
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = _rays((0.0, 40.0, 0.0), d)
    got = r.render_rays(rays, max_depth=6)
    info = r.ray_render_info()
    assert info["closest"] == len(rays) and info["shadow"] == 0  # every path ended at its first segment
    want = oracle.env(rays[:, 3:6], faces)
    rel = float(np.abs(got - want).sum() / np.abs(want).sum())
    print(f"{env}: relative L1 to oracle.env {rel:.2e}, bit-equal {float((_bits(got) == _bits(want)).mean()):.4f}")
    assert rel <= 1e-3  # tests/test_gpu_parity.py's bound on the linear radiance of an image (its environment tests')


# ------------------------------------------------------------------------------- 6. pointers and streams
GUARD = 64


def _guarded(a, fill):
    """a inside a larger device tensor filled with a sentinel: (view, whole)."""
    a = np.ascontiguousarray(a)
    flat = a.reshape(-1)
    big = torch.from_numpy(np.full(flat.size + 2 * GUARD, fill, flat.dtype)).to("cuda:0")
    view = big[GUARD:GUARD + flat.size]
    view.copy_(torch.from_numpy(flat.copy()).to("cuda:0"))
    torch.cuda.synchronize()
    return view.view(a.shape), big


def _intact(big, fill):
    b = big.cpu().numpy()
    return bool((b[:GUARD] == b.dtype.type(fill)).all() and (b[-GUARD:] == b.dtype.type(fill)).all())


def test_device_pointers_guards_streams_and_normalize(clean):
    r = clean
    cam = _setup(r, "default_emitter")
    rays, rng = _frame_rays(r, cam, 1)
    want = r.render_rays(rays, seeds=rng, max_depth=6)  # the host-array path
    _equal(want, _frame(r, cam, 6, 1), "host path vs the frame")
    drays, big_r = _guarded(rays, 7.0)
    dseeds, big_s = _guarded(rng.view(np.int32), 77)
    dout, big_o = _guarded(np.zeros((W * H, 3), np.float32), 123456.0)
    assert drays.data_ptr() % 16 == 0
    got = r.render_rays(drays, seeds=dseeds, max_depth=6, out=dout)
    assert got.data_ptr() == dout.data_ptr() and isinstance(got, torch.Tensor)
    _equal(got.cpu().numpy(), want, "device path vs host path")
    assert _intact(big_r, 7.0) and _intact(big_s, 77) and _intact(big_o, 123456.0)
    assert np.array_equal(_bits(drays.cpu().numpy()), _bits(rays)) and np.array_equal(dseeds.cpu().numpy().view(np.uint32), rng)
    # the same call enqueued on a torch stream: nothing waits on the host, the stream waits for the result
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(stream):
        dout2 = torch.full((W * H, 3), -1.0, dtype=torch.float32, device="cuda:0")
        r.render_rays(drays, seeds=dseeds, max_depth=6, out=dout2, stream=stream.cuda_stream)
        copy = dout2.clone()  # (ordered after the result on that stream)
    stream.synchronize()
    _equal(copy.cpu().numpy(), want, "enqueued on a torch stream vs synchronous")
    assert r.ray_render_info()["ms"] > 0.0
    # SPTR_RAYS_NORMALIZE on scaled directions equals the call on their safe_normalize'd copies
    scaled = rays.copy()
    scaled[:, 3:6] *= np.float32(3.0)
    v = scaled[:, 3:6]
    l2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]  # dot()'s order, float32
    unit = rays.copy()
    unit[:, 3:6] = v * (np.float32(1.0) / np.sqrt(l2))[:, None]
    _equal(r.render_rays(scaled, seeds=rng, max_depth=6, normalize=True), r.render_rays(unit, seeds=rng, max_depth=6),
           "normalize vs safe_normalize'd copies")


# ------------------------------------------------------------------------------- 7. no trace left
def _golden(r):
    g = np.load(os.path.join(GOLD, "radiance.npz"), allow_pickle=False)
    cam = sptr.camera_lookat(aspect=64 / 48)
    st = r.render(cam, 64, 48, spp=1, max_depth=6)
    rgb, acc = r.read_rgb8(), r.read_accum()
    frac = float((rgb == g["default_emitter_d6_rgb"]).all(axis=2).mean())
    rel = float(np.abs(acc - g["default_emitter_d6_accum"]).sum() / np.abs(g["default_emitter_d6_accum"]).sum())
    assert frac >= 0.995 and rel <= 5e-3, (frac, rel)  # (tests/test_gpu_golden.py's criteria for this frame)
    return st, acc


COUNTERS = ("rays_closest", "rays_shadow", "samples", "waves", "rays_tail", "traced_primary", "traced_bounce",
            "traced_by_depth", "traced_fused", "paths_handed_off", "cull_launches")


def test_a_ray_render_leaves_the_golden_frame_and_its_stats(clean, shape_rays):
    r = clean
    _setup(r, "default_emitter")
    st0, acc0 = _golden(r)
    st1, acc1 = _golden(r)  # (a repeat without a ray render in between: what "the same" means)
    r.render_rays(shape_rays[0][:50001], samples=2, max_depth=6)
    assert r.ray_render_info()["closest"] > 50001
    st2, acc2 = _golden(r)
    _equal(acc1, acc0, "golden frame repeated")
    _equal(acc2, acc0, "golden frame after a ray render")
    for k in COUNTERS:
        a, b, c = (st.as_dict()[k] for st in (st0, st1, st2))
        assert b == c and (a == b or k == "cull_launches"), (k, a, b, c)  # (the first call computed the cull mask)


def test_a_captured_graph_is_replayed_not_captured_again(clean, shape_rays):
    r = clean
    cam = _setup(r, "default_emitter")
    r.set_launch_mode(3)  # a graph for every repeated shape
    for _ in range(3):
        r.render(cam, W, H, spp=2, max_depth=6)
    want = r.read_accum()
    g0 = r.graph_info()
    assert g0["valid"] == 1 and g0["captures"] >= 1
    r.render_rays(shape_rays[0][:W * H * 2], max_depth=6)
    r.render(cam, W, H, spp=2, max_depth=6)
    g1 = r.graph_info()
    assert g1["valid"] == 1 and g1["captures"] == g0["captures"] and g1["nodes"] == g0["nodes"]
    _equal(r.read_accum(), want, "replayed graph after a ray render")


def test_a_history_carry_survives_a_ray_render(clean, shape_rays):
    r = clean
    _setup(r, "default")
    a = sptr.camera_lookat(aspect=W / H)
    b = sptr.camera_lookat(pos=(0.3, 3.0, 8.0), target=(0.0, 1.0, 0.0), aspect=W / H)
    r.set_denoise(2)
    r.set_denoise_history(8)
    r.render(a, W, H, spp=1)
    r.render(b, W, H, spp=1)
    want, info0 = r.read_denoised(), r.history_info()
    assert info0["carried"] and info0["reprojected"] > 0
    r.set_denoise_history(8)  # (drops the history held)
    r.render(a, W, H, spp=1)
    r.render_rays(shape_rays[0][:30000], max_depth=6)
    r.render(b, W, H, spp=1)
    info1 = r.history_info()
    assert info1["carried"] and info1["reprojected"] == info0["reprojected"]
    _equal(r.read_denoised(), want, "denoised frame with a ray render between the two frames")


def test_after_update_geometry(shape_rays):
    r = sptr.Renderer(0)
    try:
        r.set_dynamic(True)
        flat = sptr.setup_default(r, "default_emitter")
        cam = sptr.camera_lookat(aspect=W / H)
        rays, rng = _frame_rays(r, cam, 1)
        before = r.render_rays(rays, seeds=rng, max_depth=6)
        sph = flat.spheres.copy()
        sph[:, 0] += 0.35
        sph[:, 1] += 0.2
        r.update_geometry(flat.positions + np.float32(0.05), sph)
        want = _frame(r, cam, 6, 1)
        got = r.render_rays(rays, seeds=rng, max_depth=6)
        _equal(got, want, "after update_geometry: render_rays vs the frame of the refitted scene")
        assert (_bits(got) != _bits(before)).mean() > 0.05  # (the move matters)
    finally:
        r.close()


# ------------------------------------------------------------------------------- 8. errors
def _raw(r, stream=None, reserved=(0, 0, 0, 0), **kw):
    q = sptr.RayRender()
    for k, v in kw.items():
        setattr(q, k, v)
    q.reserved = (C.c_uint32 * 4)(*reserved)
    return r._L.sptr_render_rays(r._h, C.byref(q), C.c_void_p(stream) if stream else None)


def test_errors_leave_the_context_usable(shape_rays):
    n = 1000
    rays = np.ascontiguousarray(shape_rays[0][:n])
    out = np.zeros((n, 3), np.float32)
    ok = dict(rays=rays.ctypes.data, n=n, samples=1, frame_index=1, max_depth=6, flags=0, radiance=out.ctypes.data)
    r = sptr.Renderer(0)
    assert _raw(r, **ok) == NO_SCENE
    with pytest.raises(sptr.SptrError, match="rc=-3:"):
        r.render_rays(rays)
    info = r.ray_render_info()
    assert info == {"ms": 0.0, "closest": 0, "shadow": 0, "chunks": 0}
    sptr.setup_default(r, "default_emitter")
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    shifted = torch.zeros(n * 8 + 4, dtype=torch.float32, device="cuda:0")[1:1 + n * 8]  # 4 bytes off 16-byte alignment
    dout = torch.zeros(n * 3, dtype=torch.float32, device="cuda:0")
    assert shifted.data_ptr() % 16 == 4
    cases = {
        "NULL rays": dict(ok, rays=None),
        "NULL radiance": dict(ok, radiance=None),
        "samples == 0": dict(ok, samples=0),
        "max_depth == 0": dict(ok, max_depth=0),
        "frame_index == 0": dict(ok, frame_index=0),
        "frame_index + samples - 1 overflows": dict(ok, frame_index=0xFFFFFFFF, samples=2),
        "unknown flag": dict(ok, flags=8),
        "non-zero reserved": dict(ok, reserved=(0, 0, 1, 0)),
        "more than 2^28 rays": dict(ok, n=(1 << 28) + 1),
        "more than 2^29 paths": dict(ok, n=1 << 20, samples=(1 << 9) + 1),
        "host pointers on a stream": dict(ok, stream=stream.cuda_stream),
        "misaligned device rays": dict(ok, rays=shifted.data_ptr(), radiance=dout.data_ptr(), flags=sptr.SPTR_RAYS_DEVICE_PTRS),
    }
    for what, kw in cases.items():
        assert _raw(r, **kw) == INVALID, what
        assert r._L.sptr_last_error(r._h), what
        _golden(r)
    assert not out.any() and not dout.cpu().numpy().any()  # (no refused call wrote anything)
    assert _raw(r, **dict(ok, n=0, rays=None, radiance=None)) == 0  # n == 0: OK, nothing launched
    assert r.ray_render_info()["chunks"] == 0
    with pytest.raises(sptr.SptrError):
        r.render_rays(rays, stream=stream.cuda_stream)
    got = r.render_rays(rays, max_depth=6)  # and the context still renders rays
    assert np.isfinite(got).all() and (got > 0).any() and r.ray_render_info()["chunks"] == 1
    r.close()


# ------------------------------------------------------------------------------- 9. sptr_cli --panorama
def _panorama_dirs(w, h):
    """sptr_cli --panorama's directions, as tools/sptr_cli.cpp documents them."""
    f32 = np.float32
    pi = f32(3.14159265358979323846)
    th = pi * (np.arange(h, dtype=f32) + f32(0.5)) / f32(h)
    ph = f32(2.0) * pi * (np.arange(w, dtype=f32) + f32(0.5)) / f32(w)
    st, ct = np.sin(th.astype(np.float64)).astype(f32), np.cos(th.astype(np.float64)).astype(f32)
    sp, cp = np.sin(ph.astype(np.float64)).astype(f32), np.cos(ph.astype(np.float64)).astype(f32)
    d = np.empty((h, w, 3), f32)
    d[..., 0] = st[:, None] * cp[None, :]
    d[..., 1] = ct[:, None]
    d[..., 2] = st[:, None] * sp[None, :]
    return d


@pytest.mark.parametrize("spp", [1, 3])
def test_cli_panorama(tmp_path, spp):
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"
    w, h = 64, 32
    out = tmp_path / "pano.pfm"
    res = subprocess.run([exe, "--scene", "default", "--panorama", str(w), str(h), "--spp", str(spp), "--depth", "6", "--json",
                          "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    with open(out, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == b"%d %d\n" % (w, h) and f.readline() == b"-1.0\n"
        img = np.frombuffer(f.read(), "<f4").reshape(h, w, 3)
    r = sptr.Renderer(0)
    try:
        sptr.setup_default(r, "default")
        cam = sptr.camera_lookat(aspect=800 / 600)  # the tool's camera: (0, 3, 8) -> (0, 1, 0)
        got = r.render_rays(_rays(cam.as_array()[:3], _panorama_dirs(w, h)), samples=spp, frame_index=1, max_depth=6)
        mine = r.ray_render_info()
    finally:
        r.close()
    _equal(img.reshape(-1, 3), got / np.float32(spp), f"sptr_cli --panorama {w} {h} --spp {spp} vs render_rays")
    assert info["panorama"] == [w, h] and info["samples"] == spp and info["chunks"] == 1 and info["ms"] > 0.0
    assert (info["closest"], info["shadow"]) == (mine["closest"], mine["shadow"])
    assert (img[:4] > 0).all() and np.isfinite(img).all()  # (the top rows look at the sky)
