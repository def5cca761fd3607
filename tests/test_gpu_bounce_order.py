"""The fused bounce launches that shade the previous hit first and then trace (k_shade_trace) against the two
other ways the library runs the same bounces: the separate k_trace / k_shade / k_shadow launches
(SPTR_FRAME_COUNT_VISITS) and the block-local chain (sptr_set_bounce_chain 2: bounce01_path / bounce_ray).
Every case renders one frame the three ways in this process and compares the accumulation buffer (as
uint32), the resolved image, the shard's resolved tiles and the ray counters for exact equality.  Where the
launches are cut, and which block and lane a path runs on, must not enter a result, so nothing here has a
tolerance.

The library runs k_shade_trace for batches of more than 5 x 2^22 paths and the launches it replaced there
(k_bounce01 + k_bounce) for smaller ones (sptr_api.cpp shade_first_on).  Sections 1 to 3 use the smallest
shapes that reach each branch of the launch sequence; their default path is the small-batch one.  Section 4
repeats the branches with one batch just above the threshold, the smallest that k_shade_trace runs on."""
import numpy as np
import pytest

import sptr

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (50, 37)]  # whole tiles; tile slots outside the image and partial waves
SPPS = [1, 5]


class _DevWords:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<i4", "data": (ptr, False), "version": 3}


def _counts(st):
    return (st.rays_closest, st.rays_shadow, tuple(st.traced_by_depth))


def _state(renderer, st):
    import torch

    ptr, nbytes = renderer.tiles_device()
    tiles = torch.as_tensor(_DevWords(ptr, nbytes), device="cuda").cpu().numpy().copy()
    return renderer.read_accum().copy(), renderer.read_rgb8().copy(), tiles, _counts(st), st.traced_fused


def _same(a, b, what):
    assert len(a) == len(b) and a
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[3] == y[3], (what, i, x[3], y[3])
        assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)), (what, i, "accum")
        assert np.array_equal(x[1], y[1]), (what, i, "rgb8")
        assert np.array_equal(x[2], y[2]), (what, i, "tiles")


def _three(renderer, run, what):
    """run(flags) -> list of states; the default fused path, the separate launches, the chain.  Returns the
    default path's states."""
    fused = run(0)
    separate = run(sptr.SPTR_FRAME_COUNT_VISITS)
    try:
        renderer.set_bounce_chain(2)
        chain = run(0)
    finally:
        renderer.set_bounce_chain(0)
    _same(fused, separate, (what, "fused vs separate launches"))
    _same(fused, chain, (what, "fused vs chain"))
    assert all(s[4] == 0 for s in separate)  # the comparison path fused nothing
    return fused


def _frames(renderer, cam_of, what, shapes=SHAPES, spps=SPPS, **kw):
    out = []
    for W, H in shapes:
        cam = cam_of(W, H)
        for spp in spps:
            out += _three(renderer, lambda flags: [_state(renderer, renderer.render(cam, W, H, spp=spp, flags=flags, **kw))],
                          (what, W, H, spp))
    return out


def _default_cam(W, H):
    return sptr.camera_lookat(aspect=W / H)


# ---- 1. depths and the hand-over to the tail ---------------------------------------------------------------
@pytest.mark.parametrize("depth,tail", [(1, 0), (2, 0), (3, 0), (6, 0), (8, 0), (6, 3), (6, 32), (8, 32)])
def test_depths(renderer, depth, tail):
    """Depth 1: no fused launch; 2: the first launch is the closing one; 3: one later launch, Russian
    roulette from its continuation on; 6 and 8 with the automatic tail (from bounce 4: the closing launch
    writes k_tail's rays), with the tail from bounce 3, and without a tail (32: the closing launch is the
    path's last bounce and writes nothing; 8: more bounces than the per-depth statistics hold)."""
    sptr.setup_default(renderer, "default_emitter")
    try:
        renderer.set_tail_depth(tail)
        res = _frames(renderer, _default_cam, f"depth {depth} tail {tail}", max_depth=depth)
    finally:
        renderer.set_tail_depth(0)
    for s in res:
        assert (s[4] > 0) == (depth >= 2), (depth, s[4])  # the fused launches traced rays
        assert sum(s[3][2][depth:]) == 0


# ---- 2. full and empty segments ----------------------------------------------------------------------------
def _box_scene():
    """The default camera inside a closed box of 12 triangles: every ray of every bounce hits."""
    lo, hi = np.array([-20.0, -20.0, -20.0], np.float32), np.array([20.0, 25.0, 20.0], np.float32)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    return sptr.FlatScene(positions=v, indices=idx, tri_geom_first=np.array([0, 12], np.uint32),
                          spheres=np.zeros((0, 4), np.float32), geom_material=np.array([0], np.uint32))


def _far_sphere_scene():
    """One small sphere on the default camera's axis, 60 units away: it covers a few pixels, so almost every
    ray misses, most blocks hold no record and whole launches run on empty streams."""
    pos, target = np.array([0.0, 3.0, 8.0]), np.array([0.0, 1.0, 0.0])
    d = (target - pos) / np.linalg.norm(target - pos)
    c = pos + 60.0 * d
    return sptr.FlatScene(positions=np.zeros((0, 3), np.float32), indices=np.zeros((0, 3), np.uint32),
                          tri_geom_first=np.array([0], np.uint32),
                          spheres=np.array([[c[0], c[1], c[2], 1.0]], np.float32), geom_material=np.array([0], np.uint32))


@pytest.mark.parametrize("tail", [0, 32])
def test_every_ray_hits(renderer, tail):
    renderer.upload_scene(_box_scene())
    renderer.set_materials(sptr.preset_materials(False))
    renderer.set_lights(sptr.default_lights())
    renderer.set_environment(None)
    try:
        renderer.set_tail_depth(tail)
        res = _frames(renderer, _default_cam, f"box tail {tail}")
    finally:
        renderer.set_tail_depth(0)
    for s in res:
        by_depth = s[3][2]
        assert by_depth[1] == by_depth[0] > 0, by_depth  # nothing escapes: bounce 1 traces every path


def test_almost_every_ray_misses(renderer):
    renderer.upload_scene(_far_sphere_scene())
    renderer.set_materials(sptr.preset_materials(False))
    renderer.set_lights(sptr.default_lights())
    renderer.set_environment(None)
    res = _frames(renderer, _default_cam, "far sphere")
    for s in res:
        by_depth = s[3][2]
        assert by_depth[1] * 50 < by_depth[0], by_depth


# ---- 3. call shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
def test_pixel_lanes(renderer, lanes):
    sptr.setup_default(renderer, "default_emitter")
    try:
        renderer.set_pixel_lanes(lanes)
        _frames(renderer, _default_cam, f"lanes {lanes}")
        assert renderer.pixel_lanes_info()["active"] == (lanes == 2)
    finally:
        renderer.set_pixel_lanes(0)


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_launch_modes(renderer, mode):
    """Mode 3: a shape's second call is captured and its third replays the graph, for each of the three ways
    (flags and chain mode are part of the graph key)."""
    sptr.setup_default(renderer, "default_emitter")
    W, H, spp = 50, 37, 5
    cam = _default_cam(W, H)

    def run(flags):
        g0 = renderer.graph_info()
        out = [_state(renderer, renderer.render(cam, W, H, spp=spp, frame_begin=1 + i * spp, flags=flags)) for i in range(3)]
        if mode == 3 and flags == 0:
            g = renderer.graph_info()
            assert g["valid"] == 1 and g["captures"] == g0["captures"] + 1, (g0, g)
        return out

    try:
        renderer.set_launch_mode(mode)
        _three(renderer, run, f"launch mode {mode}")
    finally:
        renderer.set_launch_mode(0)


def test_shard_three_of_eight(renderer):
    """128x64 in place of 64x64: 64x64 is four tiles, and rank 3 of 8 needs a tile of its own to render (the
    tiles are dealt round-robin); 50x37, also four tiles, gives rank 3 its last, partial tile."""
    sptr.setup_default(renderer, "default_emitter")
    _frames(renderer, _default_cam, "shard 3 of 8", shapes=[(128, 64), (50, 37)], shard_rank=3, shard_count=8)


def test_debug_mode(renderer):
    sptr.setup_default(renderer, "default_emitter")
    try:
        renderer.set_debug_mode(1)
        res = _frames(renderer, _default_cam, "debug mode 1")
    finally:
        renderer.set_debug_mode(0)
    assert all(np.abs(s[0]).sum() > 0 for s in res)


# ---- 4. batches that k_shade_trace runs on -----------------------------------------------------------------
SHADE_FIRST_MIN_PATHS = 5 << 22  # sptr_api.cpp kShadeFirstMinPaths
BW, BH, BSPP = 1000, 1010, 21    # 32 x 32 tiles, the right and bottom ones partial: 2^20 pixel slots x 21


def _big(renderer, what, lanes=1, spp=BSPP, **kw):
    """One batch per lane of BW x BH x spp / lanes paths, the three ways."""
    assert 1024 * 1024 * spp // lanes > SHADE_FIRST_MIN_PATHS
    cam = _default_cam(BW, BH)
    try:
        renderer.set_pixel_lanes(lanes)
        return _three(renderer, lambda flags: [_state(renderer, renderer.render(cam, BW, BH, spp=spp, flags=flags, **kw))],
                      what)
    finally:
        renderer.set_pixel_lanes(0)


@pytest.mark.parametrize("depth,tail", [(2, 0), (3, 0), (6, 0), (6, 3), (6, 32), (8, 32)])
def test_big_batch_depths(renderer, depth, tail):
    """As test_depths, on k_shade_trace: the first launch as the closing one (2), one later launch (3), the
    closing launch handing over to k_tail (6 with the automatic tail from bounce 4, and from 3), and the
    closing launch as the path's last bounce (tail 32)."""
    sptr.setup_default(renderer, "default_emitter")
    try:
        renderer.set_tail_depth(tail)
        res = _big(renderer, f"big depth {depth} tail {tail}", max_depth=depth)
    finally:
        renderer.set_tail_depth(0)
    assert res[0][4] > 0 and sum(res[0][3][2][depth:]) == 0


def test_big_batch_every_ray_hits(renderer):
    renderer.upload_scene(_box_scene())
    renderer.set_materials(sptr.preset_materials(False))
    renderer.set_lights(sptr.default_lights())
    renderer.set_environment(None)
    by_depth = _big(renderer, "big box")[0][3][2]
    assert by_depth[1] == by_depth[0] > 0, by_depth


def test_big_batch_almost_every_ray_misses(renderer):
    renderer.upload_scene(_far_sphere_scene())
    renderer.set_materials(sptr.preset_materials(False))
    renderer.set_lights(sptr.default_lights())
    renderer.set_environment(None)
    by_depth = _big(renderer, "big far sphere")[0][3][2]
    assert by_depth[1] * 50 < by_depth[0], by_depth


def test_big_batch_two_lanes(renderer):
    sptr.setup_default(renderer, "default_emitter")
    _big(renderer, "big, two lanes", lanes=2, spp=2 * BSPP)


def test_big_batch_graph_replay(renderer):
    sptr.setup_default(renderer, "default_emitter")
    cam = _default_cam(BW, BH)

    def run(flags):
        return [_state(renderer, renderer.render(cam, BW, BH, spp=BSPP, frame_begin=1 + i * BSPP, flags=flags))
                for i in range(3)]

    try:
        renderer.set_pixel_lanes(1)
        renderer.set_launch_mode(3)
        _three(renderer, run, "big graph replay")
    finally:
        renderer.set_launch_mode(0)
        renderer.set_pixel_lanes(0)


def test_big_batch_debug_mode(renderer):
    sptr.setup_default(renderer, "default_emitter")
    try:
        renderer.set_debug_mode(1)
        res = _big(renderer, "big debug mode 1")
    finally:
        renderer.set_debug_mode(0)
    assert np.abs(res[0][0]).sum() > 0
