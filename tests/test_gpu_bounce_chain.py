"""The block-local bounce chain (sptr_set_bounce_chain, k_bounce_chain) against the launch per bounce it
replaces (k_bounce01 + k_bounce): every case renders with the chain off (mode 1) and on (mode 2) in this
process and compares the accumulation (as uint32), the resolved image, the shard's resolved tiles and the
query counters for exact equality.  Which block and lane a path runs on must not enter a result, so nothing
here has a tolerance."""
import numpy as np
import pytest

import sptr

pytestmark = pytest.mark.gpu

TILE = 32


class _DevWords:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<i4", "data": (ptr, False), "version": 3}


def _counts(st):
    return (st.rays_closest, st.rays_shadow, st.rays_tail, st.traced_fused, tuple(st.traced_by_depth), st.samples)


def _state(renderer):
    import torch

    ptr, nbytes = renderer.tiles_device()
    tiles = torch.as_tensor(_DevWords(ptr, nbytes), device="cuda").cpu().numpy().copy()
    return renderer.read_accum().copy(), renderer.read_rgb8().copy(), tiles


def _same(a, b, what=""):
    """a, b: lists of (accum, rgb8, tiles, counters) of the two modes."""
    assert len(a) == len(b) and a
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[3] == y[3], (what, i, x[3], y[3])
        assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)), (what, i, "accum")
        assert np.array_equal(x[1], y[1]), (what, i, "rgb8")
        assert np.array_equal(x[2], y[2]), (what, i, "tiles")


def _both(renderer, run, what=""):
    """run() under mode 1 (off) and mode 2 (on); returns the two results after comparing them."""
    out = {}
    try:
        for mode in (1, 2):
            renderer.set_bounce_chain(mode)
            out[mode] = run()
    finally:
        renderer.set_bounce_chain(0)
    _same(out[1], out[2], what)
    return out[1], out[2]


def _one(renderer, cam, W, H, spp, **kw):
    st = renderer.render(cam, W, H, spp=spp, **kw)
    return [_state(renderer) + (_counts(st),)]


# ---- 1. mostly empty blocks ----------------------------------------------------------------------------
@pytest.mark.parametrize("tail,depth", [(0, 6), (6, 6), (0, 1), (0, 2), (0, 3), (32, 32)])
def test_small_batch_depths(renderer, tail, depth):
    """96x64x4 paths over a resident grid: most blocks hold no ray in some phase.  tail 0: the automatic
    tail takes over at bounce 4 (the chain publishes its segment counts for k_tail); tail 6 / 32: the chain
    runs to the last bounce and publishes nothing; depths 1, 2, 3: no chain at all, phase 1 alone, and one
    later phase (with 6: both parities of the ray tables); depth 32: many phases, the late ones empty."""
    W, H = 96, 64
    sptr.setup_default(renderer, "default_emitter")
    cam = sptr.camera_lookat(aspect=W / H)
    try:
        renderer.set_tail_depth(tail)
        off, on = _both(renderer, lambda: _one(renderer, cam, W, H, 4, max_depth=depth), f"tail {tail} depth {depth}")
    finally:
        renderer.set_tail_depth(0)
    c = off[0][3]
    assert c[5] == W * H * 4
    if tail == 0 and depth == 6:
        assert c[2] > 0  # the tail ran
    if tail in (6, 32):
        assert c[2] == 0
    if depth >= 2:
        assert c[3] > 0  # fused bounces traced rays


# ---- 2. several chunks per block -----------------------------------------------------------------------
def test_blocks_loop_in_phases_1_and_2(renderer):
    """640x360x64: more bounce-2 rays than 2048 blocks x 256 threads (2048 is the cap on a resident grid), so
    at least one block runs more than one chunk in phase 2 (and so in phase 1).  (32 spp leaves 358 K rays at
    bounce 2, under the 524 K bound, so the spp is raised.)"""
    W, H, spp = 640, 360, 64
    sptr.setup_default(renderer, "default_emitter")
    cam = sptr.camera_lookat(aspect=W / H)
    off, _ = _both(renderer, lambda: _one(renderer, cam, W, H, spp), "640x360x64")
    assert off[0][3][4][2] > 2048 * 256, off[0][3][4]


# ---- 3. call shapes --------------------------------------------------------------------------------------
SW, SH, SSPP = 320, 200, 8


def _shape_setup(renderer):
    sptr.setup_default(renderer, "default_emitter")
    return sptr.camera_lookat(aspect=SW / SH)


def test_pixel_lanes(renderer):
    cam = _shape_setup(renderer)
    res = {}
    try:
        for lanes in (1, 2):
            renderer.set_pixel_lanes(lanes)

            def run():
                r = _one(renderer, cam, SW, SH, SSPP)
                assert renderer.pixel_lanes_info()["active"] == (lanes == 2)
                return r

            res[lanes] = _both(renderer, run, f"lanes {lanes}")
    finally:
        renderer.set_pixel_lanes(0)
    _same(res[1][0], res[2][1], "one chain of launches vs two lanes with the bounce chain")


def test_every_shard_of_eight(renderer):
    cam = _shape_setup(renderer)
    ntiles = ((SW + TILE - 1) // TILE) * ((SH + TILE - 1) // TILE)
    assert ntiles % 8 != 0  # ragged tile counts

    def run():
        out = []
        for r in range(8):
            out += _one(renderer, cam, SW, SH, SSPP, shard_rank=r, shard_count=8)
        return out

    _both(renderer, run, "8 shards")


def test_async_on_caller_stream(renderer):
    import torch

    cam = _shape_setup(renderer)
    stream = torch.cuda.Stream()

    def run():
        for fb in (1, 1 + SSPP):
            renderer.render(cam, SW, SH, spp=SSPP, frame_begin=fb, flags=sptr.SPTR_FRAME_ASYNC, stream=stream.cuda_stream)
        st = renderer.collect_stats()
        return [_state(renderer) + (_counts(st),)]

    off, _ = _both(renderer, run, "async")
    assert off[0][3][5] == SW * SH * SSPP * 2


def test_graph_replay(renderer):
    """Launch mode 3: a shape's second call is captured, its third replays the graph; the bounce-chain mode
    is part of the graph key, so each mode captures a graph of its own."""
    cam = _shape_setup(renderer)

    def run():
        g0 = renderer.graph_info()
        out = []
        for i in range(3):
            out += _one(renderer, cam, SW, SH, SSPP, frame_begin=1 + i * SSPP)
        g = renderer.graph_info()
        assert g["valid"] == 1 and g["captures"] == g0["captures"] + 1, (g0, g)
        return out

    try:
        renderer.set_launch_mode(3)
        _both(renderer, run, "graph replay")
    finally:
        renderer.set_launch_mode(0)


def test_three_batches(renderer):
    cam = _shape_setup(renderer)
    P = ((SW + TILE - 1) // TILE) * ((SH + TILE - 1) // TILE) * TILE * TILE  # tile-padded pixels of the shard

    def run():
        st = renderer.render(cam, SW, SH, spp=SSPP)
        assert st.waves == 3, st.waves
        return [_state(renderer) + (_counts(st),)]

    try:
        renderer.set_wave_paths(P * 3)
        _both(renderer, run, "three batches")
    finally:
        renderer.set_wave_paths(0)


def test_timing_trace(renderer):
    cam = _shape_setup(renderer)
    launches = []

    def run():
        st = renderer.render(cam, SW, SH, spp=SSPP, flags=sptr.SPTR_FRAME_TIMING_TRACE)
        assert st.ms_trace > 0
        launches.append(st.trace_launches)
        return [_state(renderer) + (_counts(st),)]

    _both(renderer, run, "timing trace")
    assert launches[1] < launches[0], launches


# ---- 4. other kernel instantiations ----------------------------------------------------------------------
def _synthetic_equirect(h=32, w=64):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([0.2 + 0.8 * x / w, 0.3 + 0.7 * y / h, 0.5 + 0.5 * np.sin(x * 0.3) * np.cos(y * 0.2)], axis=-1)
    return img.astype(np.float32)


@pytest.mark.parametrize("case", ["cubemap", "debug", "test_triangle"])
def test_other_instantiations(renderer, case):
    W, H = 96, 64
    cam = sptr.camera_lookat(aspect=W / H)
    faces = sptr.equirect_to_faces(_synthetic_equirect(), 64) if case == "cubemap" else None
    sptr.setup_default(renderer, "test_triangle" if case == "test_triangle" else "default_emitter", env_faces=faces)
    try:
        if case == "debug":
            renderer.set_debug_mode(1)
        off, _ = _both(renderer, lambda: _one(renderer, cam, W, H, 4), case)
    finally:
        renderer.set_debug_mode(0)
        renderer.set_environment(None)
    assert np.abs(off[0][0]).sum() > 0


# ---- 5. the setter ---------------------------------------------------------------------------------------
def test_setter_arguments_and_inapplicable_scene(renderer):
    L = sptr.lib()
    assert L.sptr_set_bounce_chain(None, 1) < 0  # no context
    for bad in (3, 7, 0xFFFFFFFF):
        with pytest.raises(sptr.SptrError):
            renderer.set_bounce_chain(bad)
    for ok in (0, 1, 2, 0):
        renderer.set_bounce_chain(ok)
    # a scene traversed from L2 (wide BVH): the chain does not apply, the launch sequence is the same
    W, H = 96, 64
    sptr.setup_default(renderer, "sphere_mesh", 60, 120)
    cam = sptr.camera_lookat(aspect=W / H)
    launches = []

    def run():
        st = renderer.render(cam, W, H, spp=4, flags=sptr.SPTR_FRAME_TIMING_TRACE)
        launches.append(st.trace_launches)
        return [_state(renderer) + (_counts(st),)]

    off, _ = _both(renderer, run, "sphere_mesh")
    assert len(set(launches)) == 1, launches
    assert off[0][3][3] == 0  # no fused bounce in such a scene
