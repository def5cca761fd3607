"""The sky split of a lane-group bounce 0 (sptr_set_sky_split, csrc/sky_split.h): the bulk of the culled pixels
summed thread per pixel by k_sky's list mode, the unculled pixels and the culled remainder walked as an item list
by k_trace_wp.  Every case renders with the split off (mode 1, the launch sequence the rest of the suite checks
against the oracle) and on (mode 2) in this process and compares the accumulation (as uint32), the resolved image,
the shard's resolved tiles and the counters for exact equality: which thread sums a pixel must not enter a result,
so nothing here has a tolerance.

Shapes: 16 spp (the smallest batch that takes lane groups), depth 6, default_emitter, 4096 bulk threads, so that
a 256 x 256 frame has more than one culled pixel per bulk thread and a remainder, unless a case says otherwise."""
import numpy as np
import pytest

import adversarial_common as A
import sptr

pytestmark = pytest.mark.gpu

TILE = 32
T_TEST = 4096
SPP = 16
COUNT = sptr.SPTR_FRAME_COUNT_VISITS


class _DevWords:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<i4", "data": (ptr, False), "version": 3}


def _counts(st, visits=False):
    c = (st.rays_closest, st.rays_shadow, st.traced_primary, st.traced_bounce, st.samples)
    if visits:
        c += (st.hits_primary, tuple(st.traced_by_depth))
    return c


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


def _both(renderer, run, what="", threads=T_TEST):
    """run() under mode 1 (off) and mode 2 (on); returns the two results after comparing them."""
    out = {}
    try:
        for mode in (1, 2):
            renderer.set_sky_split(mode, threads)
            out[mode] = run(mode)
    finally:
        renderer.set_sky_split(0, 0)
    _same(out[1], out[2], what)
    return out[1], out[2]


def _one(renderer, cam, W, H, spp=SPP, split=None, flags=0, **kw):
    """One call, then the same call in the visit-count pass.  split: whether the call must have split."""
    out = []
    for count in (0, COUNT):
        st = renderer.render(cam, W, H, spp=spp, max_depth=6, flags=flags | count, **kw)
        if split is not None:
            assert (renderer.sky_split_info()["bulk_threads"] != 0) == split, (split, renderer.sky_split_info())
        out.append(_state(renderer) + (_counts(st, visits=bool(count)),))
    return out


def _cam(W, H, pos=(0.0, 3.0, 8.0), target=(0.0, 1.0, 0.0)):
    return sptr.camera_lookat(pos=pos, target=target, aspect=W / H)


def _cameras(scene, W, H):
    """default; behind (all geometry behind the camera: every pixel culled, no hit record); close (the first
    sphere fills the frame: nothing culled); inside the triangle geometry's box."""
    c, rad, lo, hi = A.bounds({"positions": scene.positions, "indices": scene.indices, "spheres": scene.spheres})
    p = scene.positions[np.unique(scene.indices.astype(np.int64))].astype(np.float64)
    inside = 0.5 * (p.min(axis=0) + p.max(axis=0))
    s = scene.spheres[0].astype(np.float64)
    return {"default": _cam(W, H),
            "behind": _cam(W, H, pos=tuple(c + [0.0, 0.5, 2.5 * rad + 1.0]), target=tuple(c + [0.0, 1.5, 5.0 * rad + 9.0])),
            "close": _cam(W, H, pos=(s[0], s[1], s[2] + 1.05 * s[3] + 1e-3), target=tuple(s[:3])),
            "inside": _cam(W, H, pos=tuple(inside), target=tuple(inside + [0.3, -0.2, -1.0]))}


# ---- 1. frame sizes and cameras --------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(256, 256), (201, 121), (96, 64)])
def test_sizes_and_cameras(renderer, W, H):
    """256 x 256: m > 1 for the cameras that cull most pixels; 201 x 121: partial tiles and quads; 96 x 64: fewer
    culled pixels than bulk threads, m = 0, every pixel an item."""
    scene = sptr.setup_default(renderer, "default_emitter")
    # (96 x 64 holds 6144 pixels, 5096 of them culled from the default camera: 8192 bulk threads give m = 0 for
    # every camera; 4096 give m = 1 with a remainder there, and m = 0 for the close camera)
    for name, cam in _cameras(scene, W, H).items():
        if (W, H) == (96, 64):
            big, _ = _both(renderer, lambda mode: _one(renderer, cam, W, H, split=(mode == 2)), (W, H, name, "m = 0"),
                           threads=2 * T_TEST)
            assert W * H - big[0][3][2] // SPP < 2 * T_TEST  # n_culled < T
        off, on = _both(renderer, lambda mode: _one(renderer, cam, W, H, split=(mode == 2)), (W, H, name))
        traced = off[0][3][2]
        assert traced % SPP == 0 and traced <= W * H * SPP
        culled = W * H - traced // SPP
        if name == "behind":  # no primary hit, so no hit record; (nearly) every pixel culled
            assert off[1][3][5] == 0 and culled >= 0.95 * W * H, (culled, off[1][3][5])
        if name == "close":
            assert culled == 0
        if (W, H) == (256, 256) and name in ("default", "behind"):
            assert culled // T_TEST > 1, culled  # m > 1
        if (W, H) == (256, 256) and name == "default":
            assert culled % T_TEST != 0, culled  # and a remainder of culled pixels for the lane groups
        if (W, H) == (96, 64) and name == "close":
            assert culled < T_TEST  # m = 0 at 4096 threads too


# ---- 2. accumulation -------------------------------------------------------------------------------------
AW, AH = 201, 121


def test_two_calls_accumulate(renderer):
    """The second call continues the first (reset = 0, acc0 = 16): both kernels start from the stored sums."""
    sptr.setup_default(renderer, "default_emitter")
    cam = _cam(AW, AH)

    def run(mode):
        out = []
        for fb in (1, 1 + SPP):
            st = renderer.render(cam, AW, AH, spp=SPP, frame_begin=fb)
            out.append(_state(renderer) + (_counts(st),))
        return out

    off, _ = _both(renderer, run, "two calls")
    assert not np.array_equal(off[0][0], off[1][0])


def test_three_batches(renderer):
    """One call of 48 spp in three batches of 16 (set_wave_paths): each batch splits, the later ones add to
    the earlier ones' sums."""
    sptr.setup_default(renderer, "default_emitter")
    cam = _cam(AW, AH)
    P = ((AW + TILE - 1) // TILE) * ((AH + TILE - 1) // TILE) * TILE * TILE  # tile-padded pixels of the shard

    def run(mode):
        st = renderer.render(cam, AW, AH, spp=3 * SPP)
        assert st.waves == 3, st.waves
        assert (renderer.sky_split_info()["bulk_threads"] != 0) == (mode == 2)
        return [_state(renderer) + (_counts(st),)]

    try:
        renderer.set_wave_paths(P * SPP)
        _both(renderer, run, "three batches")
    finally:
        renderer.set_wave_paths(0)


def test_ragged_last_round(renderer):
    """17 spp: the lane groups' third round holds one sample, the bulk threads' loop a remainder of one."""
    sptr.setup_default(renderer, "default_emitter")
    _both(renderer, lambda mode: _one(renderer, _cam(AW, AH), AW, AH, spp=17, split=(mode == 2)), "17 spp")


# ---- 3. environment ----------------------------------------------------------------------------------------
def _synthetic_equirect(h=32, w=64):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([0.2 + 0.8 * x / w, 0.3 + 0.7 * y / h, 0.5 + 0.5 * np.sin(x * 0.3) * np.cos(y * 0.2)], axis=-1)
    return img.astype(np.float32)


def test_cubemap(renderer):
    """The kCube instantiations of both kernels: the default scene under a synthetic cubemap."""
    faces = sptr.equirect_to_faces(_synthetic_equirect(), 64)
    sptr.setup_default(renderer, "default", env_faces=faces)
    try:
        off, _ = _both(renderer, lambda mode: _one(renderer, _cam(256, 256), 256, 256, split=(mode == 2)), "cubemap")
    finally:
        renderer.set_environment(None)
    assert np.abs(off[0][0]).sum() > 0


# ---- 4. context variants -----------------------------------------------------------------------------------
def test_shard_one_of_two(renderer):
    sptr.setup_default(renderer, "default_emitter")
    _both(renderer, lambda mode: _one(renderer, _cam(256, 256), 256, 256, split=(mode == 2), shard_rank=1, shard_count=2),
          "shard 1 of 2")


def test_two_pixel_lanes(renderer):
    """The setter is forwarded to the pixel lane: each lane splits its own tiles."""
    sptr.setup_default(renderer, "default_emitter")
    try:
        renderer.set_pixel_lanes(2)

        def run(mode):
            r = _one(renderer, _cam(256, 256), 256, 256, split=(mode == 2))
            assert renderer.pixel_lanes_info()["active"]
            return r

        two, _ = _both(renderer, run, "two lanes")
        renderer.set_pixel_lanes(1)
        one, _ = _both(renderer, lambda mode: _one(renderer, _cam(256, 256), 256, 256, split=(mode == 2)), "one chain")
    finally:
        renderer.set_pixel_lanes(0)
    for x, y in zip(one, two):  # one chain of launches against two lanes: the same frame
        assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[2], y[2])


@pytest.mark.parametrize("launch_mode", [0, 1, 3])
@pytest.mark.parametrize("recull", [False, True])
def test_launch_modes_and_camera_switch(renderer, launch_mode, recull):
    """Four calls of one shape, the camera switched before the third: in mode 3 the second call is captured and
    the later ones replay a graph (the camera is part of its key), so a replayed list-mode launch must take the
    counts of its own call's cull from the device.  With SPTR_FRAME_RECULL the cull, and both lists, are made
    inside the call's own sequence (the box cull at this size)."""
    scene = sptr.setup_default(renderer, "default_emitter")
    W, H = 201, 121
    cams = _cameras(scene, W, H)
    order = [cams["default"], cams["default"], cams["behind"], cams["default"], cams["behind"]]
    flags = sptr.SPTR_FRAME_RECULL if recull else 0

    def run(mode):
        out = []
        for i, cam in enumerate(order):
            st = renderer.render(cam, W, H, spp=SPP, frame_begin=1 + i * SPP, flags=flags)
            assert (renderer.sky_split_info()["bulk_threads"] != 0) == (mode == 2)
            out.append(_state(renderer) + (_counts(st),))
        return out

    try:
        renderer.set_launch_mode(launch_mode)
        _both(renderer, run, ("launch mode", launch_mode, recull))
    finally:
        renderer.set_launch_mode(0)


def test_no_cull_does_not_split(renderer):
    """SPTR_FRAME_NO_CULL: there are no lists, so mode 2 keeps the parent's launches."""
    sptr.setup_default(renderer, "default_emitter")
    cam = _cam(256, 256)
    _both(renderer, lambda mode: _one(renderer, cam, 256, 256, split=False, flags=sptr.SPTR_FRAME_NO_CULL), "no cull")


# ---- 5. the automatic grid and the automatic rule ------------------------------------------------------------
def test_automatic_bulk_threads(renderer):
    """bulk_threads = 0: the list mode's own grid (a fraction of its resident threads), 1024 x 576 x 16 spp."""
    scene = sptr.setup_default(renderer, "default_emitter")
    W, H = 1024, 576
    cams = _cameras(scene, W, H)
    for name in ("behind", "default"):
        st0 = {}

        def run(mode):
            st = renderer.render(cams[name], W, H, spp=SPP, max_depth=6)
            st0[mode] = renderer.sky_split_info()["bulk_threads"]
            return [_state(renderer) + (_counts(st),)]

        _both(renderer, run, ("automatic grid", name), threads=0)
        assert st0[1] == 0 and st0[2] >= 256 and st0[2] % 256 == 0, st0


def test_mode_0_leaves_small_batches_alone(renderer):
    """Mode 0 issues no list-mode launch for a 96 x 64 frame or for the 8-way shard of a 1080p frame (fewer
    than two pixels per bulk thread): sptr_sky_split_info reports no split."""
    sptr.setup_default(renderer, "default_emitter")
    renderer.set_sky_split(0, 0)
    renderer.render(_cam(96, 64), 96, 64, spp=SPP, max_depth=6)
    assert renderer.sky_split_info()["bulk_threads"] == 0
    for spp in (SPP, 64):  # (64 spp: the bench's shard, a call large enough for two pixel lanes)
        renderer.render(_cam(1920, 1080), 1920, 1080, spp=spp, max_depth=6, shard_rank=3, shard_count=8)
        assert renderer.sky_split_info()["bulk_threads"] == 0


def test_setter_arguments(renderer):
    L = sptr.lib()
    assert L.sptr_set_sky_split(None, 1, 0) < 0  # no context
    for bad in (3, 7, 0xFFFFFFFF):
        with pytest.raises(sptr.SptrError):
            renderer.set_sky_split(bad, 0)
    for ok in ((0, 0), (1, 0), (2, 4096), (2, 1000), (0, 0)):
        renderer.set_sky_split(*ok)
