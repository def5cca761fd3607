"""Shadow entries (sptr_set_shadow_entries, csrc/shadow_entry.h): the table of light-space cells from which the
in-place shadow rays of an LDS-staged scene with one directional light start their walk.

Every case renders with the table forced (mode 2) and without it (mode 0: every shadow ray walks from the
scene's root) and compares the accumulation buffers byte for byte, the ray counters and the per-bounce ray
counts, in a plain call and in the visit-count pass, whose shadow node visits must not grow with the table and
must shrink on default + emitter.  Shapes: 96 x 64 (whole tiles) and 201 x 121 (partial tiles), 16 spp, depth 6."""
import numpy as np
import pytest

import sptr

pytestmark = pytest.mark.gpu

COUNT = sptr.SPTR_FRAME_COUNT_VISITS
SHAPES = [(96, 64), (201, 121)]
SCENES = ["default_emitter", "default"]
SPP, DEPTH = 16, 6
CAMERAS = {"default": ((0.0, 3.0, 8.0), (0.0, 1.0, 0.0)),
           "low, along +x": ((-6.0, 0.6, 0.5), (0.0, 1.0, 0.0)),
           "from above": ((0.5, 9.0, 0.5), (0.0, 0.0, 0.0))}


def _cam(W, H, name="default"):
    pos, target = CAMERAS[name]
    return sptr.camera_lookat(pos=pos, target=target, aspect=W / H)


@pytest.fixture
def r(renderer):
    """The session's renderer, left as it was found: automatic entries, automatic lanes and launch mode,
    a static scene, the default light."""
    try:
        yield renderer
    finally:
        renderer.set_shadow_entries(1)
        renderer.set_pixel_lanes(0)
        renderer.set_launch_mode(0)
        renderer.set_dynamic(False)
        renderer.set_lights(sptr.default_lights())


def _counts(st):
    return (st.rays_closest, st.rays_shadow, list(st.traced_by_depth))


def _both(r, cam, W, H, what, repeats=1, **kw):
    """One plain call and one visit-count call in mode 0 and in mode 2 (the last of `repeats` identical calls
    each); asserts the equalities and returns the shadow node visits (mode 0, mode 2)."""
    got = {}
    for mode in (0, 2):
        r.set_shadow_entries(mode)
        for _ in range(repeats):
            st = r.render(cam, W, H, spp=SPP, max_depth=DEPTH, **kw)
        acc = r.read_accum().copy()
        for _ in range(repeats):
            sv = r.render(cam, W, H, spp=SPP, max_depth=DEPTH, flags=COUNT, **kw)
        got[mode] = (st, acc, sv, r.read_accum().copy())
    (st0, acc0, sv0, accv0), (st2, acc2, sv2, accv2) = got[0], got[2]
    assert st0.rays_shadow > 0, what
    assert np.array_equal(acc0.view(np.uint32), acc2.view(np.uint32)), (what, "accum")
    assert np.array_equal(accv0.view(np.uint32), accv2.view(np.uint32)), (what, "accum, visit-count pass")
    assert np.array_equal(acc0.view(np.uint32), accv0.view(np.uint32)), (what, "accum, plain against visit-count pass")
    assert _counts(st0) == _counts(st2), (what, _counts(st0), _counts(st2))
    assert _counts(sv0) == _counts(sv2), (what, _counts(sv0), _counts(sv2))
    assert (sv0.rays_closest, sv0.rays_shadow) == (st0.rays_closest, st0.rays_shadow), what
    print(f"{what}: shadow rays {sv0.rays_shadow}, shadow node visits {sv0.shadow_node_visits} -> {sv2.shadow_node_visits}, "
          f"prim tests {sv0.shadow_prim_tests} -> {sv2.shadow_prim_tests}")
    assert sv2.shadow_node_visits <= sv0.shadow_node_visits, (what, sv0.shadow_node_visits, sv2.shadow_node_visits)
    return sv0.shadow_node_visits, sv2.shadow_node_visits


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene", SCENES)
def test_identical_to_root_walk(r, scene, shape):
    W, H = shape
    sptr.setup_default(r, scene)
    builds = r.shadow_entries_info()["builds"]
    for name in CAMERAS:
        v0, v2 = _both(r, _cam(W, H, name), W, H, f"{scene} {W}x{H} {name}")
        if scene == "default_emitter":
            assert v2 < v0, (name, v0, v2)
    info = r.shadow_entries_info()
    assert info["mode"] == 2 and info["builds"] == builds + 1, info  # one table serves every camera
    assert info["cells"] > 0 and info["bytes"] == 4 * info["cells"] ** 2 <= 256 << 10, info
    assert 0.0 < info["cells_unoccluded"] <= info["cells_below_root"] <= 1.0, info


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("launch_mode", [0, 1, 3])
def test_lanes_and_launch_modes(r, lanes, launch_mode):
    W, H = SHAPES[1]
    sptr.setup_default(r, "default_emitter")
    r.set_pixel_lanes(lanes)
    r.set_launch_mode(launch_mode)
    # (launch mode 3 captures a repeated call shape on its second call and replays it on the third)
    v0, v2 = _both(r, _cam(W, H), W, H, f"lanes {lanes}, launch mode {launch_mode}", repeats=3 if launch_mode == 3 else 1)
    assert v2 < v0


@pytest.mark.parametrize("shards", [1, 3])
def test_shards(r, shards):
    W, H = SHAPES[1]
    sptr.setup_default(r, "default_emitter")
    for rank in range(shards):
        v0, v2 = _both(r, _cam(W, H), W, H, f"shard {rank} of {shards}", shard_rank=rank, shard_count=shards)
        assert v2 < v0


def test_other_lights_leave_the_table_unused(r):
    W, H = SHAPES[0]
    sptr.setup_default(r, "default_emitter")
    sun = sptr.default_lights()[0]
    point = sptr.Light(1, (2.0, 6.0, 3.0), tuple(sun.color), 40.0)
    for what, lights in (("point light", [point]), ("no light", []), ("sun and point light", [sun, point])):
        r.set_lights(lights)
        r.set_shadow_entries(2)
        builds = r.shadow_entries_info()["builds"]
        got = {}
        for mode in (0, 2):
            r.set_shadow_entries(mode)
            st = r.render(_cam(W, H), W, H, spp=SPP, max_depth=DEPTH)
            acc = r.read_accum().copy()
            sv = r.render(_cam(W, H), W, H, spp=SPP, max_depth=DEPTH, flags=COUNT)
            got[mode] = (_counts(st), acc, _counts(sv), sv.shadow_node_visits, r.read_accum().copy())
        assert got[0][0] == got[2][0] and got[0][2] == got[2][2] and got[0][3] == got[2][3], what
        assert np.array_equal(got[0][1].view(np.uint32), got[2][1].view(np.uint32)), what
        assert np.array_equal(got[0][4].view(np.uint32), got[2][4].view(np.uint32)), what
        assert (got[0][0][1] > 0) == bool(lights), what
        info = r.shadow_entries_info()
        assert info["builds"] == builds and info["cells"] == 0, (what, info)


def test_rebuilt_after_refit_transform_and_light(r):
    W, H = SHAPES[1]
    cam = _cam(W, H)
    r.set_dynamic(True, transforms=True)
    flat = sptr.setup_default(r, "default_emitter")
    r.set_shadow_entries(2)
    _both(r, cam, W, H, "dynamic upload")
    builds = r.shadow_entries_info()["builds"]
    base = r.read_accum().copy()

    def moved(what):
        nonlocal builds, base
        v0, v2 = _both(r, cam, W, H, what)
        info = r.shadow_entries_info()
        assert info["builds"] == builds + 1 and info["cells"] > 0, (what, builds, info)
        builds = info["builds"]
        acc = r.read_accum().copy()
        assert not np.array_equal(acc, base), what  # the change is seen
        base = acc
        assert v2 < v0, what

    sph = flat.spheres.copy()
    sph[0, 0] += 0.7   # one sphere along x ...
    sph[1, 1] += 0.4   # ... and one up: their shadows move across cells
    r.update_geometry(None, sph)
    moved("sphere moved by refit")
    G = len(flat.tri_geom_first) - 1
    xf = np.tile(np.eye(4, dtype=np.float32), (G, 1, 1))
    xf[:, 3, 0] = 0.8  # every triangle geometry along x (xforms[g][col][row])
    sph2 = sph.copy()
    sph2[2, 2] -= 0.6
    r.update_transforms(xf, sph2)
    moved("moved by transform")
    sun = sptr.default_lights()[0]
    r.set_lights([sptr.Light(0, (0.9, -0.35, 0.4), tuple(sun.color), sun.intensity)])  # turned, and low
    moved("light turned")


def test_automatic_mode_builds_nothing_for_small_calls(r):
    W, H = SHAPES[1]
    sptr.setup_default(r, "default_emitter")  # (a new upload: no table is current)
    r.set_shadow_entries(1)
    builds = r.shadow_entries_info()["builds"]
    for scene in SCENES:
        sptr.setup_default(r, scene)
        for name in CAMERAS:
            r.render(_cam(W, H, name), W, H, spp=SPP, max_depth=DEPTH)
            r.render(_cam(W, H, name), W, H, spp=SPP, max_depth=DEPTH, flags=COUNT)
    info = r.shadow_entries_info()
    assert info["mode"] == 1 and info["builds"] == builds and info["cells"] == 0, info


def test_automatic_mode_builds_once_per_upload(r):
    """The automatic mode: the first table after an upload is built by a call of 2^23 samples; a table ended by a
    refit or by another light direction is not replaced by a call of that size (the bound of a rebuild is 2^27),
    which walks from the root and renders what mode 0 renders; a new upload is built for again."""
    W = H = 1024
    spp = 8  # 2^23 samples in one chain
    cam = _cam(W, H)
    r.set_pixel_lanes(1)
    r.set_dynamic(True)
    flat = sptr.setup_default(r, "default_emitter")
    r.set_shadow_entries(1)
    builds = r.shadow_entries_info()["builds"]

    def frame(want_builds, want_table, what):
        st = r.render(cam, W, H, spp=spp, max_depth=DEPTH)
        acc = r.read_accum().copy()
        info = r.shadow_entries_info()
        assert info["builds"] == want_builds and (info["cells"] > 0) == want_table, (what, want_builds, info)
        r.set_shadow_entries(0)
        st0 = r.render(cam, W, H, spp=spp, max_depth=DEPTH)
        assert np.array_equal(acc.view(np.uint32), r.read_accum().view(np.uint32)), what
        assert _counts(st) == _counts(st0), what
        r.set_shadow_entries(1)

    frame(builds + 1, True, "first call after the upload")
    frame(builds + 1, True, "cached")
    sph = flat.spheres.copy()
    sph[0, 0] += 0.7
    r.update_geometry(None, sph)
    frame(builds + 1, False, "after a refit")
    sun = sptr.default_lights()[0]
    r.set_lights([sptr.Light(0, (0.9, -0.35, 0.4), tuple(sun.color), sun.intensity)])
    frame(builds + 1, False, "after the light turned")
    sptr.setup_default(r, "default_emitter")
    frame(builds + 2, True, "after a new upload")


def test_arguments(r):
    L = sptr.lib()
    assert L.sptr_set_shadow_entries(None, 1) < 0
    assert L.sptr_shadow_entries_info(None, None) < 0
    with pytest.raises(sptr.SptrError):
        r.set_shadow_entries(3)
    assert r.shadow_entries_info()["mode"] in (0, 1, 2)
