"""The exact bounce-0 cull of LDS-staged BVH2 scenes (k_cull<true>, csrc/cull_prims.h) and the per-quad walk
entry words it leaves for the bounce-0 trace kernels.

1. Bit identity against the uncut walk: every case renders with default flags and with SPTR_FRAME_NO_CULL
   (every camera ray walks from the scene's root) and compares the accumulation buffer byte for byte and the
   ray counters; with SPTR_FRAME_COUNT_VISITS also the primary hits and the later bounces' ray counts.
2. Tightness: the unculled pixels of default + emitter at 480 x 270 stay within the quads the primitives
   touch (evaluated here in float64) plus one ring of quads, and within the box cull's count.
3. Entries pay: node visits and primitive tests per traced camera ray are below the box cull's.

Parent figures (the library before this cull, same setup, 480 x 270 x 16 spp, depth 6, measured on an
MI355X): see PARENT_*.  This cull at that shape: 15 528 pixels unculled (touched quads 15 480, plus one ring
17 128), 1.7606 node visits and 4.7347 primitive tests per traced camera ray."""
import numpy as np
import pytest

import adversarial_common as A
import sptr

pytestmark = pytest.mark.gpu

NO_CULL = sptr.SPTR_FRAME_NO_CULL
COUNT = sptr.SPTR_FRAME_COUNT_VISITS
SHAPES = [(201, 121), (96, 64)]  # partial tiles and quads cut by the image edge; whole tiles
SPPS = [1, 16]                   # path-major bounce 0 (k_trace, k_sky); lane groups or thread per pixel

# the library before the exact cull, default_emitter, default camera, 480 x 270, 16 spp, depth 6
PARENT_UNCULLED = 32496          # traced_primary / spp
PARENT_NODES_PER_RAY = 2.8521    # node_visits_primary / traced_primary (2.852186)
PARENT_PRIMS_PER_RAY = 5.7752    # (tri_tests_primary + sphere_tests_primary) / traced_primary (5.775234)


def _cam(W, H, pos=(0.0, 3.0, 8.0), target=(0.0, 1.0, 0.0)):
    return sptr.camera_lookat(pos=pos, target=target, aspect=W / H)


def _counts(st):
    return (st.rays_closest, st.rays_shadow, st.traced_bounce)


def _check_pair(r, cam, W, H, spp, what, **kw):
    """One frame with the cull and its entries, one without; then both again in the visit-count pass."""
    st = r.render(cam, W, H, spp=spp, **kw)
    acc = r.read_accum().copy()
    st0 = r.render(cam, W, H, spp=spp, flags=NO_CULL, **kw)
    acc0 = r.read_accum().copy()
    assert np.array_equal(acc.view(np.uint32), acc0.view(np.uint32)), (what, "accum")
    assert _counts(st) == _counts(st0), (what, _counts(st), _counts(st0))
    assert st.traced_primary <= st0.traced_primary, what
    sv = r.render(cam, W, H, spp=spp, flags=COUNT, **kw)
    accv = r.read_accum().copy()
    sv0 = r.render(cam, W, H, spp=spp, flags=COUNT | NO_CULL, **kw)
    assert np.array_equal(accv.view(np.uint32), acc0.view(np.uint32)), (what, "accum, visit-count pass")
    assert np.array_equal(r.read_accum().view(np.uint32), acc0.view(np.uint32)), (what, "accum, visit-count pass, no cull")
    assert _counts(sv) == _counts(sv0) and _counts(sv)[:2] == _counts(st0)[:2], what  # (fused launches count in traced_fused)
    assert sv.hits_primary == sv0.hits_primary, (what, sv.hits_primary, sv0.hits_primary)
    assert list(sv.traced_by_depth)[1:] == list(sv0.traced_by_depth)[1:], what
    assert sv.hits_primary <= sv.traced_primary, (what, sv.hits_primary, sv.traced_primary)
    assert sv.traced_primary == st.traced_primary, what
    return st, sv


def _scene_cameras(scene, W, H):
    """The default camera; one inside the triangle geometry's box (the glass cube) or at the primitives' centre;
    one at (-6, 1, 0) looking along +x (the sphere row overlaps on screen: ancestor entries); one with all
    geometry behind it; one so close to the first sphere (or first vertex) that it fills the frame."""
    c, rad, lo, hi = A.bounds({"positions": scene.positions, "indices": scene.indices, "spheres": scene.spheres})
    if len(scene.indices):
        p = scene.positions[np.unique(scene.indices.astype(np.int64))].astype(np.float64)
        inside = 0.5 * (p.min(axis=0) + p.max(axis=0))
    else:
        inside = c
    cams = [("default", _cam(W, H)),
            ("inside", _cam(W, H, pos=tuple(inside), target=tuple(inside + [0.3, -0.2, -1.0]))),
            ("along +x", _cam(W, H, pos=(-6.0, 1.0, 0.0), target=(0.0, 1.0, 0.0))),
            ("behind", _cam(W, H, pos=tuple(c + [0.0, 0.5, 2.5 * rad + 1.0]), target=tuple(c + [0.0, 1.5, 5.0 * rad + 9.0])))]
    if len(scene.spheres):
        s = scene.spheres[0].astype(np.float64)
        cams.append(("close", _cam(W, H, pos=(s[0], s[1], s[2] + 1.05 * s[3] + 1e-3), target=tuple(s[:3]))))
    else:
        v = scene.positions[scene.indices[0, 0]].astype(np.float64)
        cams.append(("close", _cam(W, H, pos=(v[0] + 0.01, v[1] + 0.02, v[2] + 0.05), target=tuple(v))))
    # the scene seen whole, and seen along its longest axis from just outside (its primitives in a row)
    cams.append(("framed", _cam(W, H, pos=tuple(c + 4.0 * rad * np.array([0.3, 0.5, 1.0]) / np.linalg.norm([0.3, 0.5, 1.0])),
                                target=tuple(c))))
    ax = int(np.argmax(hi - lo))
    e = np.zeros(3)
    e[ax] = 1.0
    cams.append(("row", _cam(W, H, pos=tuple(c - (0.5 * (hi - lo)[ax] + 3.0) * e), target=tuple(c))))
    return cams


def _flat(case):
    sc = case.scene
    return sptr.FlatScene(sc["positions"], sc["indices"], sc["tri_geom_first"], sc["spheres"], sc["geom_material"])


def _adversarial(fam, name):
    return next(c for c in A.family(fam) if c.name == name)


def _upload(r, name):
    if name in ("default", "default_emitter", "test_triangle"):
        return sptr.setup_default(r, name)
    fam, case = name.split(":")
    flat = _flat(_adversarial(fam, case))
    r.upload_scene(flat)
    r.set_materials(sptr.preset_materials(False))
    r.set_lights(sptr.default_lights())
    r.set_environment(None)
    return flat


SCENES = ["default", "default_emitter", "test_triangle", "spheres:spheres_line", "axis:axis_grid_pos", "axis:axis_box_pos"]


# ---- 1. bit identity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
def test_identical_to_uncut_walk(renderer, scene):
    flat = _upload(renderer, scene)
    assert renderer.scene_layout()["lds_bytes"] > 0 and renderer.scene_layout()["bvh_width"] == 2  # the exact cull's scenes
    culled_some = False
    for W, H in SHAPES:
        for cname, cam in _scene_cameras(flat, W, H):
            for spp in SPPS:
                st, _ = _check_pair(renderer, cam, W, H, spp, (scene, W, H, cname, spp), max_depth=6)
                culled_some = culled_some or st.traced_primary < W * H * spp
    # the cull ran: some camera leaves pixels whose rays are not traced (a scene that is one leaf range is never culled)
    assert culled_some or scene not in ("default", "default_emitter")


@pytest.mark.parametrize("lanes", [1, 2])
def test_pixel_lanes(renderer, lanes):
    sptr.setup_default(renderer, "default_emitter")
    try:
        renderer.set_pixel_lanes(lanes)
        for W, H in SHAPES:
            for pos in ((0.0, 3.0, 8.0), (-6.0, 1.0, 0.0)):
                _check_pair(renderer, _cam(W, H, pos=pos), W, H, 16, ("lanes", lanes, W, H, pos), max_depth=6)
        assert renderer.pixel_lanes_info()["active"] == (lanes == 2)
    finally:
        renderer.set_pixel_lanes(0)


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_launch_modes_and_cached_entries(renderer, mode):
    """Three calls of one shape: the second reuses the cached mask and entries; in mode 3 it is captured and the
    third replays the graph.  Then SPTR_FRAME_RECULL, which recomputes both inside the call's own sequence."""
    sptr.setup_default(renderer, "default_emitter")
    W, H, spp = 201, 121, 16
    cam = _cam(W, H, pos=(-6.0, 1.0, 0.0))
    try:
        renderer.set_launch_mode(mode)
        ref = []
        for i in range(3):
            renderer.render(cam, W, H, spp=spp, frame_begin=1 + i * spp, flags=NO_CULL)
            ref.append(renderer.read_accum().copy())
        culls = 0
        for flags in (0, sptr.SPTR_FRAME_RECULL):
            for i in range(3):
                st = renderer.render(cam, W, H, spp=spp, frame_begin=1 + i * spp, flags=flags)
                culls += st.cull_launches
                assert np.array_equal(renderer.read_accum().view(np.uint32), ref[i].view(np.uint32)), (mode, flags, i)
        assert culls == 1 + 3, culls  # once for the cached key, once per RECULL call
    finally:
        renderer.set_launch_mode(0)


def test_small_recull_call_keeps_the_box_cull(renderer):
    """A call that recomputes its mask in its own sequence (SPTR_FRAME_RECULL) and has fewer than 2^24
    samples keeps the box cull (sptr_api.cpp cull_exact_for): more camera rays traced, the same image; the
    cached key records which cull made the mask, so the next plain call of that camera recomputes it, exact."""
    sptr.setup_default(renderer, "default_emitter")
    W, H, spp = 201, 121, 16
    cam = _cam(W, H)
    assert W * H * spp < 1 << 24
    exact = renderer.render(cam, W, H, spp=spp)
    ref = renderer.read_accum().copy()
    box = renderer.render(cam, W, H, spp=spp, flags=sptr.SPTR_FRAME_RECULL)
    assert np.array_equal(renderer.read_accum().view(np.uint32), ref.view(np.uint32))
    assert box.cull_launches == 1 and box.traced_primary > exact.traced_primary, (box.traced_primary, exact.traced_primary)
    again = renderer.render(cam, W, H, spp=spp)
    assert np.array_equal(renderer.read_accum().view(np.uint32), ref.view(np.uint32))
    assert again.cull_launches == 1 and again.traced_primary == exact.traced_primary
    assert renderer.render(cam, W, H, spp=spp).cull_launches == 0  # cached now


def test_scene_at_the_lds_limit(renderer):
    """The largest triangle scene that is staged into LDS (adversarial_common's staging family): k_cull<true>
    holds the scene's 48 KB beside its 32.5 KB descent stacks, one block per CU."""
    t, _ = A.staging_counts()
    case = _adversarial("staging", f"staging_{t}")
    flat = _flat(case)
    renderer.upload_scene(flat)
    renderer.set_materials(sptr.preset_materials(False))
    renderer.set_lights(sptr.default_lights())
    renderer.set_environment(None)
    lay = renderer.scene_layout()
    assert lay["bvh_width"] == 2 and 47 * 1024 < lay["lds_bytes"] <= A.header_constant("kLdsSceneBytes"), lay
    W, H = 201, 121
    for cname, cam in _scene_cameras(flat, W, H)[-2:]:  # framed, and along the longest axis
        st, _ = _check_pair(renderer, cam, W, H, 16, ("lds limit", cname), max_depth=6)
        assert st.traced_primary < W * H * 16


@pytest.mark.parametrize("shards", [1, 3])
def test_shards(renderer, shards):
    sptr.setup_default(renderer, "default_emitter")
    for W, H in SHAPES:
        for rank in range(shards):
            _check_pair(renderer, _cam(W, H), W, H, 16, ("shards", shards, rank, W, H), max_depth=6, shard_rank=rank,
                        shard_count=shards)


def test_entries_rebuilt_after_geometry_update():
    """A moved scene invalidates the cached entries with the mask: the frame after sptr_update_geometry equals
    the uncut walk of the moved scene, and differs from the frame before."""
    base = sptr.builtin_scene("default_emitter")
    r = sptr.Renderer(0)
    try:
        r.set_dynamic(True)
        r.upload_scene(base)
        r.set_materials(sptr.preset_materials(True))
        r.set_lights(sptr.default_lights())
        r.set_environment(None)
        W, H = 201, 121
        cam = _cam(W, H)
        r.render(cam, W, H, spp=16)
        before = r.read_accum().copy()
        sph = base.spheres.copy()
        sph[:, 0] += 0.75  # the sphere row moves right: pixels culled before are hit now
        sph[:, 1] += 0.25
        r.update_geometry(base.positions, sph)
        st, _ = _check_pair(r, cam, W, H, 16, "after update_geometry", max_depth=6)
        assert st.cull_launches == 1
        assert not np.array_equal(r.read_accum(), before)
    finally:
        r.close()


# ---- 2. tightness, 3. entries pay --------------------------------------------------------------------------
TW, TH, TSPP = 480, 270, 16


def _touched_quads(scene, cam):
    """(TH / 2, TW / 2) bool: the quad holds a pixel one of whose 3 x 3 sub-positions (corners included) hits a
    primitive, in float64: spheres by the discriminant, the axis-aligned cube by slabs."""
    p = scene.positions[np.unique(scene.indices.astype(np.int64))].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    tri = scene.positions[scene.indices.astype(np.int64)].astype(np.float64)  # every triangle lies in a face of that box
    flat = [(np.ptp(tri[:, :, a], axis=1) == 0.0) & ((tri[:, 0, a] == lo[a]) | (tri[:, 0, a] == hi[a])) for a in range(3)]
    assert np.any(flat, axis=0).all() and len(tri) == 12
    o = np.array(cam.pos, np.float64)
    f, rt, up = (np.array(v, np.float64) for v in (cam.forward, cam.right, cam.up))
    u = np.arange(2 * TW + 1) / (2.0 * TW)
    v = np.arange(2 * TH + 1) / (2.0 * TH)
    d = (f[None, None, :] + ((u - 0.5) * 2.0 * cam.half_width)[None, :, None] * rt
         + (-(v - 0.5) * 2.0 * cam.half_height)[:, None, None] * up)
    hit = np.zeros(d.shape[:2], bool)
    for s in scene.spheres.astype(np.float64):
        oc = o - s[:3]
        a, b, c = (d * d).sum(axis=2), (d * oc).sum(axis=2), (oc * oc).sum() - s[3] ** 2
        disc = b * b - a * c
        with np.errstate(invalid="ignore"):
            hit |= (disc >= 0.0) & ((-b + np.sqrt(np.maximum(disc, 0.0))) > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t0, t1).max(axis=2), np.maximum(t0, t1).min(axis=2)
    hit |= (tn <= tf) & (tf > 0.0)
    # lattice point (j, i) = sub-position (i / 2, j / 2) pixels: pixel (x, y) owns lattice points 2x..2x+2, 2y..2y+2
    pix = np.zeros((TH, TW), bool)
    for dj in range(3):
        for di in range(3):
            pix |= hit[dj:dj + 2 * TH:2, di:di + 2 * TW:2]
    return pix.reshape(TH // 2, 2, TW // 2, 2).any(axis=(1, 3))


@pytest.fixture(scope="module")
def tight_frame(renderer):
    scene = sptr.setup_default(renderer, "default_emitter")
    cam = _cam(TW, TH)
    st = renderer.render(cam, TW, TH, spp=TSPP, max_depth=6, flags=COUNT)
    return scene, cam, st


def test_tightness(tight_frame):
    scene, cam, st = tight_frame
    q = _touched_quads(scene, cam)
    ring = q.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sh = np.zeros_like(q)
            ys, yd = (slice(max(dy, 0), q.shape[0] + min(dy, 0)), slice(max(-dy, 0), q.shape[0] + min(-dy, 0)))
            xs, xd = (slice(max(dx, 0), q.shape[1] + min(dx, 0)), slice(max(-dx, 0), q.shape[1] + min(-dx, 0)))
            sh[yd, xd] = q[ys, xs]
            ring |= sh
    bound = 4 * int(ring.sum())
    assert st.traced_primary % TSPP == 0
    unculled = st.traced_primary // TSPP
    print(f"unculled {unculled}; touched quads' pixels {4 * int(q.sum())}, with one ring {bound}; box cull {PARENT_UNCULLED}")
    assert unculled <= bound, (unculled, bound)
    # the exact cull prunes by the box cull's own box tests on its way down, so its unculled set is a subset of
    # the box cull's: their counts, the box cull's pinned from a run of the library before this cull
    assert unculled <= PARENT_UNCULLED, (unculled, PARENT_UNCULLED)
    assert unculled * TSPP >= st.hits_primary  # every hit belongs to an unculled pixel


def test_entries_pay(tight_frame):
    _, _, st = tight_frame
    nodes = st.node_visits_primary / st.traced_primary
    prims = (st.tri_tests_primary + st.sphere_tests_primary) / st.traced_primary
    print(f"per traced camera ray: node visits {nodes:.4f} (box cull {PARENT_NODES_PER_RAY}), "
          f"primitive tests {prims:.4f} (box cull {PARENT_PRIMS_PER_RAY})")
    assert nodes < PARENT_NODES_PER_RAY, (nodes, PARENT_NODES_PER_RAY)
    assert prims < PARENT_PRIMS_PER_RAY, (prims, PARENT_PRIMS_PER_RAY)
