"""Shading data of an LDS-staged scene read from the staged copy: the fused bounce launches (k_shade_trace, or
k_bounce01 / k_bounce on small batches) take a hit's geometry from the scene in LDS and its material index from
the per-primitive table staged beside it (csrc/prim_mat_table.h), where the separate launches
(SPTR_FRAME_COUNT_VISITS: k_trace / k_shade / k_shadow, whose k_shade stages nothing) read the global arrays.
Every value read is a copy of the same word, so each case renders both ways in this process and compares the
accumulation buffer (as uint32), the resolved image, the shard's resolved tiles and the ray counters for exact
equality; nothing here has a tolerance except the one comparison with the CPU oracle, which uses
tests/test_gpu_golden.py's."""
import numpy as np
import pytest

import adversarial_common as A
import oracle
import sptr

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (50, 37)]  # whole tiles; tile slots outside the image and partial waves
SPPS = [1, 5]
BW, BH, BSPP = 1000, 1010, 21  # test_gpu_bounce_order.py's batch just above 5 << 22 paths: k_shade_trace runs
LIM = A.header_constant("kLdsSceneBytes")


class _DevWords:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<i4", "data": (ptr, False), "version": 3}


def _state(renderer, st):
    import torch

    ptr, nbytes = renderer.tiles_device()
    tiles = torch.as_tensor(_DevWords(ptr, nbytes), device="cuda").cpu().numpy().copy()
    counts = (st.rays_closest, st.rays_shadow, tuple(st.traced_by_depth))
    return renderer.read_accum().copy(), renderer.read_rgb8().copy(), tiles, counts, st.traced_fused


def _pair(renderer, cam, W, H, spp, what, **kw):
    """One frame by the default path and by the separate launches; returns the default path's state."""
    fused = _state(renderer, renderer.render(cam, W, H, spp=spp, **kw))
    sep = _state(renderer, renderer.render(cam, W, H, spp=spp, flags=sptr.SPTR_FRAME_COUNT_VISITS, **kw))
    assert sep[4] == 0, what  # the comparison path fused nothing
    assert fused[3] == sep[3], (what, fused[3], sep[3])
    assert np.array_equal(fused[0].view(np.uint32), sep[0].view(np.uint32)), (what, "accum")
    assert np.array_equal(fused[1], sep[1]), (what, "rgb8")
    assert np.array_equal(fused[2], sep[2]), (what, "tiles")
    return fused


def _cam(W, H):
    return sptr.camera_lookat(aspect=W / H)


def _frames(renderer, what, shapes=SHAPES, spps=SPPS, **kw):
    return [_pair(renderer, _cam(W, H), W, H, spp, (what, W, H, spp), **kw) for W, H in shapes for spp in spps]


# ---- scenes and materials ----------------------------------------------------------------------------------
def _mat(albedo, metallic=0.0, roughness=0.5, emission=(0.0, 0.0, 0.0), ior=1.0):
    m = sptr.Material()
    m.albedo[:] = albedo
    m.metallic, m.roughness, m.ior, m.type = metallic, roughness, ior, 0
    m.emission[:] = emission
    return m


def _materials(n):
    """n materials that shade differently: diffuse colours, with a metal, a glass and an emitter among the first."""
    out = []
    for i in range(n):
        c = (0.15 + 0.8 * ((i * 5) % 7) / 6.0, 0.15 + 0.8 * ((i * 3) % 5) / 4.0, 0.15 + 0.8 * ((i * 2) % 3) / 2.0)
        if i == 1:
            out.append(_mat(c, metallic=1.0, roughness=0.2))
        elif i == 3:
            out.append(_mat(c, ior=1.5))
        elif i == 4:
            out.append(_mat(c, emission=(2.0, 1.5, 1.0)))
        else:
            out.append(_mat(c))
    return out


def _quad(x0, x1, y0, y1, z):
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def _scene(quads, spheres, geom_material):
    """Triangle geometries (one quad each; a floor first) and spheres in front of the default camera."""
    pos, idx, first = [], [], [0]
    floor = np.array([[-8, 0, -8], [8, 0, -8], [8, 0, 6], [-8, 0, 6]], np.float32)
    parts = [(floor, np.array([[0, 2, 1], [0, 3, 2]], np.uint32))] + [_quad(*q) for q in quads]
    nv = 0
    for v, i in parts:
        pos.append(v)
        idx.append(i + nv)
        nv += len(v)
        first.append(first[-1] + len(i))
    return sptr.FlatScene(positions=np.concatenate(pos), indices=np.concatenate(idx),
                          tri_geom_first=np.array(first, np.uint32),
                          spheres=np.array(spheres, np.float32).reshape(-1, 4),
                          geom_material=np.array(geom_material, np.uint32))


QUADS = [(-3.5, -1.5, 0.0, 2.5, -2.0), (-1.0, 1.0, 0.5, 3.0, -3.0), (1.5, 3.5, 0.0, 2.5, -2.0)]
SPHERES = [(-2.0, 0.8, 1.0, 0.8), (0.0, 1.0, 0.5, 1.0), (2.2, 0.6, 1.5, 0.6)]
# 4 triangle geometries then 3 spheres; material order differs from geometry order; geometry 2's index is out
# of range of the 7 materials, so it takes getMaterialFromHit's fallback (its geomID as the index)
MIXED_MATS = [5, 2, 99, 0, 4, 1, 3]


def _mixed():
    return _scene(QUADS, SPHERES, MIXED_MATS)


def _setup(renderer, scene, mats):
    renderer.upload_scene(scene)
    renderer.set_materials(mats)
    renderer.set_lights(sptr.default_lights())
    renderer.set_environment(None)


def _grid(n_tris, n_geoms):
    """n_tris small triangles on a wall facing the default camera, dealt to n_geoms geometries in runs."""
    cols = 32
    k = np.arange(n_tris)
    x0 = -5.0 + 10.0 * (k % cols) / cols
    y0 = 0.2 + 5.0 * (k // cols) / (n_tris // cols + 1)
    dx, dy = 10.0 / cols * 0.9, 5.0 / (n_tris // cols + 1) * 0.9
    z = np.full(n_tris, -1.0)
    pos = np.stack([np.stack([x0, y0, z], 1), np.stack([x0 + dx, y0, z], 1), np.stack([x0, y0 + dy, z], 1)], 1)
    first = np.linspace(0, n_tris, n_geoms + 1).astype(np.uint32)
    return sptr.FlatScene(positions=pos.reshape(-1, 3).astype(np.float32),
                          indices=np.arange(3 * n_tris, dtype=np.uint32).reshape(-1, 3), tri_geom_first=first,
                          spheres=np.zeros((0, 4), np.float32),
                          geom_material=(np.arange(n_geoms, dtype=np.uint32) * 3) % n_geoms)


def _hits(state):
    return state[3][2][1]  # bounce 1 traced rays: bounce 0 hit something and its shading continued


def _fused_hits(res):
    """Every default-path render ran the fused launches (without a table the library would quietly run the
    separate ones, and the two renders of a pair would be one path) and shaded hits."""
    return all(s[4] > 0 and _hits(s) > 0 for s in res)


def _same_images(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and
                                    np.array_equal(x[1], y[1]) for x, y in zip(a, b))


# ---- 1. mixed scene: depths, tail, shard, oracle -----------------------------------------------------------
@pytest.mark.parametrize("depth,tail", [(2, 0), (6, 0), (6, 3)])
def test_mixed_scene(renderer, depth, tail):
    """Depth 2: the first fused launch is the closing one; 6: first, later and closing; tail 3 hands over to
    k_tail on the staged scene."""
    _setup(renderer, _mixed(), _materials(7))
    try:
        renderer.set_tail_depth(tail)
        res = _frames(renderer, f"mixed depth {depth} tail {tail}", max_depth=depth)
        if tail:  # k_tail's shading has the fused launches' as its reference: without a tail (32) they shade every bounce
            renderer.set_tail_depth(32)
            assert _same_images(res, _frames(renderer, f"mixed depth {depth}, no tail", max_depth=depth))
    finally:
        renderer.set_tail_depth(0)
    assert _fused_hits(res)


@pytest.mark.parametrize("rank", [0, 1])
def test_mixed_scene_two_way_shard(renderer, rank):
    _setup(renderer, _mixed(), _materials(7))
    assert _fused_hits(_frames(renderer, f"mixed shard {rank} of 2", shard_rank=rank, shard_count=2))


def test_mixed_scene_against_oracle(renderer):
    """64x64, 4 spp, depth 6 against the CPU oracle's image of the same scene, materials and light, under
    test_gpu_golden.py's tolerances (_image_close's defaults: 0.999 of the pixels exact, relative L1 1e-3)."""
    scene, mats = _mixed(), _materials(7)
    _setup(renderer, scene, mats)
    W = H = 64
    cam = _cam(W, H)
    got = _pair(renderer, cam, W, H, 4, "mixed oracle")
    P = oracle.Prepared({"positions": scene.positions, "indices": scene.indices, "tri_geom_first": scene.tri_geom_first,
                         "spheres": scene.spheres, "geom_material": scene.geom_material}, bvh=True)
    oacc, orgb, _ = P.render(cam.as_array(), W, H, sptr.materials_as_array(mats),
                             sptr.lights_as_array(sptr.default_lights()), frames=4, threads=4)
    acc, rgb = got[0], got[1]
    frac = float((rgb == orgb).all(axis=2).mean())
    m = np.isfinite(acc) & np.isfinite(oacc)
    rel = float(np.abs(acc[m] - oacc[m]).sum() / max(1e-12, np.abs(oacc[m]).sum()))
    print(f"mixed scene vs oracle: exact-pixel fraction {frac:.5f}, relative L1 {rel:.3e}")
    assert (np.isfinite(acc) != np.isfinite(oacc)).sum() <= 3
    assert frac >= 0.999, frac
    assert rel <= 1e-3, rel


# ---- 2. one kind of primitive ------------------------------------------------------------------------------
def test_spheres_only(renderer):
    s = sptr.FlatScene(positions=np.zeros((0, 3), np.float32), indices=np.zeros((0, 3), np.uint32),
                       tri_geom_first=np.array([0], np.uint32), spheres=np.array(SPHERES, np.float32),
                       geom_material=np.array([2, 0, 1], np.uint32))
    _setup(renderer, s, _materials(3))
    assert _fused_hits(_frames(renderer, "spheres only"))


def test_triangles_only(renderer):
    _setup(renderer, _scene(QUADS, [], [3, 1, 0, 2]), _materials(4))
    assert _fused_hits(_frames(renderer, "triangles only"))


# ---- 3. more materials than are staged ---------------------------------------------------------------------
def test_thirty_three_materials(renderer):
    """33 materials: indices 0..31 are staged, 32 is read from global memory (the sh.mats path).  The floor, the
    largest thing in view, has index 32."""
    _setup(renderer, _scene(QUADS, SPHERES, [32, 31, 7, 0, 32, 16, 4]), _materials(33))
    assert _fused_hits(_frames(renderer, "33 materials"))


# ---- 4. the table follows the materials and the scene ------------------------------------------------------
def test_set_materials_then_new_upload(renderer):
    """geom_material [9, 8, 7, 6, 5, 4, 3] with 10 materials maps directly; with 3 every index is out of range
    and falls back to geomID % 3, so the table changes with set_materials alone.  Then another scene is uploaded
    into the same renderer."""
    scene = _scene(QUADS, SPHERES, [9, 8, 7, 6, 5, 4, 3])
    _setup(renderer, scene, _materials(10))
    ten = _frames(renderer, "10 materials")
    renderer.set_materials(_materials(3))
    three = _frames(renderer, "3 materials")
    assert not np.array_equal(ten[0][1], three[0][1])
    renderer.upload_scene(_scene(QUADS[:2], SPHERES[:1], [1, 2, 0, 1]))
    again = _frames(renderer, "new upload")
    assert not np.array_equal(again[0][1], three[0][1])
    # and the first state again: the same images as at the start
    renderer.upload_scene(scene)
    renderer.set_materials(_materials(10))
    back = _frames(renderer, "10 materials again")
    assert _same_images(ten, back)
    assert all(_fused_hits(r) for r in (ten, three, again, back))


def test_set_materials_with_two_lanes(renderer):
    """The pixel lane renders its own build of the scene with its own table, which follows the owner's
    set_materials: two lanes active before the upload, then the 10 -> 3 change of the fallback mapping, on a
    batch large enough for the two lanes to run."""
    scene = _scene(QUADS, SPHERES, [9, 8, 7, 6, 5, 4, 3])
    cam = _cam(BW, BH)
    try:
        renderer.set_pixel_lanes(2)
        _setup(renderer, scene, _materials(10))
        ten = _pair(renderer, cam, BW, BH, 2 * BSPP, "two lanes, 10 materials")
        assert renderer.pixel_lanes_info()["active"]
        renderer.set_materials(_materials(3))
        three = _pair(renderer, cam, BW, BH, 2 * BSPP, "two lanes, 3 materials")
        assert renderer.pixel_lanes_info()["active"]
        renderer.set_pixel_lanes(1)
        one = _pair(renderer, cam, BW, BH, 2 * BSPP, "one lane, 3 materials")
    finally:
        renderer.set_pixel_lanes(0)
    assert _fused_hits([ten, three, one])
    assert not np.array_equal(ten[1], three[1])
    assert np.array_equal(three[1], one[1])  # (the accumulators differ in how the batches are cut, the image does not)


def test_bvh_width_changed_after_upload(renderer):
    """set_bvh_width after the upload decides anew whether the scene is a staged BVH2, the form the fused launches
    run on: width 4 does not fuse, back at 2 the bounces fuse again, with a table."""
    try:
        renderer.set_bvh_width(4)
        _setup(renderer, _mixed(), _materials(7))
        assert renderer.scene_layout()["bvh_width"] == 4
        wide = _frames(renderer, "width 4")
        assert all(s[4] == 0 and _hits(s) > 0 for s in wide)
        renderer.set_bvh_width(2)
        assert renderer.scene_layout()["bvh_width"] == 2
        assert _fused_hits(_frames(renderer, "width 2 after the upload"))
    finally:
        renderer.set_bvh_width(0)


def test_dynamic_scene(renderer):
    """After update_geometry (a refit in place) and after update_transforms (per-geometry matrices)."""
    scene, mats = _mixed(), _materials(7)
    try:
        renderer.set_dynamic(True, transforms=True)
        _setup(renderer, scene, mats)
        rest = _frames(renderer, "dynamic, rest pose")
        moved = scene.positions.copy()
        moved[4:, 1] += 0.5  # every quad up; the floor stays
        sph = scene.spheres.copy()
        sph[:, 0] += 0.3
        renderer.update_geometry(moved, sph)
        up = _frames(renderer, "dynamic, update_geometry")
        assert not np.array_equal(up[0][1], rest[0][1])
        xf = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
        xf[2, 3, 0] = 1.0  # geometry 2 one unit along x (xforms[g][col][row])
        renderer.update_transforms(xf, scene.spheres)
        tr = _frames(renderer, "dynamic, update_transforms")
        assert not np.array_equal(tr[0][1], up[0][1])
        assert all(_fused_hits(r) for r in (rest, up, tr))
    finally:
        renderer.set_dynamic(False)


# ---- 5. around the staging limits --------------------------------------------------------------------------
def _staged_bytes(n):
    return A.staged_bytes(n, n, 0, n)


def _table_bytes(n):
    return (4 * n + 15) // 16 * 16


T_STAGED = max(n for n in range(1, 2000) if _staged_bytes(n) <= LIM)                  # largest scene staged as a BVH2
T_TABLE = max(n for n in range(1, 2000) if _staged_bytes(n) + _table_bytes(n) <= LIM)  # ... with its table in LDS


def _grid_case(renderer, n):
    """Upload the n-triangle wall, check scene_layout() against scene_view's formula, render both ways."""
    _setup(renderer, _grid(n, 7), _materials(7))
    lay = renderer.scene_layout()
    assert lay["num_prim_refs"] == n
    total = lay["node_bytes"] + 48 * n + (n + 3) // 4 * 16
    assert lay["lds_bytes"] == (total if total <= LIM else 0), lay
    assert lay["bvh_width"] == (2 if n <= T_STAGED else 4), lay
    res = _frames(renderer, f"grid {n}")
    assert all(_hits(s) > 0 for s in res)
    assert all((s[4] > 0) == (n <= T_STAGED) for s in res)  # the bounces fuse on a staged BVH2 only
    return lay


@pytest.mark.parametrize("n", [T_TABLE, T_TABLE + 1, T_STAGED, T_STAGED + 1],
                         ids=["table-in-lds", "table-global", "largest-bvh2", "first-bvh4"])
def test_staging_limits(renderer, n):
    """Triangles only: the largest scene whose material table is staged beside it and the first whose table stays
    in global memory (the scene itself still staged); the largest scene staged as a BVH2, the one the fused
    kernels shade from LDS, and the next, which the library stages as a BVH4 and does not fuse."""
    assert T_TABLE < T_STAGED
    lay = _grid_case(renderer, n)
    assert lay["lds_bytes"] != 0
    if n <= T_STAGED:
        assert lay["lds_bytes"] == _staged_bytes(n)


def test_staged_or_not(renderer):
    """The largest triangle count that is staged at all and the next, which is traversed from global memory:
    found by bisection on scene_layout()'s lds_bytes between the first BVH4 scene and a scene whose triangle
    records and references alone exceed the limit."""
    lo, hi = T_STAGED + 1, LIM // 52 + 1

    def staged(n):
        renderer.upload_scene(_grid(n, 7))
        return renderer.scene_layout()["lds_bytes"] != 0

    assert staged(lo) and not staged(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if staged(mid):
            lo = mid
        else:
            hi = mid
    assert _grid_case(renderer, lo)["lds_bytes"] != 0
    assert _grid_case(renderer, hi)["lds_bytes"] == 0


# ---- 6. a batch that k_shade_trace runs on -----------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
def test_big_batch(renderer, lanes):
    """First, later and closing instantiations on one batch per lane just above 5 << 22 paths."""
    spp = BSPP * lanes
    assert 1024 * 1024 * spp // lanes > (5 << 22)
    _setup(renderer, _mixed(), _materials(7))
    try:
        renderer.set_pixel_lanes(lanes)
        s = _pair(renderer, _cam(BW, BH), BW, BH, spp, f"big batch, {lanes} lane(s)")
        assert renderer.pixel_lanes_info()["active"] == (lanes == 2)
    finally:
        renderer.set_pixel_lanes(0)
    assert s[4] > 0 and _hits(s) > 0
