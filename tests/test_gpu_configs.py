"""GPU parity on the BASELINE configurations the other suites only cover at reduced shape:

  C3  rattan chair glTF (6116 tris) + the synthetic HDR environment (written as Radiance .hdr, read
      back through the product's reader, equirect -> 512^2 cube faces), rendered vs the oracle fed
      the same flat scene and faces;
  C4  3840x2160: pixel/tile indexing and the 8-way interleaved shard union at full 4K size, and the
      whole 4K frame (2 spp) vs the oracle;
  C5  the 10M-triangle sphere mesh at full tessellation (1250 x 4000; BVH height ~41, BVH4 traversed
      from HBM): first hits on camera + random rays and a small render vs the oracle with its own BVH.

Tolerances as in test_gpu_parity.py's docstring (bit-exact first hits >= 99.99 %, images >= 99.9 %
exact RGB8 pixels and relative L1 <= 1e-3; the 10M-triangle mesh allows the grazing-ray residue of
its degenerate pole triangles, 99.95 % hits and 99.5 % pixels)."""
import os

import numpy as np
import pytest

import oracle
import residue
import sptr
import workloads

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)


def _image_close(rgb, orgb, acc, oacc, exact_frac=0.999, rel_l1=1e-3):
    frac = float((rgb == orgb).all(axis=2).mean())
    fin, ofin = np.isfinite(acc), np.isfinite(oacc)
    assert (fin != ofin).sum() <= max(3, 1e-6 * fin.size), "non-finite pixels differ"
    m = fin & ofin
    rel = float(np.abs(acc[m] - oacc[m]).sum() / max(1e-12, np.abs(oacc[m]).sum()))
    assert frac >= exact_frac, f"exact-pixel fraction {frac}"
    assert rel <= rel_l1, f"relative L1 {rel}"
    return frac, rel


def _camera_rays(cam, W, H, acc=1):
    d, _ = oracle.primary(cam.as_array(), W, H, acc)
    rays = np.zeros((W * H, 8), np.float32)
    rays[:, 0:3] = np.broadcast_to(cam.as_array()[:3], d.shape).reshape(-1, 3)
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 7] = np.inf
    return rays


def _random_rays(n, seed, lo, hi):
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = g.uniform(lo, hi, size=(n, 3))
    rays[:, 3:6] = d
    rays[:, 7] = np.inf
    return rays


def _flat_dict(flat):
    return {k: getattr(flat, k) for k in ("positions", "indices", "tri_geom_first", "spheres", "geom_material")}


# --------------------------------------------------------------------------------------------- C3
def test_c3_chair_hdr_vs_oracle(renderer):
    wl = workloads.WORKLOADS["c3"]
    import tempfile

    faces = workloads.hdr_env_faces()  # synthetic sky -> .hdr -> product reader -> product cube faces
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "sky.hdr")
        workloads.write_hdr(p, workloads.synthetic_sky_equirect())
        e = sptr.load_hdr(p)
    assert np.array_equal(oracle.equirect_to_faces(e, 512), faces)  # the oracle's own equirect mapping agrees
    flat = sptr.setup_default(renderer, wl.scene, wl.p0, wl.p1, env_faces=faces)
    assert len(flat.indices) == 6116 and list(flat.geom_material) == [7]  # one chair mesh, Wood
    P = oracle.Prepared(_flat_dict(flat), bvh=True)
    # first hits: camera rays and random rays from around the chair
    cam = sptr.camera_lookat(aspect=1.0)
    lo, hi = flat.positions.min(0), flat.positions.max(0)
    rays = np.concatenate([_camera_rays(cam, 160, 160), _random_rays(60000, 3, lo - 0.3, hi + 0.3)])
    g, pr, t, ng = renderer.intersect(rays)
    og, opr, ot, ong = P.intersect(rays)
    same = (g == og) & (pr == opr)
    assert same.mean() >= 0.9999, same.mean()
    h = same & (og != 0xFFFFFFFF)
    assert h.sum() > 3000
    assert np.array_equal(t[h].view(np.uint32), ot[h].view(np.uint32))
    # the C3 render path (HDR cubemap miss shading, Wood material, one sun) at 128x72 x 4 spp
    W, H, S = 128, 72, 4
    cam = sptr.camera_lookat(aspect=W / H)
    st = renderer.render(cam, W, H, spp=S)
    rgb, acc = renderer.read_rgb8(), renderer.read_accum()
    oacc, orgb, ocnt = P.render(cam.as_array(), W, H, oracle.preset_materials(False), oracle.default_lights(),
                                frames=S, env_faces=faces, threads=THREADS)
    _image_close(rgb, orgb, acc, oacc)
    assert st.samples == ocnt["samples"] == W * H * S
    assert abs(int(st.rays_closest) - ocnt["rays_closest"]) <= 1e-3 * ocnt["rays_closest"]
    renderer.set_environment(None)


def test_c3_batches_bit_exact(renderer):
    """C3's L2-resident BVH4 + cubemap in one 32-sample batch: bit-identical to 8-sample batches, and
    close to the oracle."""
    wl = workloads.WORKLOADS["c3"]
    faces = workloads.hdr_env_faces()
    flat = sptr.setup_default(renderer, wl.scene, wl.p0, wl.p1, env_faces=faces)
    W, H, S = 96, 64, 32
    cam = sptr.camera_lookat(aspect=W / H)
    try:
        st = renderer.render(cam, W, H, spp=S)
        assert st.waves == 1
        acc, rgb = renderer.read_accum().copy(), renderer.read_rgb8().copy()
        renderer.set_wave_paths(3 * 2 * 1024 * 8)
        st8 = renderer.render(cam, W, H, spp=S)
        assert st8.waves == S // 8
        assert (st8.rays_closest, st8.rays_shadow) == (st.rays_closest, st.rays_shadow)
        assert np.array_equal(acc.view(np.uint32), renderer.read_accum().view(np.uint32))
        assert np.array_equal(rgb, renderer.read_rgb8())
    finally:
        renderer.set_wave_paths(0)
    P = oracle.Prepared(_flat_dict(flat), bvh=True)
    oacc, orgb, ocnt = P.render(cam.as_array(), W, H, oracle.preset_materials(False), oracle.default_lights(),
                                frames=S, env_faces=faces, threads=THREADS)
    _image_close(rgb, orgb, acc, oacc)
    renderer.set_environment(None)


# --------------------------------------------------------------------------------------------- C4
@pytest.fixture(scope="module")
def c4_frame(renderer):
    W, H, S = 3840, 2160, 2
    sptr.setup_default(renderer, "default")
    cam = sptr.camera_lookat(aspect=W / H)
    st = renderer.render(cam, W, H, spp=S)
    return cam, st, renderer.read_rgb8().copy(), renderer.read_accum().copy()


def test_c4_4k_vs_oracle(renderer, c4_frame):
    cam, st, rgb, acc = c4_frame
    P = oracle.Prepared(oracle.builtin_scene("default"), bvh=True)
    oacc, orgb, ocnt = P.render(cam.as_array(), 3840, 2160, oracle.preset_materials(False), oracle.default_lights(),
                                frames=2, threads=THREADS)
    _image_close(rgb, orgb, acc, oacc)
    assert st.samples == ocnt["samples"] == 3840 * 2160 * 2
    assert abs(int(st.rays_closest) - ocnt["rays_closest"]) <= 1e-4 * ocnt["rays_closest"]


def test_c4_4k_pixel_indexing(renderer, c4_frame):
    """Raygen at 4K: directions and RNG states of every pixel bit-exact (pixel_seed = y*W + x spans
    8.3M values; the camera's (x + jx) / W divisions at W = 3840)."""
    cam, _, _, _ = c4_frame
    d, r = renderer.primary_rays(cam, 3840, 2160, 1024)
    od, orr = oracle.primary(cam.as_array(), 3840, 2160, 1024)
    assert np.array_equal(r, orr)
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32))


def test_c4_8way_shard_union(renderer, c4_frame):
    """The C4 multi-GPU schedule at full size: 8 interleaved tile shards, each rank's resolved tiles
    packed as the gather to rank 0 sends them, unpacked on rank 0 == the one-GPU frame, byte for byte."""
    cam, st0, rgb0, _ = c4_frame
    G, W, H = 8, 3840, 2160
    tpr = sptr.tiles_per_rank(W, H, G)
    gathered = np.zeros(G * tpr * 1024, np.uint32)
    samples = rays = 0
    for r in range(G):
        s = renderer.render(cam, W, H, spp=2, shard_rank=r, shard_count=G)
        samples += s.samples
        rays += s.rays_closest + s.rays_shadow
        gathered[r * tpr * 1024:(r + 1) * tpr * 1024] = sptr.pack_tiles(renderer.read_rgb8(), G, r)
    assert samples == W * H * 2
    assert rays == st0.rays_closest + st0.rays_shadow
    assert np.array_equal(sptr.unpack_tiles(gathered, G, W, H), rgb0)


# --------------------------------------------------------------------------------------------- C5
@pytest.fixture(scope="module")
def c5_scene(renderer):
    wl = workloads.WORKLOADS["c5"]
    flat = sptr.setup_default(renderer, wl.scene, wl.p0, wl.p1)
    P = oracle.Prepared(oracle.builtin_scene("sphere_mesh", wl.p0, wl.p1), bvh=True)
    return flat, P


def _c5_fan_rows(flat, geom, prim):
    """First hits on the two fan rows of the sphere mesh (SceneDesc.h:265-275: stack rows 0 and
    stacks-1 meet at the poles; their triangles are slivers, half of them degenerate up to the
    rounding of sin(pi)), where a ray grazes several triangles at (nearly) the same distance."""
    wl = workloads.WORKLOADS["c5"]
    first = np.asarray(flat.tri_geom_first)
    mesh = int(np.argmax(np.diff(first)))  # the 10M-triangle geometry
    row = prim.astype(np.int64) // (2 * wl.p1)
    return (geom == mesh) & ((row == 0) | (row == wl.p0 - 1))


_log_parity = residue.log_parity


def test_c5_deep_bvh_first_hits(renderer, c5_scene):
    """First hits and occlusion on the full 10M-triangle mesh vs the oracle (its own SAH BVH).  Every
    mismatch is classified: (a) a first hit on the mesh's pole fan rows (_c5_fan_rows) on either side,
    or (b) a tie — both sides hit at the same t bits, and the two BVHs test the tied primitives in a
    different order.  SURVEY.md §8(c)'s 99.99 % first-hit identity is asserted on all other rays; the
    measured fractions are logged (tests/README: SPTR_PARITY_LOG)."""
    flat, P = c5_scene
    lay, info = renderer.scene_layout(), renderer.scene_info()
    assert lay["num_tris"] == 10_000_000 and info["prims"] == 10_000_000 + 8
    assert lay["bvh_width"] == 4 and lay["lds_bytes"] == 0  # BVH4 from HBM
    assert info["depth"] >= 40  # the deep-BVH stress this config exists for
    assert 3 * ((info["depth"] - 1) // 2 + 1) <= 96  # within the BVH4 stack bound (sptr_internal.h kStack)
    cam = sptr.camera_lookat(aspect=16 / 9)
    rays = np.concatenate([_camera_rays(cam, 384, 216), _random_rays(120000, 9, (-1.5, 0.2, 0.5), (1.5, 3.0, 3.5))])
    g, pr, t, ng = renderer.intersect(rays)
    og, opr, ot, ong = P.intersect(rays)
    same = (g == og) & (pr == opr)
    hit = (g != 0xFFFFFFFF) & (og != 0xFFFFFFFF)
    fan = _c5_fan_rows(flat, g, pr) | _c5_fan_rows(flat, og, opr)
    tie = hit & (t.view(np.uint32) == ot.view(np.uint32))
    mism = ~same
    rest = ~(mism & (fan | tie))
    h = same & (og != 0xFFFFFFFF)
    # any-hit shadow queries through the same deep tree (order-independent: no tie class)
    sh = rays[::4].copy()
    sh[:, 6] = 1e-4
    occ, oocc = renderer.occluded(sh), P.occluded(sh)
    occ_fan = fan[::4]
    rec = {"rays": int(len(rays)), "hits": int(h.sum()), "identity_all": float(same.mean()),
           "mismatch": int(mism.sum()), "mismatch_fan": int((mism & fan).sum()),
           "mismatch_tie": int((mism & tie & ~fan).sum()), "mismatch_other": int((mism & ~fan & ~tie).sum()),
           "identity_outside_class": float(same[rest].mean()),
           "t_bits_equal_on_same_hits": float((t[h].view(np.uint32) == ot[h].view(np.uint32)).mean()),
           "occlusion_agree_all": float((occ == oocc).mean()),
           "occlusion_disagree": int((occ != oocc).sum()),
           "occlusion_disagree_fan": int(((occ != oocc) & occ_fan).sum()),
           "occlusion_agree_outside_fan": float((occ == oocc)[~occ_fan].mean())}
    _log_parity("c5_first_hits", rec)
    assert h.sum() > 30000
    # §8(c) over every ray, and again outside the documented class; the class itself is bounded (r03
    # measured 0 mismatches of either kind), so a regression on the fan rows cannot hide in it
    assert rec["identity_all"] >= 0.9999, rec
    assert rec["identity_outside_class"] >= 0.9999, rec
    assert rec["mismatch_fan"] + rec["mismatch_tie"] <= 1e-4 * len(rays), rec
    assert rec["t_bits_equal_on_same_hits"] >= 0.9999, rec
    assert rec["occlusion_agree_all"] >= 0.9999, rec
    assert rec["occlusion_agree_outside_fan"] >= 0.9999, rec


def test_c5_render_vs_oracle(renderer, c5_scene):
    """A small C5 render vs the oracle.  Pixels any of whose camera samples first hits the pole fan
    rows or ties (as in test_c5_deep_bvh_first_hits) form the documented exclusion class; §8(c)'s
    99.9 % exact RGB8 pixels and 1e-3 relative L1 hold on the rest (fractions logged)."""
    flat, P = c5_scene
    W, H, S = 128, 72, 2
    cam = sptr.camera_lookat(aspect=W / H)
    st = renderer.render(cam, W, H, spp=S)
    rgb, acc = renderer.read_rgb8(), renderer.read_accum()
    oacc, orgb, ocnt = P.render(cam.as_array(), W, H, oracle.preset_materials(False), oracle.default_lights(),
                                frames=S, threads=THREADS)
    assert st.samples == W * H * S
    cls = np.zeros(W * H, bool)
    for a in range(1, S + 1):
        rays = _camera_rays(cam, W, H, a)
        g, pr, t, _ = renderer.intersect(rays)
        og, opr, ot, _ = P.intersect(rays)
        tie = (g != 0xFFFFFFFF) & (og != 0xFFFFFFFF) & (t.view(np.uint32) == ot.view(np.uint32)) & (pr != opr)
        cls |= _c5_fan_rows(flat, g, pr) | _c5_fan_rows(flat, og, opr) | tie
    cls = cls.reshape(H, W)
    exact = (rgb == orgb).all(axis=2)
    fin = np.isfinite(acc).all(axis=2) & np.isfinite(oacc).all(axis=2)
    m = fin & ~cls
    rel_rest = float(np.abs(acc[m] - oacc[m]).sum() / max(1e-12, np.abs(oacc[m]).sum()))
    rel_all = float(np.abs(acc[fin] - oacc[fin]).sum() / max(1e-12, np.abs(oacc[fin]).sum()))
    rec = {"pixels": W * H, "class_pixels": int(cls.sum()), "exact_all": float(exact.mean()),
           "exact_outside_class": float(exact[~cls].mean()), "rel_l1_all": rel_all, "rel_l1_outside_class": rel_rest,
           "differing_pixels_in_class": int((~exact & cls).sum()), "differing_pixels_outside": int((~exact & ~cls).sum())}
    _log_parity("c5_render", rec)
    assert rec["exact_all"] >= 0.999 and rel_all <= 1e-3, rec
    assert rec["exact_outside_class"] >= 0.999, rec
    assert rel_rest <= 1e-3, rec
    assert rec["differing_pixels_in_class"] <= 1e-3 * W * H, rec


# ------------------------------------------------------------------- full-size timed configurations
def _render_as_bench(renderer, cam, W, H, S):
    """The timed call shape of bench.py (in-step cull, SPTR_FRAME_RECULL) three times: direct launches,
    then the captured graph (second call of the shape, launch mode 3), then its replay.  All three must be identical;
    the replay's image is returned."""
    runs = []
    try:
        renderer.set_launch_mode(3)  # (mode 0 launches a large call with side-stream launches directly)
        for _ in range(3):
            st = renderer.render(cam, W, H, spp=S, flags=sptr.SPTR_FRAME_RECULL)
            runs.append((st, renderer.read_rgb8().copy(), renderer.read_accum().copy()))
        g = renderer.graph_info()
    finally:
        renderer.set_launch_mode(0)
    for st, rgb, acc in runs[1:]:
        assert np.array_equal(rgb, runs[0][1])
        assert np.array_equal(acc.view(np.uint32), runs[0][2].view(np.uint32))
        assert (st.rays_closest, st.rays_shadow) == (runs[0][0].rays_closest, runs[0][0].rays_shadow)
    assert g["valid"] == 1, g
    return runs[-1]


def _full_size_parity(name, renderer, P, cam, W, H, S, rgb, acc, orgb, oacc, flat=None, fan_aware=False,
                      env_faces=None):
    """residue.full_size_parity with, for the 10M-triangle mesh (fan_aware), its BVH tie class: a camera
    sample's first hit on a pole fan row or a t tie between primitives, on either side."""
    def tie_fn(ys, xs):
        tie = np.zeros(len(ys), bool)
        for a in range(1, S + 1):
            d, _ = oracle.primary(cam.as_array(), W, H, a)
            rays = np.zeros((len(ys), 8), np.float32)
            rays[:, 0:3] = cam.as_array()[:3]
            rays[:, 3:6] = d[ys, xs]
            rays[:, 7] = np.inf
            g, pr, t, _ = renderer.intersect(rays)
            og, opr, ot, _ = P.intersect(rays)
            tt = (g != 0xFFFFFFFF) & (og != 0xFFFFFFFF) & (t.view(np.uint32) == ot.view(np.uint32)) & (pr != opr)
            tie |= _c5_fan_rows(flat, g, pr) | _c5_fan_rows(flat, og, opr) | tt
        return tie

    return residue.full_size_parity(name, renderer, P, cam, W, H, S, rgb, acc, orgb, oacc,
                                    tie_fn=tie_fn if fan_aware else None, env_faces=env_faces, log=_log_parity)


def test_c5_full_size_vs_oracle(renderer, c5_scene):
    """C5 at the size bench.py times it: 1920x1080 x 64 spp on the full 10M-triangle mesh, one 2^27-path
    batch (BVH4 from HBM, treelets over the whole tree, k_shadow_dyn beside the bounce traces, k_sky beside
    bounce 0, the k_tail refill from bounce 3, per-XCD shadow queues over the resident grid), captured and
    replayed as a launch graph, against the oracle (its own SAH BVH) rendering the same frame."""
    flat, P = c5_scene
    wl = workloads.WORKLOADS["c5"]
    if renderer.scene_layout()["num_tris"] != 10_000_000:  # another test replaced the scene
        workloads.setup(renderer, wl)
    W, H, S = wl.width, wl.height, wl.spp
    cam = workloads.camera(wl)
    st, rgb, acc = _render_as_bench(renderer, cam, W, H, S)
    assert st.samples == W * H * S and st.waves == 1
    oacc, orgb, ocnt = P.render(cam.as_array(), W, H, oracle.preset_materials(False), oracle.default_lights(),
                                frames=S, threads=THREADS)
    assert st.samples == ocnt["samples"]
    _full_size_parity("c5_full_size", renderer, P, cam, W, H, S, rgb, acc, orgb, oacc, flat, fan_aware=True)
    assert abs(int(st.rays_closest) - ocnt["rays_closest"]) <= 1e-3 * ocnt["rays_closest"], (st.rays_closest, ocnt)
    assert abs(int(st.rays_shadow) - ocnt["rays_shadow"]) <= 1e-3 * ocnt["rays_shadow"], (st.rays_shadow, ocnt)


def test_c3_full_size_vs_oracle(renderer):
    """C3 at the size bench.py times it: the rattan chair + HDR cubemap, 1920x1080 x 256 spp in one 2^29-path
    batch (L2-resident BVH4, k_sky folding the culled pixels beside bounce 0, k_tail from bounce 2),
    captured and replayed, against the oracle rendering all 256 samples."""
    wl = workloads.WORKLOADS["c3"]
    faces = workloads.hdr_env_faces()
    flat = workloads.setup(renderer, wl)
    W, H, S = wl.width, wl.height, wl.spp
    cam = workloads.camera(wl)
    st, rgb, acc = _render_as_bench(renderer, cam, W, H, S)
    assert st.samples == W * H * S
    P = oracle.Prepared(_flat_dict(flat), bvh=True)
    oacc, orgb, ocnt = P.render(cam.as_array(), W, H, oracle.preset_materials(False), oracle.default_lights(),
                                frames=S, env_faces=faces, threads=THREADS)
    _full_size_parity("c3_full_size", renderer, P, cam, W, H, S, rgb, acc, orgb, oacc, env_faces=faces)
    assert abs(int(st.rays_closest) - ocnt["rays_closest"]) <= 1e-3 * ocnt["rays_closest"]
    assert abs(int(st.rays_shadow) - ocnt["rays_shadow"]) <= 1e-3 * ocnt["rays_shadow"]
    renderer.set_environment(None)


def test_c4_multibatch_vs_oracle(renderer):
    """C4's 4K frame at 16 spp in four 4-sample batches (set_wave_paths 2^25): the pixel-major bounce 0,
    the batch-to-batch accumulation and the resolve of the last batch at the C4 size, captured and
    replayed, against the oracle."""
    W, H, S = 3840, 2160, 16
    sptr.setup_default(renderer, "default")
    cam = sptr.camera_lookat(aspect=W / H)
    try:
        renderer.set_wave_paths(1 << 25)
        st, rgb, acc = _render_as_bench(renderer, cam, W, H, S)
    finally:
        renderer.set_wave_paths(0)
    assert st.waves == 4 and st.samples == W * H * S
    P = oracle.Prepared(oracle.builtin_scene("default"), bvh=True)
    oacc, orgb, ocnt = P.render(cam.as_array(), W, H, oracle.preset_materials(False), oracle.default_lights(),
                                frames=S, threads=THREADS)
    _full_size_parity("c4_multibatch", renderer, P, cam, W, H, S, rgb, acc, orgb, oacc)
    assert abs(int(st.rays_closest) - ocnt["rays_closest"]) <= 1e-4 * ocnt["rays_closest"]
