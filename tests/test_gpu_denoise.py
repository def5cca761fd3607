"""GPU tests of the first-hit AOVs (sptr_read_aov) and the edge-avoiding denoiser (sptr_set_denoise).

Configurations: 150x82 (ragged: partial 32x32 tiles on both edges, and wider than the 64-pixel reach of
the step-16 iteration) of the scenes default and default_emitter (BVH2 staged in LDS) and of the 30x70
sphere mesh with set_bvh_width(4) (the wide walk from L2).

AOV ids are compared with Renderer.intersect on the numpy pixel-centre rays (tests/denoise_ref.py): the
expected number of differing pixels is 0, and the 99.9 % floor only keeps a 1-ulp direction difference at a
silhouette from failing the test.  The same comparison oracle to oracle on the CPU, with every direction
component nudged by 1 ulp, differs on 0 of 12300 pixels in each of the three configurations
(tests/test_denoise_cpu.py::test_one_ulp_direction_nudge_moves_few_ids asserts it stays under the cap).

The filter is compared bit for bit with the numpy restatement fed the GPU's own accumulation and AOV
planes; only the resolve's powf differs between ocml and glibc, hence the project's image
criterion (>= 99.9 % identical RGB8 pixels) for read_rgb8."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import oracle
import sptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 150, 82
CONFIGS = [("default", 0, 0, 0), ("default_emitter", 0, 0, 0), ("sphere_mesh", 30, 70, 4)]
_PAGE_LOCKED = []  # (the library keeps a lagged-readback destination page-locked until another takes its place)


def _reset(r):
    r.set_denoise(0)
    r.set_pixel_lanes(0)
    r.set_launch_mode(0)
    r.set_bvh_width(0)


@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def cfg(request, renderer):
    """The scene on the shared renderer, with the reference first hits of the pixel-centre rays (computed
    once per configuration, read-only)."""
    name, p0, p1, width = request.param
    _reset(renderer)
    renderer.set_bvh_width(width)
    flat = sptr.setup_default(renderer, name, p0, p1)
    cam = sptr.camera_lookat(aspect=W / H)
    dirs = D.pixel_centre_dirs(cam.as_array(), W, H)
    geom, prim, t, ng = renderer.intersect(D.pixel_centre_rays(cam.as_array(), W, H, dirs))
    mats = sptr.materials_as_array(sptr.preset_materials(with_light=(name == "default_emitter")))
    nz, albedo, ids = D.aov_from_hits(geom, prim, t, ng, dirs, mats, flat.geom_material)
    for a in (nz, albedo, ids):
        a.setflags(write=False)
    lay = renderer.scene_layout()
    assert (lay["lds_bytes"] != 0) == (width == 0) and lay["bvh_width"] == (4 if width else 2)
    yield {"name": name, "cam": cam, "nz": nz, "albedo": albedo, "ids": ids, "lds": width == 0}
    _reset(renderer)


def _read_aovs(r):
    nz = np.concatenate([r.read_aov(sptr.SPTR_AOV_NORMAL), r.read_aov(sptr.SPTR_AOV_DEPTH)[..., None]], axis=-1)
    return nz, r.read_aov(sptr.SPTR_AOV_ALBEDO), r.read_aov(sptr.SPTR_AOV_ID)


def _same_image(rgb, ref):
    return float((rgb == ref).all(axis=2).mean())


def test_aov_planes_match_intersect(cfg, renderer):
    renderer.set_denoise(0)
    renderer.render(cfg["cam"], W, H, spp=1)
    nz, albedo, ids = _read_aovs(renderer)
    agree = (ids == cfg["ids"]).all(axis=-1)
    print(f"{cfg['name']}: ids differ on {int((~agree).sum())} of {agree.size} pixels")
    assert agree.mean() >= 0.999
    hit = cfg["ids"][..., 0] != D.MISS
    assert hit.any() and (~hit).any()
    m = agree & hit
    assert np.array_equal(nz[m, 3].view(np.uint32), cfg["nz"][m, 3].view(np.uint32))  # depth = intersect's t
    assert np.abs(nz[m, 0:3] - cfg["nz"][m, 0:3]).max() <= 1e-6
    assert np.array_equal(albedo[m].view(np.uint32), cfg["albedo"][m].view(np.uint32))
    m = agree & ~hit  # the miss encodings, exactly
    assert (ids[m] == D.MISS).all() and (nz[m] == np.array([0, 0, 0, -1], np.float32)).all() and (albedo[m] == 0).all()


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("iterations", [1, 5])
def test_filter_is_bit_equal_to_the_restatement(cfg, renderer, iterations, n):
    renderer.set_denoise(iterations)
    renderer.render(cfg["cam"], W, H, spp=n)
    den, rgb, acc = renderer.read_denoised(), renderer.read_rgb8(), renderer.read_accum()
    nz, albedo, _ = _read_aovs(renderer)
    ref = D.denoise(acc, n, nz, albedo, iterations)
    fin = np.isfinite(ref).all(axis=-1)
    assert np.array_equal(fin, np.isfinite(den).all(axis=-1))
    nbad = int((den[fin].view(np.uint32) != ref[fin].view(np.uint32)).any(axis=-1).sum())
    print(f"{cfg['name']} it={iterations} n={n}: {nbad} of {int(fin.sum())} finite pixels differ from the restatement")
    assert nbad == 0
    hit = nz[..., 3] >= 0
    assert not np.array_equal(den[hit], D.mean(acc, n)[hit])  # (the filter ran)
    same = _same_image(rgb, oracle.resolve(ref, 1))
    print(f"  RGB8 identical to oracle.resolve of the restatement: {same:.5f}")
    assert same >= 0.999
    assert np.array_equal(renderer.read_accum(), acc)  # the accumulation is only read


def test_four_single_frames_equal_one_call_of_four(cfg, renderer):
    renderer.set_denoise(3)
    cam = sptr.camera_lookat(pos=(0.0, 3.0, 8.25), aspect=W / H)  # (a camera of this test's own: AOVs not cached)
    before = renderer.denoise_info()["aov_passes"]
    for i in range(4):
        renderer.render(cam, W, H, spp=1, frame_begin=1 + i)
    assert renderer.denoise_info()["aov_passes"] == before + 1  # a static camera pays for the AOVs once
    den, rgb = renderer.read_denoised(), renderer.read_rgb8()
    renderer.render(cam, W, H, spp=4)
    assert np.array_equal(renderer.read_denoised().view(np.uint32), den.view(np.uint32))
    assert np.array_equal(renderer.read_rgb8(), rgb)


def test_two_pixel_lanes_equal_one(cfg, renderer):
    """Two lanes split the accumulation over two contexts (LDS-staged scenes; the others keep one chain
    whatever the setting): c_0 is gathered from both."""
    renderer.set_denoise(3)
    out = []
    for lanes in (1, 2):
        renderer.set_pixel_lanes(lanes)
        renderer.render(cfg["cam"], W, H, spp=2)
        assert renderer.pixel_lanes_info()["active"] == (lanes == 2 and cfg["lds"])
        out.append((renderer.read_denoised(), renderer.read_rgb8()))
    renderer.set_pixel_lanes(0)
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1], out[1][1])


def test_launch_modes_agree(cfg, renderer):
    renderer.set_denoise(2)
    out = []
    for mode in (0, 1, 2, 3):
        renderer.set_launch_mode(mode)
        for i in range(3):  # the shape repeats: modes 0 / 3 replay a captured graph where they capture one
            renderer.render(cfg["cam"], W, H, spp=1, frame_begin=1 + i)
        out.append((renderer.read_denoised(), renderer.read_rgb8()))
    renderer.set_launch_mode(0)
    for den, rgb in out[1:]:
        assert np.array_equal(den.view(np.uint32), out[0][0].view(np.uint32))
        assert np.array_equal(rgb, out[0][1])


def test_lagged_readback_returns_the_previous_denoised_image(cfg, renderer):
    renderer.set_denoise(3)
    buf = np.zeros(W * H * 3, np.uint8)
    small = np.zeros(32 * 32 * 3, np.uint8)
    _PAGE_LOCKED.extend([buf, small])
    # (a call of another size first, so that no snapshot of this size is left from an earlier test)
    renderer.render(cfg["cam"], 32, 32, spp=1, flags=sptr.SPTR_FRAME_ASYNC)
    renderer.read_rgb8_lagged(small)
    prev = None
    for i in range(3):
        renderer.render(cfg["cam"], W, H, spp=1, frame_begin=1 + i, flags=sptr.SPTR_FRAME_ASYNC)
        got = renderer.read_rgb8_lagged(buf)
        assert got == (prev is not None)
        if got:
            assert np.array_equal(buf.reshape(H, W, 3), prev)
        prev = renderer.read_rgb8().copy()
        assert _same_image(prev, oracle.resolve(renderer.read_denoised(), 1)) >= 0.999  # (the denoised image)
    renderer.collect_stats()


def test_off_and_errors():
    """On a context of its own, so that "before the denoiser was ever enabled" holds."""
    r = sptr.Renderer(0)
    try:
        sptr.setup_default(r, "default")
        cam = sptr.camera_lookat(aspect=W / H)
        r.render(cam, W, H, spp=2)
        plain = r.read_rgb8()
        with pytest.raises(sptr.SptrError):
            r.read_denoised()
        r.set_denoise(3)
        r.render(cam, W, H, spp=2)
        assert not np.array_equal(r.read_rgb8(), plain)
        assert r.read_denoised().shape == (H, W, 3)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.render(cam, W, H, spp=1, shard_rank=0, shard_count=2)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.render(cam, W, H, spp=1, integrator=sptr.SPTR_INTEGRATOR_PATHTRACER)
        r.render(cam, W, H, spp=1, flags=sptr.SPTR_FRAME_NO_RESOLVE)  # no resolve, no pass
        with pytest.raises(sptr.SptrError):
            r.read_denoised()
        r.set_denoise(0)
        r.render(cam, W, H, spp=2)
        assert np.array_equal(r.read_rgb8(), plain)
        with pytest.raises(sptr.SptrError):
            r.read_denoised()
        r.render(cam, W, H, spp=1, integrator=sptr.SPTR_INTEGRATOR_PATHTRACER)  # (allowed again)
    finally:
        r.close()


def test_cli_denoise_matches_python(tmp_path):
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"
    out = tmp_path / "img.ppm"
    res = subprocess.run([exe, "--scene", "default", "--w", str(W), "--h", str(H), "--spp", "3", "--denoise", "3",
                          "--json", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert '"ms_aov"' in res.stdout and '"ms_filter"' in res.stdout
    with open(out, "rb") as f:
        parts = f.read().split(b"\n", 3)
    rgb = np.frombuffer(parts[3], np.uint8).reshape(H, W, 3)
    r = sptr.Renderer(0)  # (a context of its own: the shared one holds the configuration's scene)
    try:
        sptr.setup_default(r, "default")
        r.set_denoise(3)
        cam = sptr.camera_lookat(aspect=W / H)
        for i in range(3):
            r.render(cam, W, H, spp=1, frame_begin=1 + i)
        assert np.array_equal(r.read_rgb8(), rgb)
    finally:
        r.close()
