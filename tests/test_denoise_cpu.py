"""The denoiser's filter (sptr_set_denoise) on the CPU alone: tests/denoise_ref.py, the numpy float32
restatement the GPU kernels are compared with bit for bit (tests/test_gpu_denoise.py), applied to oracle
renders of the default scene with first-hit features from the oracle's own closest-hit queries.

Quality is the RMSE of the resolved RGB8 image against a 512-frame oracle render, over all pixels of the
320x240 default view.  Measured here with the defaults at 3 iterations (noisy -> denoised): n = 1:
9.07 -> 4.95, n = 4: 3.97 -> 2.95, n = 16: 2.25 -> 2.02 (DESIGN.md "Denoiser").  The test asserts the
order only, not a ratio."""
import os

import numpy as np
import pytest

import denoise_ref as D
import oracle

W, H = 320, 240
THREADS = min(16, os.cpu_count() or 1)
COUNTS = (1, 4, 16)


@pytest.fixture(scope="module")
def data():
    scene = oracle.builtin_scene("default")
    P = oracle.Prepared(scene, bvh=True)
    cam = oracle.camera()
    mats = oracle.preset_materials(False)
    acc, done, snaps = None, 0, {}
    for n in COUNTS + (512,):
        acc, _, _ = P.render(cam, W, H, mats, oracle.default_lights(), frames=n - done, frame_begin=done + 1,
                             threads=THREADS, accum=acc)
        done = n
        snaps[n] = acc.copy()
    dirs = D.pixel_centre_dirs(cam, W, H)
    g, p, t, ng = P.intersect(D.pixel_centre_rays(cam, W, H, dirs))
    nz, albedo, _ = D.aov_from_hits(g, p, t, ng, dirs, mats, scene["geom_material"])
    for a in list(snaps.values()) + [nz, albedo]:
        a.setflags(write=False)
    return {"snaps": snaps, "nz": nz, "albedo": albedo, "truth": oracle.resolve(snaps[512], 512)}


def _rmse(rgb, truth):
    return float(np.sqrt(((rgb.astype(np.float64) - truth.astype(np.float64)) ** 2).mean()))


def test_features_cover_hits_and_sky(data):
    hit = data["nz"][..., 3] >= 0
    assert 0.05 < hit.mean() < 0.95  # the view holds both surfaces and sky
    n = data["nz"][hit, 0:3]
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert (data["nz"][~hit] == np.array([0, 0, 0, -1], np.float32)).all() and (data["albedo"][~hit] == 0).all()


@pytest.mark.parametrize("n", COUNTS)
def test_denoised_is_closer_to_the_converged_image(data, n):
    noisy = _rmse(oracle.resolve(data["snaps"][n], n), data["truth"])
    c = D.denoise(data["snaps"][n], n, data["nz"], data["albedo"], 3)
    den = _rmse(oracle.resolve(c, 1), data["truth"])
    print(f"n={n}: RMSE noisy {noisy:.2f} denoised {den:.2f}")
    assert den < noisy


def test_miss_pixels_pass_through_bit_unchanged(data):
    c0 = D.mean(data["snaps"][1], 1)
    c = D.denoise(data["snaps"][1], 1, data["nz"], data["albedo"], 5)
    miss = data["nz"][..., 3] < 0
    assert miss.any() and np.array_equal(c[miss].view(np.uint32), c0[miss].view(np.uint32))
    assert not np.array_equal(c[~miss], c0[~miss])  # (the filter did something elsewhere)


def test_injected_inf_pixel_passes_through_and_contaminates_nothing(data):
    hit = data["nz"][..., 3] >= 0
    # a hit pixel whose 5x5 neighbours are hits too: inside a surface, so that neighbours do read it
    y, x = next((int(y), int(x)) for y, x in zip(*np.nonzero(hit))
                if 2 <= y < H - 2 and 2 <= x < W - 2 and hit[y - 2:y + 3, x - 2:x + 3].all())
    acc = data["snaps"][4].copy()
    acc[y, x] = (np.inf, 1.0, np.nan)
    c = D.denoise(acc, 4, data["nz"], data["albedo"], 5)
    ref = D.denoise(data["snaps"][4], 4, data["nz"], data["albedo"], 5)
    assert np.isinf(c[y, x, 0]) and c[y, x, 1] == np.float32(0.25) and np.isnan(c[y, x, 2])
    other = np.ones((H, W), bool)
    other[y, x] = False
    assert np.isfinite(c[other]).all()
    # the pixel weighs 0 in its neighbours' sums, so they merely lack one tap, and beyond the filter's
    # reach (5 iterations: 2 * (1 + 2 + 4 + 8 + 16) = 62 pixels) nothing changes at all
    far = np.ones((H, W), bool)
    far[max(0, y - 62):y + 63, max(0, x - 62):x + 63] = False
    assert np.array_equal(c[far], ref[far])
    assert not np.array_equal(c[y, x + 1], ref[y, x + 1])


@pytest.mark.parametrize("name,p0,p1", [("default", 0, 0), ("default_emitter", 0, 0), ("sphere_mesh", 30, 70)])
def test_one_ulp_direction_nudge_moves_few_ids(name, p0, p1):
    """The cap of tests/test_gpu_denoise.py's id comparison (99.9 % equal) against what a 1-ulp difference
    of the ray directions can do at silhouettes: oracle to oracle, every component nudged up, then down, at
    that test's 150x82 view.  Measured: 0 of 12300 pixels in every case."""
    Wg, Hg = 150, 82
    P = oracle.Prepared(oracle.builtin_scene(name, p0, p1), bvh=True)
    cam = oracle.camera(aspect=Wg / Hg)
    d = D.pixel_centre_dirs(cam, Wg, Hg)
    g0, q0, _, _ = P.intersect(D.pixel_centre_rays(cam, Wg, Hg, d))
    for toward in (np.inf, -np.inf):
        g1, q1, _, _ = P.intersect(D.pixel_centre_rays(cam, Wg, Hg, np.nextafter(d, np.float32(toward))))
        assert ((g0 != g1) | (q0 != q1)).mean() < 1e-3


def test_zero_iterations_is_the_identity(data):
    c0 = D.mean(data["snaps"][4], 4)
    c = D.denoise(data["snaps"][4], 4, data["nz"], data["albedo"], 0)
    assert np.array_equal(c.view(np.uint32), c0.view(np.uint32))
