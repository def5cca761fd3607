"""Temporal reprojection (sptr_set_denoise_history) on the CPU alone: tests/temporal_ref.py, the numpy float32
restatement the GPU kernels are compared with bit for bit (tests/test_gpu_temporal.py), applied to oracle
renders of the default scene with first-hit features from the oracle's own closest-hit queries, at 320x240
as tests/test_denoise_cpu.py.

The camera path: 8 cameras orbiting the default target about the vertical axis by ORBIT_DEG per frame, one
oracle frame each in an accumulation of its own; frame k is seeded as accumulation index k + 1 (what
sptr_set_seed_offset(k) gives a restarted accumulation).  Quality is the RMSE of the resolved RGB8 image at
the last camera against a 512-frame oracle render there.  Run as a script (with oracle/ on PYTHONPATH), this
file prints the table of DESIGN.md §6f (the cap M in {4, 8, 16, 32}, with and without seed offsets).

Measured here (M = 4): 3 iterations without history 4.44, with history 3.89, with history and every frame
seeded as frame 1 4.00.  Without the variance clip of the history (temporal_ref.CLIP) the same path gave
5.71: the default scene's spheres are glass and polished metal, whose colour belongs to the view."""
import math
import os

import numpy as np
import pytest

import denoise_ref as D
import oracle
import temporal_ref as T

W, H = 320, 240
THREADS = min(16, os.cpu_count() or 1)
FRAMES = 8
ORBIT_DEG = 3.0
ITER = 3
M_DEFAULT = 4  # the default of HipBackend and sptr_cli (lowest last-frame RMSE of the table)
POS, TARGET = (0.0, 3.0, 8.0), (0.0, 1.0, 0.0)


def orbit_camera(k: int) -> np.ndarray:
    a = math.radians(ORBIT_DEG * k)
    dx, dz = POS[0] - TARGET[0], POS[2] - TARGET[2]
    pos = (TARGET[0] + dx * math.cos(a) + dz * math.sin(a), POS[1], TARGET[2] - dx * math.sin(a) + dz * math.cos(a))
    return oracle.camera(pos=pos, target=TARGET, aspect=W / H)


def _features(P, scene, mats, cam):
    dirs = D.pixel_centre_dirs(cam, W, H)
    g, p, t, ng = P.intersect(D.pixel_centre_rays(cam, W, H, dirs))
    return D.aov_from_hits(g, p, t, ng, dirs, mats, scene["geom_material"])


def build_data():
    scene = oracle.builtin_scene("default")
    P = oracle.Prepared(scene, bvh=True)
    mats, lights = oracle.preset_materials(False), oracle.default_lights()
    cams = [orbit_camera(k) for k in range(FRAMES)]
    feats = [_features(P, scene, mats, c) for c in cams]
    offset = [P.render(c, W, H, mats, lights, frames=1, frame_begin=k + 1, threads=THREADS)[0] for k, c in enumerate(cams)]
    same = [offset[0]] + [P.render(c, W, H, mats, lights, frames=1, frame_begin=1, threads=THREADS)[0] for c in cams[1:]]
    truth, _, _ = P.render(cams[-1], W, H, mats, lights, frames=512, threads=THREADS)
    # the standing camera: frames 1..4 at camera 0, each alone, and their accumulation
    stand = [offset[0]] + [P.render(cams[0], W, H, mats, lights, frames=1, frame_begin=k + 1, threads=THREADS)[0]
                           for k in range(1, 4)]
    acc4, _, _ = P.render(cams[0], W, H, mats, lights, frames=4, threads=THREADS)
    for a in offset + same + stand + [acc4] + [x for f in feats for x in f]:
        a.setflags(write=False)
    return {"cams": cams, "feats": feats, "offset": offset, "same": same, "stand": stand, "acc4": acc4,
            "truth": oracle.resolve(truth, 512)}


@pytest.fixture(scope="module")
def data():
    return build_data()


def _rmse(rgb, truth):
    return float(np.sqrt(((rgb.astype(np.float64) - truth.astype(np.float64)) ** 2).mean()))


def run_path(frames, cams, feats, max_history):
    """Every frame an accumulation of its own (n = 1), each pass the next one's carry: the last pass's
    (filtered, hist, reprojected)."""
    carry, out = None, None
    for acc, cam, (nz, albedo, ids) in zip(frames, cams, feats):
        out = T.denoise(acc, 1, nz, albedo, ids, cam, carry, max_history, ITER)
        carry = {"hist": out[1], "nz": nz, "ids": ids, "cam": cam}
    return out


def test_the_path_moves_the_image_a_few_pixels_per_frame(data):
    nz, _, _ = data["feats"][1]
    cam0, cam1 = data["cams"][0], data["cams"][1]
    d = D.pixel_centre_dirs(cam1, W, H)
    hit = nz[..., 3] >= 0
    v = (cam1[0:3] + nz[..., 3:4] * d - cam0[0:3]).astype(np.float64)
    nx = (v @ cam0[6:9].astype(np.float64)) / ((v @ cam0[3:6].astype(np.float64)) * cam0[12])
    fx = (nx * 0.5 + 0.5) * W - 0.5
    move = np.abs(fx - np.arange(W)[None, :])[hit]
    print(f"orbit {ORBIT_DEG} deg: the hits move {move.mean():.2f} px on average, {move.max():.2f} at most")
    assert 1.0 <= move.mean() <= 8.0


def test_history_is_closer_to_the_converged_image(data):
    nz, albedo, _ = data["feats"][-1]
    plain = _rmse(oracle.resolve(D.denoise(data["offset"][-1], 1, nz, albedo, ITER), 1), data["truth"])
    den, hist, cnt = run_path(data["offset"], data["cams"], data["feats"], M_DEFAULT)
    with_history = _rmse(oracle.resolve(den, 1), data["truth"])
    same, _, _ = run_path(data["same"], data["cams"], data["feats"], M_DEFAULT)
    print(f"last frame RMSE: {ITER} iterations {plain:.2f}, with history (M = {M_DEFAULT}) {with_history:.2f}; "
          f"without seed offsets {_rmse(oracle.resolve(same, 1), data['truth']):.2f}; "
          f"{cnt} of {int((nz[..., 3] >= 0).sum())} hit pixels took history, mean m' {hist[..., 3][nz[..., 3] >= 0].mean():.2f}")
    assert with_history < plain


def test_standing_camera_converges_to_the_accumulation(data):
    cams, feats = [data["cams"][0]] * 4, [data["feats"][0]] * 4
    _, hist, _ = run_path(data["stand"], cams, feats, M_DEFAULT)
    nz = feats[0][0]
    mean4 = D.mean(data["acc4"], 4)
    ok = (nz[..., 3] >= 0) & np.isfinite(mean4).all(axis=-1)
    assert ok.any()
    print(f"m' in [{hist[ok, 3].min():.6f}, {hist[ok, 3].max():.6f}]")
    assert np.abs(hist[ok, 3] - 4.0).max() <= 1e-3
    rel = float(np.abs(hist[ok, 0:3].astype(np.float64) - mean4[ok]).sum() / np.abs(mean4[ok].astype(np.float64)).sum())
    print(f"t_0 against the 4-frame mean: relative L1 {rel:.2e}")
    assert rel <= 1e-3


def test_no_carry_is_the_identity(data):
    nz, albedo, ids = data["feats"][0]
    for n, acc in ((1, data["offset"][0]), (4, data["acc4"])):
        den, hist, cnt = T.denoise(acc, n, nz, albedo, ids, data["cams"][0], None, M_DEFAULT, ITER)
        ref = D.denoise(acc, n, nz, albedo, ITER)
        assert cnt == 0 and np.array_equal(den.view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(hist[..., 0:3].view(np.uint32), D.mean(acc, n).view(np.uint32))
        assert (hist[..., 3] == np.where(nz[..., 3] >= 0, np.float32(n), np.float32(0))).all()


@pytest.mark.parametrize("carry_cam", ["behind", "away"])
def test_a_carry_camera_that_cannot_see_the_surfaces_gives_no_history(data, carry_cam):
    nz, albedo, ids = data["feats"][0]
    cam = data["cams"][0]
    first = T.reproject(D.mean(data["offset"][0], 1), 1, nz, ids, cam, None, M_DEFAULT)[0]
    # behind: beyond the scene, looking on along the same axis; away: at the camera's place, turned round
    pc = (oracle.camera(pos=(0.0, -3.0, -40.0), target=(0.0, -5.0, -48.0), aspect=W / H) if carry_cam == "behind"
          else oracle.camera(pos=POS, target=(0.0, 5.0, 16.0), aspect=W / H))
    carry = {"hist": first, "nz": nz, "ids": ids, "cam": pc}
    hist, cnt = T.reproject(D.mean(data["offset"][1], 1), 1, nz, ids, cam, carry, M_DEFAULT)
    ref, _ = T.reproject(D.mean(data["offset"][1], 1), 1, nz, ids, cam, None, M_DEFAULT)
    assert cnt == 0 and np.array_equal(hist.view(np.uint32), ref.view(np.uint32))


def test_injected_inf_carried_pixel_weighs_nothing(data):
    nz, albedo, ids = data["feats"][0]
    cam = data["cams"][0]
    hit = nz[..., 3] >= 0
    y, x = next((int(y), int(x)) for y, x in zip(*np.nonzero(hit))
                if 2 <= y < H - 2 and 2 <= x < W - 2 and hit[y - 2:y + 3, x - 2:x + 3].all()
                and (ids[y - 2:y + 3, x - 2:x + 3, 0] == ids[y, x, 0]).all())
    first = T.reproject(D.mean(data["stand"][0], 1), 1, nz, ids, cam, None, M_DEFAULT)[0]
    bad = first.copy()
    bad[y, x, 0:3] = (np.inf, 1.0, np.nan)
    c0 = D.mean(data["stand"][1], 1)
    clean, n_clean = T.reproject(c0, 1, nz, ids, cam, {"hist": first, "nz": nz, "ids": ids, "cam": cam}, M_DEFAULT)
    got, n_got = T.reproject(c0, 1, nz, ids, cam, {"hist": bad, "nz": nz, "ids": ids, "cam": cam}, M_DEFAULT)
    assert np.isfinite(got).all()  # nothing is contaminated
    # at a standing camera a pixel's taps are its own carried pixel and neighbours one pixel away at most
    far = np.ones((H, W), bool)
    far[y - 1:y + 2, x - 1:x + 2] = False
    assert np.array_equal(got[far].view(np.uint32), clean[far].view(np.uint32))
    assert not np.array_equal(got[y, x], clean[y, x])  # (its own carried pixel was its main tap)
    assert n_clean - 1 <= n_got <= n_clean


if __name__ == "__main__":
    dat = build_data()
    nz_l, albedo_l, _ = dat["feats"][-1]
    print(f"noisy 1 spp: {_rmse(oracle.resolve(dat['offset'][-1], 1), dat['truth']):.2f}")
    print(f"{ITER} iterations, no history: "
          f"{_rmse(oracle.resolve(D.denoise(dat['offset'][-1], 1, nz_l, albedo_l, ITER), 1), dat['truth']):.2f}")
    for M in (4, 8, 16, 32):
        a = _rmse(oracle.resolve(run_path(dat["offset"], dat["cams"], dat["feats"], M)[0], 1), dat["truth"])
        b = _rmse(oracle.resolve(run_path(dat["same"], dat["cams"], dat["feats"], M)[0], 1), dat["truth"])
        print(f"M = {M:2d}: with seed offsets {a:.3f}, every frame seeded as frame 1 {b:.3f}")
