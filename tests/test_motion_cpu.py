"""Motion vectors (sptr_set_history_motion) on the CPU alone: tests/motion_ref.py, the numpy float32 restatement
the GPU kernel is compared with bit for bit (tests/test_gpu_motion.py), applied to oracle renders of scenes whose
geometry moves under a standing camera.

Geometry k of a sequence is refit_common.deform(positions, spheres, a k); frame k is one oracle frame of it,
seeded as accumulation index k + 1.  First-hit features come from the oracle's closest-hit queries on the
pixel-centre rays, the barycentrics from query_common.emulated_uv (the kernel's expressions in float32).  Every
pass is the next one's carry, read through the geometry it saw.

Run as a script (with oracle/ on PYTHONPATH) this file prints the table of DESIGN.md §6h.  Measured here
(default, 320 x 240, a = 0.3, 8 frames, M = 4, 3 iterations, last-frame RGB8 RMSE against 128 oracle frames):
no history 4.79, history kept without motion vectors (clipped) 4.42, motion vectors (clipped) 4.38; the script's
table takes 256 frames as the truth (4.77, 4.40, 4.36)."""
import os

import numpy as np
import pytest

import denoise_ref as D
import motion_ref as M
import oracle
import query_common as Q
import refit_common as R
import temporal_ref as T

THREADS = min(16, os.cpu_count() or 1)
ITER = 3
MAX_HISTORY = 4
SMALL = (150, 82)
STEP = 0.3
# what the GPU tests' inputs must show on their last step (tests/test_gpu_motion.py asserts the first on the device)
FLOOR_TAKEN, FLOOR_MOVING = 0.9, 0.6
GPU_POSITIONS = [(0.0, 3.0, 8.0), (0.41869, 3.0, 7.98904)]  # the default camera and one 3 degrees on (test_gpu_temporal.py)


def features(P, scene, mats, cam, W, H):
    """(nz, albedo, ids, uv) of the scene's first hits along the pixel-centre rays."""
    dirs = D.pixel_centre_dirs(cam, W, H)
    rays = D.pixel_centre_rays(cam, W, H, dirs)
    g, p, t, ng = P.intersect(rays)
    nz, albedo, ids = D.aov_from_hits(g, p, t, ng, dirs, mats, scene["geom_material"])
    uv = np.zeros((H * W, 2), np.float32)
    mask, tri = Q.triangle_hits(scene["tri_geom_first"], g, p)
    if mask.any():
        u, v = Q.emulated_uv(scene["positions"], scene["indices"], rays[mask], tri)
        uv[mask, 0], uv[mask, 1] = u, v
    return nz, albedo, ids, uv.reshape(H, W, 2)


def build_sequence(name, p0, p1, W, H, a, frames, truth_frames=0, geometry=None, positions=None):
    """Frames 0..frames-1 of one scene under a standing camera (or, with positions, frame k seen from
    positions[k]): per frame the geometry, the camera, the features and one oracle frame; with truth_frames, the
    resolved truth_frames-frame render of the last geometry."""
    base = oracle.builtin_scene(name, p0, p1)
    mats, lights = oracle.preset_materials(name == "default_emitter"), oracle.default_lights()
    cam = oracle.camera(aspect=W / H)
    geometry = geometry or (lambda k: R.deform(base["positions"], base["spheres"], a * k))
    steps = []
    for k in range(frames):
        if positions:
            cam = oracle.camera(pos=positions[k], aspect=W / H)
        pos, sph = geometry(k)
        scene = dict(base, positions=pos, spheres=sph)
        P = oracle.Prepared(scene, bvh=True)
        acc = P.render(cam, W, H, mats, lights, frames=1, frame_begin=k + 1, threads=THREADS)[0]
        steps.append({"geo": (pos, sph), "cam": cam, "feat": features(P, scene, mats, cam, W, H), "acc": acc})
    seq = {"cam": cam, "steps": steps, "topo": (base["indices"], base["tri_geom_first"]), "W": W, "H": H}
    if truth_frames:
        seq["truth"] = oracle.resolve(P.render(cam, W, H, mats, lights, frames=truth_frames, threads=THREADS)[0], truth_frames)
    return seq


def run(seq, mode):
    """The sequence's passes, each the next one's carry.  mode "motion": through the geometry the carry saw;
    "static": the history kept as if nothing had moved (the same pass with the current geometry as previous:
    clipped, no motion vectors).  The last pass's (filtered, hist, reprojected, motion, carry)."""
    topo = seq["topo"]
    carry, out, prev = None, None, None
    for st in seq["steps"]:
        nz, albedo, ids, uv = st["feat"]
        cam = st["cam"]
        if carry is None:
            den, hist, cnt = T.denoise(st["acc"], 1, nz, albedo, ids, cam, None, MAX_HISTORY, ITER)
            out = (den, hist, cnt, None, None)
        else:
            seen = prev if mode == "motion" else st["geo"]
            out = M.denoise(st["acc"], 1, nz, albedo, ids, uv, cam, carry, MAX_HISTORY, ITER, topo, seen, st["geo"]) + (carry,)
        carry = {"hist": out[1], "nz": nz, "ids": ids, "cam": cam}
        prev = st["geo"]
    return out


def _rmse(rgb, truth):
    return float(np.sqrt(((rgb.astype(np.float64) - truth.astype(np.float64)) ** 2).mean()))


def _speed(motion):
    return np.sqrt((motion.astype(np.float64) ** 2).sum(axis=-1))


def fractions(seq):
    """Of the last step's hit pixels: the part that takes history on the motion path, the part that moved more
    than half a pixel, and the part that takes history when the same carry is reprojected without motion vectors."""
    _, hist, cnt, motion, carry = run(seq, "motion")
    last = seq["steps"][-1]
    nz, _, ids, _ = last["feat"]
    hits = int((nz[..., 3] >= 0).sum())
    with np.errstate(invalid="ignore"):
        moving = int((_speed(motion) > 0.5).sum())
    _, plain = T.reproject(D.mean(last["acc"], 1), 1, nz, ids, last["cam"], carry, MAX_HISTORY)
    return cnt / hits, moving / hits, plain / hits


@pytest.fixture(scope="module", params=R.SCENES, ids=R.SCENE_IDS)
def small(request):
    name, p0, p1, _ = request.param
    return name, build_sequence(name, p0, p1, *SMALL, STEP, 4)


# ---------------------------------------------------------------------------------------- 1. the GPU tests' inputs
def test_gpu_inputs_are_not_vacuous(small):
    name, seq = small
    taken, moving, plain = fractions(seq)
    print(f"{name}: {taken:.3f} of the hit pixels take history, {moving:.3f} move more than 0.5 px, "
          f"{plain:.3f} take history without motion vectors")
    assert taken >= FLOOR_TAKEN
    assert moving >= FLOOR_MOVING
    assert plain < taken


def test_gpu_inputs_with_the_last_step_seen_from_elsewhere(small):
    """tests/test_gpu_motion.py takes its last step from a camera 3 degrees on: the floor it asserts there."""
    name, _ = small
    _, p0, p1, _ = next(c for c in R.SCENES if c[0] == name)
    seq = build_sequence(name, p0, p1, *SMALL, STEP, 4, positions=[GPU_POSITIONS[0]] * 3 + [GPU_POSITIONS[1]])
    taken, moving, plain = fractions(seq)
    print(f"{name}, camera moved: {taken:.3f} of the hit pixels take history, {moving:.3f} move more than 0.5 px, "
          f"{plain:.3f} take history without motion vectors")
    assert taken >= FLOOR_TAKEN and plain < taken


# ---------------------------------------------------------------------------------------- 2. rigid translation
@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_rigid_translation_against_a_float64_projection(cfg):
    """Independent of the restatement's algebra: the float64 projection of P - delta, P the float64 hit point."""
    name, p0, p1, _ = cfg
    W, H = SMALL
    delta = np.array([0.2, 0.0, 0.1])
    base = oracle.builtin_scene(name, p0, p1)

    def geometry(k):
        pos = (base["positions"].astype(np.float64) + k * delta).astype(np.float32)
        sph = base["spheres"].astype(np.float64)
        sph[:, 0:3] += k * delta
        return pos, sph.astype(np.float32)

    seq = build_sequence(name, p0, p1, W, H, 0.0, 2, geometry=geometry)
    _, _, cnt, motion, _ = run(seq, "motion")
    cam = seq["cam"].astype(np.float64)
    nz = seq["steps"][-1]["feat"][0]
    hit = nz[..., 3] >= 0
    d = D.pixel_centre_dirs(seq["cam"], W, H).astype(np.float64)
    v = nz[..., 3:4].astype(np.float64) * d - delta  # P - delta - pos
    zf = v @ cam[3:6]
    fx = ((v @ cam[6:9]) / (zf * cam[12]) * 0.5 + 0.5) * W - 0.5
    fy = (0.5 - (v @ cam[9:12]) / (zf * cam[13]) * 0.5) * H - 0.5
    ex = np.abs(np.arange(W)[None, :] + motion[..., 0].astype(np.float64) - fx)[hit]
    ey = np.abs(np.arange(H)[:, None] + motion[..., 1].astype(np.float64) - fy)[hit]
    print(f"{name}: {int(hit.sum())} hit pixels, worst distance to the float64 projection {max(ex.max(), ey.max()):.2e} px; "
          f"mean motion {_speed(motion)[hit].mean():.2f} px; {cnt} took history")
    assert hit.sum() > 1000 and np.isfinite(motion[hit]).all() and np.isnan(motion[~hit]).all()
    assert ex.max() <= 1e-3 and ey.max() <= 1e-3
    assert _speed(motion)[hit].mean() > 1.0  # (the translation did move the image)


# ---------------------------------------------------------------------------------------- 3. quality
@pytest.fixture(scope="module")
def big():
    return build_sequence("default", 0, 0, 320, 240, STEP, 8, truth_frames=128)


def quality(seq):
    """Last-frame RGB8 RMSE against the truth: no history, history kept without motion vectors, motion vectors."""
    last = seq["steps"][-1]
    nz, albedo, _, _ = last["feat"]
    plain = _rmse(oracle.resolve(D.denoise(last["acc"], 1, nz, albedo, ITER), 1), seq["truth"])
    static = _rmse(oracle.resolve(run(seq, "static")[0], 1), seq["truth"])
    motion = _rmse(oracle.resolve(run(seq, "motion")[0], 1), seq["truth"])
    return plain, static, motion


def test_motion_vectors_are_closer_to_the_converged_image(big):
    plain, static, motion = quality(big)
    print(f"last frame RMSE: no history {plain:.2f}, history kept without motion vectors (clipped) {static:.2f}, "
          f"motion vectors (clipped) {motion:.2f}")
    assert motion < plain


# ---------------------------------------------------------------------------------------- 4. zero motion
def test_zero_motion(small):
    """The geometry the carry saw is the current one: every pixel that takes history has not moved."""
    name, seq = small
    st = seq["steps"][1]
    nz, albedo, ids, uv = st["feat"]
    cam = seq["cam"]
    first = T.reproject(D.mean(st["acc"], 1), 1, nz, ids, cam, None, MAX_HISTORY)[0]
    carry = {"hist": first, "nz": nz, "ids": ids, "cam": cam}
    hist, cnt, motion = M.reproject(D.mean(st["acc"], 1), 1, nz, ids, uv, cam, carry, MAX_HISTORY, seq["topo"], st["geo"], st["geo"])
    took = hist[..., 3] > 1
    hits = int((nz[..., 3] >= 0).sum())
    print(f"{name}: {cnt} of {hits} hit pixels take history, worst |motion| {_speed(motion)[took].max():.2e} px")
    assert cnt == took.sum() and cnt > 0.9 * hits
    assert _speed(motion)[took].max() < 1e-3


if __name__ == "__main__":
    print("| scene, size, step a | no history | history kept, no motion vectors, clipped | motion vectors, clipped | "
          "hit pixels taking history (static / motion) | mean motion px |")
    for name, p0, p1, W, H, a in (("default", 0, 0, 320, 240, 0.3), ("default", 0, 0, 320, 240, 0.6),
                                  ("default_emitter", 0, 0, 150, 82, 0.3), ("sphere_mesh", 30, 70, 150, 82, 0.3)):
        s = build_sequence(name, p0, p1, W, H, a, 8, truth_frames=256)
        q = quality(s)
        taken, moving, plain_taken = fractions(s)
        mv = run(s, "motion")[3]
        print(f"| {name}, {W}x{H}, {a} | {q[0]:.2f} | {q[1]:.2f} | {q[2]:.2f} | {plain_taken:.3f} / {taken:.3f} | "
              f"{np.nanmean(_speed(mv)):.1f} |")
