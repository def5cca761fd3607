"""CPU: the float64 cubemap model (tests/env_ref.py) and what the GPU environment tests (tests/test_gpu_env.py)
rely on, without a device.

The oracle's float32 env_color, the same operations in the same order as the kernel's, is the check of the
model's derived error bound: on every map, face size, environment state and direction set of env_common it must
stay within the bound with a worst error / bound ratio of at most 0.5.  Six deliberately wrong variants of the
model must each miss the oracle by orders of magnitude on every map.  The mirror room's float64 path model must
drop no ray of its own set.  Worst ratios are printed as `ENV_MEASURE` lines (profiles/env_measurements.txt)."""
import numpy as np
import pytest

import adversarial_common as A
import env_common as E
import env_ref
import oracle

MAPS = [(kind, S) for kind in E.KINDS for S in E.SIZES]
ORACLE_MAX_RATIO = 0.5
MUTANT_MIN_RATIO = 100.0  # "orders of magnitude" beyond the bound


def _oracle_ratio(dirs, faces, state, either, mutant=None):
    got = oracle.env(dirs, faces, intensity=state[0], clamp=state[1])
    return env_ref.ratio(got, dirs, faces, state[0], state[1], either_face=either, mutant=mutant)


# ---- the sets ---------------------------------------------------------------------------------------------------
def test_direction_sets_are_what_they_claim():
    a = E.dirs_uniform()
    assert a.dtype == np.float32 and a.shape == (20000, 3)
    shares = E.face_shares(a)
    print("set A face shares:", shares.round(3))
    assert (shares >= 0.10).all()
    for name, (d, _) in E.direction_sets(16).items():
        n = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
        assert d.dtype == np.float32 and np.abs(n - 1.0).max() < 1e-5, name
    b = E.dirs_ties()
    i, j = E.tied_pair(b)
    rows = np.arange(len(b))
    assert (i != j).all() and (np.abs(b[rows, i]).view(np.uint32) == np.abs(b[rows, j]).view(np.uint32)).all()
    assert (np.abs(b[rows, i]) == np.abs(b).max(axis=1)).all()
    # every tie order occurs: x = y, x = z, y = z, each with the third component smaller, and x = y = z
    pairs = set(zip(i.tolist(), j.tolist()))
    assert pairs == {(0, 1), (0, 2), (1, 2)}
    # all six faces are the rule's answer somewhere in B only if y and z majors won a tie: they never win against x
    assert set(env_ref.lookup(b, E.coordinate_map(2))[2].tolist()) == {0, 1, 2, 3}
    c = E.dirs_axes()
    assert np.signbit(c[:, 1:]).any() and (c == 0).any() and (np.abs(c[c != 0]).min() < 1e-44)
    d = E.dirs_near_seams()
    assert set(env_ref.lookup(d, E.coordinate_map(2))[2].tolist()) == {0, 1, 2, 3, 4, 5}
    for S in (2, 3, 16):
        e, face, gx, gy = E.dirs_texel_grid(S)
        assert len(e) == 6 * (2 * S - 1) ** 2
        assert ((gx == 0) | (gx == S - 1)).any() and (gx % 1 == 0.5).any()


def test_model_returns_the_texel_at_texel_centres():
    """Set E through the model alone: the direction through the centre of texel (face, x, y) returns faces[face, y,
    x] (clamped, scaled) wherever the tie rule leaves the direction on that face; this pins the row / column stride
    and every flip of the (uc, vc) table against the maps' own indexing."""
    for kind in E.KINDS:
        for S in (2, 3, 16):
            faces = E.env_map(kind, S)
            d, face, gx, gy = E.dirs_texel_grid(S)
            val, tol, got_face = env_ref.lookup(d, faces, 2.5, 0.75)
            centre = (gx % 1 == 0) & (gy % 1 == 0) & (got_face == face)
            interior = (gx > 0) & (gx < S - 1) & (gy > 0) & (gy < S - 1)
            assert (got_face[interior] == face[interior]).all()
            assert centre.sum() >= 6 * max(1, (S - 2) ** 2)
            want = np.minimum(faces[face, gy.astype(int) * centre, gx.astype(int) * centre].astype(np.float64), 0.75) * 2.5
            assert (np.abs(val - want)[centre] <= tol[centre]).all(), (kind, S)
            if kind == "coordinate" and S > 2:  # and a lookup of the coordinate map says where it looked
                k = np.flatnonzero(interior & (gx % 1 == 0.5))[0]
                v1, _, _ = env_ref.lookup(d[k:k + 1], faces, 1.0, 1e30)
                f, x, y = E.decode(v1[0], S)
                assert abs(f - face[k]) < 1e-6 and abs(x - gx[k]) < 1e-6 and abs(y - gy[k]) < 1e-6


def test_cubemap_matches_float64_model():
    """Cubemap::directionToUV + bilinearSample + getCubemapColor worked by hand for one direction per face (the
    cubemap counterpart of test_oracle.py::test_sky_matches_float64_model), on the coordinate map of size 3 at the
    default state: texel coordinates (x, y) = (u, v) * 2, colour 0.8 * ((face + 1) / 8, (x + 1) / 4, (y + 1) / 4)."""
    cases = [  # direction, face, (uc / ma, vc / ma) by the face's row of the table
        ((1.0, 0.5, 0.25), 0, (-0.25, -0.5)),    # +X (-z, -y)
        ((-1.0, 0.5, 0.25), 1, (0.25, -0.5)),    # -X ( z, -y)
        ((0.5, 1.0, 0.25), 2, (0.5, 0.25)),      # +Y ( x,  z)
        ((0.5, -1.0, 0.25), 3, (0.5, -0.25)),    # -Y ( x, -z)
        ((0.5, 0.25, 1.0), 4, (0.5, -0.25)),     # +Z ( x, -y)
        ((0.5, 0.25, -1.0), 5, (-0.5, -0.25)),   # -Z (-x, -y)
    ]
    faces = E.coordinate_map(3)
    dirs = np.array([c[0] for c in cases], np.float64)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    out = oracle.env(dirs.astype(np.float32), faces)
    model, _, mface = env_ref.lookup(dirs.astype(np.float32), faces)
    for (_, face, (a, b)), o, m, mf in zip(cases, out, model, mface):
        x, y = (a + 1.0) / 2.0 * 2.0, (b + 1.0) / 2.0 * 2.0
        want = 0.8 * np.array([(face + 1) / 8.0, (x + 1.0) / 4.0, (y + 1.0) / 4.0])
        assert mf == face
        assert np.allclose(m, want, rtol=0, atol=1e-6), (face, m, want)
        assert np.allclose(o, want, rtol=0, atol=1e-6), (face, o, want)
    # the clamp comes before the intensity: a texel of 4 under (2.5, 0.75) is 0.75 * 2.5, not min(10, 0.75)
    four = np.full((6, 2, 2, 3), 4.0, np.float32)
    assert np.allclose(oracle.env(dirs.astype(np.float32), four, 2.5, 0.75), 1.875, rtol=0, atol=1e-6)
    assert np.allclose(env_ref.lookup(dirs, four, 2.5, 0.75)[0], 1.875, rtol=0, atol=1e-12)


# ---- the bound --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,S", MAPS)
def test_oracle_within_the_bound(kind, S):
    faces = E.env_map(kind, S)
    worst = 0.0
    for state in E.STATES:
        for name, (dirs, either) in E.direction_sets(S).items():
            r = _oracle_ratio(dirs, faces, state, either)
            k = int(r.argmax())
            print(f"ENV_MEASURE oracle direct {kind} S={S} state={state} set={name} n={len(dirs)} worst_ratio={r[k]:.4f}")
            if r[k] > ORACLE_MAX_RATIO and kind == "coordinate" and state[1] > 1.0:
                got = oracle.env(dirs[k:k + 1], faces, state[0], state[1])[0]
                print("  direction", dirs[k], "oracle looked at (face, x, y)", E.decode(got, S, state[0]),
                      "model", E.decode(env_ref.lookup(dirs[k:k + 1], faces, *state)[0][0], S, state[0]))
            assert r[k] <= ORACLE_MAX_RATIO, (kind, S, state, name, dirs[k], r[k])
            worst = max(worst, float(r[k]))
    print(f"ENV_MEASURE oracle direct {kind} S={S} all worst_ratio={worst:.4f}")


@pytest.mark.parametrize("kind,S", MAPS)
def test_every_mutant_is_rejected(kind, S):
    """A wrong texel, face or flip exceeds the bound by orders of magnitude: each wrong variant of the model misses
    the (right) oracle on every map, through the same measure and the same acceptance the real comparison uses."""
    faces = E.env_map(kind, S)
    sets = E.direction_sets(S)
    for mutant in env_ref.MUTANTS:
        # over the states, as the real comparison runs: (2.5, 0.75) clamps most of a noise map to one value, which
        # hides a wrong texel, and only a state that clamps can show a clamp in the wrong place
        worst = max(float(_oracle_ratio(dirs, faces, state, either, mutant).max())
                    for state in E.STATES for dirs, either in sets.values())
        print(f"ENV_MEASURE mutant {mutant} {kind} S={S} worst_ratio={worst:.3g}")
        assert worst >= MUTANT_MIN_RATIO, (mutant, kind, S, worst)


def test_a_wrong_tie_order_shows_only_on_exact_ties():
    """What set B is for: the y-before-x mutant passes on the uniform sphere and fails on the ties."""
    faces = E.env_map("noise", 16)
    assert _oracle_ratio(E.dirs_uniform(), faces, E.DEFAULT_STATE, False, "y_before_x").max() <= ORACLE_MAX_RATIO
    assert _oracle_ratio(E.dirs_ties(), faces, E.DEFAULT_STATE, False, "y_before_x").max() >= MUTANT_MIN_RATIO


# ---- the mirror room ----------------------------------------------------------------------------------------------
def test_mirror_room_model():
    rays = E.room_rays()
    assert rays.shape == (20000, 3) and rays.dtype == np.float32
    k, final, drop = E.mirror_paths(E.ROOM_ORIGIN, rays)
    shares = np.bincount(k, minlength=4) / len(k)
    print("mirror paths of 0, 1, 2, 3 mirrors:", shares, "dropped by the model:", int(drop.sum()))
    assert drop.sum() == 0
    assert (shares[1:4] >= 0.20).all() and shares[0] == 0.0
    assert (np.abs(final) == np.abs(rays)).all() and (final > 0).all(axis=1)[k == 3].all()
    # the throughput is exact in float32
    thr = np.asarray(E.MIRROR_ALBEDO, np.float32)
    assert (np.log2(thr.astype(np.float64)) % 1 == 0).all()
    t, _ = A.staging_counts()
    for N, staged in ((E.ROOM_N_STAGED, True), (E.ROOM_N_UNSTAGED, False)):
        sc = E.room_scene(N)
        n = len(sc["indices"])
        assert n == 6 * N * N and (n <= t) == staged
        assert E.room_normals_exact(sc)
        assert (A.staged_bytes(n, n, 0, n) <= A.header_constant("kLdsSceneBytes")) == staged
    # the expectation: exactly 0 where the mirrors use up the depth, albedo^k * model elsewhere
    faces = E.env_map("noise", 3)
    for depth in (1, 2, 3, 6):
        val, tol, kk, _ = E.room_expectation(E.ROOM_ORIGIN, rays, faces, 2.5, 0.75, depth)
        assert (val[kk >= depth] == 0).all() and (tol[kk >= depth] == 0).all()
        assert depth == 1 or (val[kk < depth] > 0).any()  # (every ray of the set meets a mirror)
    # the oracle on the reflected directions, within half of the bound as on the sets
    for S, kind, state in E.SITE_CONFIGS:
        faces = E.env_map(kind, S)
        val, tol, _, _ = E.room_expectation(E.ROOM_ORIGIN, rays, faces, state[0], state[1], 6)
        err = np.abs(E.room_oracle(E.ROOM_ORIGIN, rays, faces, state, 6) - val)
        worst = float(np.where(err == 0, 0.0, err / tol).max())
        print(f"ENV_MEASURE oracle mirrors {kind} S={S} state={state} n={len(rays)} worst_ratio={worst:.4f}")
        assert worst <= ORACLE_MAX_RATIO
    one = np.flatnonzero(k == 2)[0]
    v, _, _ = env_ref.lookup(final[one:one + 1], faces, 2.5, 0.75)
    val, _, _, _ = E.room_expectation(E.ROOM_ORIGIN, rays[one:one + 1], faces, 2.5, 0.75, 6)
    assert np.array_equal(val[0], v[0] * np.array([0.25, 0.0625, 1.0]))


def test_far_scene_is_off_every_direction():
    """The direct-miss scene: no direction of any set passes within 1e-3 rad of its one triangle."""
    c = E.far_scene()["positions"].astype(np.float64).mean(axis=0)
    c /= np.linalg.norm(c)
    for S in (2, 3, 16):
        for name, (d, _) in E.direction_sets(S).items():
            assert (d.astype(np.float64) @ c).max() < np.cos(1e-3), name


# ---- the face-size limit ---------------------------------------------------------------------------------------------
def test_face_size_limit_is_the_index_range():
    """kMaxEnvSize is the largest S with 6 S^2 < 2^32 (the kernel's 32-bit texel index)."""
    s = A.header_constant("kMaxEnvSize")
    assert 6 * s * s < 2 ** 32 <= 6 * (s + 1) * (s + 1) and s == 26754
    assert 6 * s < 2 ** 24  # and both operands of the 24-bit row multiply stay in range
