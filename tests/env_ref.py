"""A float64 model of the cubemap environment lookup, in numpy only: what env_color<true>
(csrc/kernels_wavefront.hip) and the oracle's env_color (oracle/wf_oracle.cpp) are both held to.

Written from the formulas of Cubemap::directionToUV, bilinearSample and EnvironmentManager::getCubemapColor,
not from either restatement:

  d = dir / |dir|                                                       (float64)
  face: x-major if |x| >= |y| and |x| >= |z|, else y-major if |y| >= |x| and |y| >= |z|, else z-major;
        the positive face if the major component is > 0
  (uc, vc): +X (-z, -y)   -X (z, -y)   +Y (x, z)   -Y (x, -z)   +Z (x, -y)   -Z (-x, -y)
  u = clamp((uc / ma + 1) / 2, 0, 1), x = u (S - 1), x0 = floor(x), x1 = min(x0 + 1, S - 1); v, y alike
  c = mix along x, then along y, of texels faces[face, y, x]
  result = min(c, max_clamp) * intensity

lookup() also returns the error bound of a float32 evaluation, per direction and channel.  With eps = 2^-24:
a float32 unit direction reaches u with an error of at most 4 eps (renormalisation <= 4 eps on a ratio of
magnitude <= 1, the division <= eps, the + 1 <= 2 eps, and the sum is halved); the bound takes du = 8 eps for
directions a test supplies and 8 eps more per axis-aligned mirror bounce before the lookup (reflect about an
axis is exact, safe_normalize adds <= 2 eps per component: DU_MIRROR = 16 eps after one).  Then
dx = (S - 1) (du + eps), and

  tol_c = intensity * ((dx + dy) * D_c + 16 eps * M_c)

with D_c the largest absolute difference of 8-neighbour texels of a face in channel c and M_c the largest texel
value: the bilinear interpolant is continuous across cell borders and its slope along x or y is at most D_c, so a
floor() that lands on the other side of an integer costs nothing extra; min(., max_clamp) does not expand errors;
16 eps * M_c covers the roundings of the three mixes and the final product.
"""
import numpy as np

f64 = np.float64
EPS = 2.0 ** -24
DU_DIRECT = 8 * EPS
DU_MIRROR = 16 * EPS

# per face: (index of uc's component, its sign, index of vc's component, its sign)
UV_TABLE = {
    0: (2, -1.0, 1, -1.0),  # +X (-z, -y)
    1: (2, +1.0, 1, -1.0),  # -X ( z, -y)
    2: (0, +1.0, 2, +1.0),  # +Y ( x,  z)
    3: (0, +1.0, 2, -1.0),  # -Y ( x, -z)
    4: (0, +1.0, 1, -1.0),  # +Z ( x, -y)
    5: (0, -1.0, 1, -1.0),  # -Z (-x, -y)
}
MUTANTS = ("swap_uv", "negated_sign", "x1_is_x0", "clamp_after_intensity", "y_before_x", "face_sign_swapped")


def du_after(mirrors: int) -> float:
    """du of a direction that went through this many axis-aligned mirror bounces."""
    return DU_DIRECT * (1 + mirrors)


def map_stats(faces):
    """(D, M) per channel: the largest 8-neighbour texel difference within a face, and the largest texel."""
    f = np.asarray(faces, f64)
    d = np.zeros(3)
    for a in (f[:, 1:, :] - f[:, :-1, :], f[:, :, 1:] - f[:, :, :-1], f[:, 1:, 1:] - f[:, :-1, :-1],
              f[:, 1:, :-1] - f[:, :-1, 1:]):
        if a.size:
            d = np.maximum(d, np.abs(a).reshape(-1, 3).max(axis=0))
    return d, np.abs(f).reshape(-1, 3).max(axis=0)


def major_axis(d, mutant=None):
    """The major axis (0, 1, 2) of each row of d in the reference's order of tests."""
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    xm = (ax >= ay) & (ax >= az)
    ym = (ay >= ax) & (ay >= az)
    if mutant == "y_before_x":
        return np.where(ym, 1, np.where(xm, 0, 2))
    return np.where(xm, 0, np.where(ym, 1, 2))


def lookup(dirs, faces, intensity=0.8, max_clamp=5.0, du=DU_DIRECT, axis=None, mutant=None, stats=None):
    """(value (n, 3), tol (n, 3), face (n,)) float64 for float32 (or any) directions.

    axis: the major axis to take per direction instead of the rule's (near a seam a float32 evaluation may
    land on the neighbouring face).  du: scalar or (n,).  mutant: one of MUTANTS, a deliberately wrong variant.
    stats: map_stats(faces), if the caller has it."""
    assert mutant is None or mutant in MUTANTS
    faces = np.asarray(faces, f64)
    S = faces.shape[1]
    assert faces.shape == (6, S, S, 3) and S >= 2
    d = np.asarray(dirs, f64).reshape(-1, 3)
    d = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
    n = len(d)
    rows = np.arange(n)
    maj = major_axis(d, mutant) if axis is None else np.asarray(axis, np.int64)
    dm = d[rows, maj]
    pos = dm > 0
    if mutant == "face_sign_swapped":
        pos = ~pos
    face = 2 * maj + np.where(pos, 0, 1)
    ma = np.abs(dm)
    uc, vc = np.empty(n), np.empty(n)
    for f, (iu, su, iv, sv) in UV_TABLE.items():
        if mutant == "negated_sign" and f == 0:
            su = -su
        m = face == f
        uc[m] = su * d[m, iu]
        vc[m] = sv * d[m, iv]
    if mutant == "swap_uv":
        uc, vc = vc, uc
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.clip((uc / ma + 1.0) * 0.5, 0.0, 1.0)
        v = np.clip((vc / ma + 1.0) * 0.5, 0.0, 1.0)
    x, y = u * (S - 1), v * (S - 1)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, S - 1), np.minimum(y0 + 1, S - 1)
    if mutant == "x1_is_x0":
        x1 = x0
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    c0 = faces[face, y0, x0] * (1.0 - fx) + faces[face, y0, x1] * fx
    c1 = faces[face, y1, x0] * (1.0 - fx) + faces[face, y1, x1] * fx
    c = c0 * (1.0 - fy) + c1 * fy
    if mutant == "clamp_after_intensity":
        value = np.minimum(c * f64(intensity), f64(max_clamp))
    else:
        value = np.minimum(c, f64(max_clamp)) * f64(intensity)
    D, M = map_stats(faces) if stats is None else stats
    dx = (S - 1) * (np.broadcast_to(np.asarray(du, f64), (n,)) + EPS)
    tol = abs(f64(intensity)) * (2.0 * dx[:, None] * D[None, :] + 16 * EPS * M[None, :])
    return value, tol, face


def near_axes(dirs, ulps=64):
    """Per direction the axes whose float32 magnitude lies within `ulps` float32 ulps of the largest one: the
    major axes a float32 evaluation of a direction next to a seam may take."""
    a = np.abs(np.asarray(dirs, f64).reshape(-1, 3))
    top = a.max(axis=1, keepdims=True)
    return a >= top * (1.0 - ulps * 2.0 ** -23)


def ratio(got, dirs, faces, intensity=0.8, max_clamp=5.0, du=DU_DIRECT, either_face=False, mutant=None, scale=None):
    """(n,) worst |got - model| / tol over the channels, per direction; with either_face the smallest over the
    candidate major axes of near_axes.  scale: (n, 3) exact factors on value and bound (a path's throughput).
    A tol of 0 (a channel the map holds constant 0) gives 0 for an exact match, else inf."""
    got = np.asarray(got, f64).reshape(-1, 3)
    faces = np.asarray(faces, f64)
    stats = map_stats(faces)

    def one(axis):
        val, tol, _ = lookup(dirs, faces, intensity, max_clamp, du, axis=axis, mutant=mutant, stats=stats)
        if scale is not None:
            val, tol = val * scale, tol * np.abs(scale)
        err = np.abs(got - val)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0.0, 0.0, err / tol)
        return np.where(np.isnan(r), np.inf, r).max(axis=1)

    best = one(None)
    if either_face:
        cand = near_axes(dirs)
        d = np.asarray(dirs, f64).reshape(-1, 3)
        for a in range(3):
            m = cand[:, a]
            if m.any():
                r = one(np.where(m, a, major_axis(d / np.sqrt((d * d).sum(axis=1, keepdims=True)))))
                best = np.where(m, np.minimum(best, r), best)
    return best
