"""Maps, environment states, direction sets and the mirror room shared by test_env_ref_cpu.py and
test_gpu_env.py (test infrastructure, numpy only; the float64 model is tests/env_ref.py).

Maps (6, S, S, 3) float32, texel (face, x, y) = faces[face, y, x]:
  coordinate  R = (face + 1) / 8, G = (x + 1) / (S + 1), B = (y + 1) / (S + 1): G and B are linear in the pixel
              coordinate, so a lookup returns where it looked (decode());
  noise       texels from {0, 0.25, ..., 7.75} per channel, fixed seed: uncorrelated neighbours, many above the
              clamps of STATES.
Direction sets (float32 unit vectors): A uniform sphere, B exact ties, C axes, D near seams, E the texel grid."""
import itertools

import numpy as np

import env_ref

f32, f64 = np.float32, np.float64
SIZES = (2, 3, 16, 257)
STATES = ((0.8, 5.0), (2.5, 0.75), (1.0, 1e30))  # (intensity, max_clamp)
DEFAULT_STATE = STATES[0]
KINDS = ("coordinate", "noise")
# the two configurations of the sites that do not run the full product
SITE_CONFIGS = ((3, "noise", (2.5, 0.75)), (16, "coordinate", DEFAULT_STATE))


def coordinate_map(S):
    f = np.empty((6, S, S, 3), f64)
    f[..., 0] = ((np.arange(6) + 1) / 8.0)[:, None, None]
    f[..., 1] = ((np.arange(S) + 1) / (S + 1.0))[None, None, :]
    f[..., 2] = ((np.arange(S) + 1) / (S + 1.0))[None, :, None]
    return f.astype(f32)


def noise_map(S, seed=1234):
    return (np.random.default_rng(seed + S).integers(0, 32, (6, S, S, 3)) * 0.25).astype(f32)


_maps = {}


def env_map(kind, S):
    if (kind, S) not in _maps:
        m = coordinate_map(S) if kind == "coordinate" else noise_map(S)
        m.setflags(write=False)
        _maps[(kind, S)] = m
    return _maps[(kind, S)]


def decode(rgb, S, intensity=1.0):
    """(face, x, y) a colour of the coordinate map stands for (unclamped states only), for failure messages."""
    c = np.asarray(rgb, f64) / intensity
    return float(c[0] * 8 - 1), float(c[1] * (S + 1) - 1), float(c[2] * (S + 1) - 1)


# ---- directions ---------------------------------------------------------------------------------------------
def _unit32(v):
    """Rows of v (float64) scaled to unit length, rounded to float32."""
    v = np.asarray(v, f64).reshape(-1, 3)
    return (v / np.sqrt((v * v).sum(axis=1, keepdims=True))).astype(f32)


def _scaled32(v32):
    """float32 rows times one float32 factor per row (1 / length): components of equal magnitude stay bitwise
    equal in magnitude."""
    v32 = np.asarray(v32, f32).reshape(-1, 3)
    s = (1.0 / np.sqrt((v32.astype(f64) ** 2).sum(axis=1))).astype(f32)
    return v32 * s[:, None]


def dirs_uniform(n=20000, seed=7):
    """A: uniform on the sphere."""
    return _unit32(np.random.default_rng(seed).normal(size=(n, 3)))


def dirs_ties(seed=8, per=200):
    """B: the 12 cube edges, the 8 corners, and `per` each of (a, +-a, b), (a, b, +-a), (b, a, +-a) with
    |b| < |a| under every sign pattern; the tied float32 components are bitwise equal in magnitude."""
    rows = []
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for si, sj in itertools.product((1.0, -1.0), repeat=2):
            v = np.zeros(3)
            v[i], v[j] = si, sj
            rows.append(v)
    rows += [np.array(s) for s in itertools.product((1.0, -1.0), repeat=3)]
    g = np.random.default_rng(seed)
    signs = np.array(list(itertools.product((1.0, -1.0), repeat=3)))
    for i, j, k in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):  # tied components i, j; the smaller one k
        a = g.uniform(0.2, 1.0, per).astype(f32).astype(f64)
        b = (a * g.uniform(0.0, 0.999, per)).astype(f32).astype(f64)
        for m in range(per):
            v = np.empty(3)
            v[i], v[j], v[k] = a[m], a[m], b[m]
            rows.append(v * signs[m % 8])
    d = _scaled32(np.array(rows, f32))
    a = np.abs(d)
    top = a.max(axis=1, keepdims=True)
    assert ((a.view(np.uint32) == top.view(np.uint32)).sum(axis=1) >= 2).all()  # an exact tie at the top
    assert len(d) == 20 + 3 * per
    return d


def tied_pair(d):
    """For rows with an exact tie at the top: the indices (i, j) of the first two tied components."""
    a = np.abs(np.asarray(d, f32))
    t = a == a.max(axis=1, keepdims=True)
    i = t.argmax(axis=1)
    t2 = t.copy()
    t2[np.arange(len(a)), i] = False
    return i, t2.argmax(axis=1)


def dirs_axes():
    """C: the six axes with every +0.0 / -0.0 in the minor components, and with minor components of 1e-30, 1e-38
    and a denormal (quotients below 2^-100: the division's unhandled range, where q + 1 must round to 1)."""
    rows = []
    for axis in range(3):
        minor = [k for k in range(3) if k != axis]
        for s in (1.0, -1.0):
            for t in (0.0, 1e-30, 1e-38, 4e-45):
                for sa, sb in itertools.product((1.0, -1.0), repeat=2):
                    v = np.zeros(3, f32)
                    v[axis] = s
                    v[minor[0]] = np.copysign(f32(t), f32(sa))
                    v[minor[1]] = np.copysign(f32(t), f32(sb))
                    rows.append(v)
    d = np.array(rows, f32)
    assert len(d) == 96 and (np.abs(d).max(axis=1) == 1.0).all()
    return d


def dirs_near_seams():
    """D: set B with one of the tied components moved by 1, 2 and 16 ulps either way (each of the two in turn)."""
    b = dirs_ties()
    i, j = tied_pair(b)
    out = []
    for comp in (i, j):
        for k in (1, 2, 16, -1, -2, -16):
            d = b.copy()
            bits = d.view(np.int32)  # the magnitude bits of a float32 order like integers
            bits[np.arange(len(d)), comp] += k
            out.append(d)
    d = np.concatenate(out)
    assert np.isfinite(d).all() and len(d) == 12 * len(b)
    return d


def dirs_texel_grid(S):
    """E: for every face the directions through every texel centre (u or v exactly 0 or 1 among them: the last
    row and column, where x1 and y1 are clamped) and every cell midpoint.  Returns (dirs, face, gx, gy) with the
    grid coordinates in texels (integers: centres; halves: midpoints)."""
    g = np.arange(2 * S - 1) * 0.5
    gx, gy = np.meshgrid(g, g, indexing="xy")
    gx, gy = gx.ravel(), gy.ravel()
    dirs, face = [], []
    for f, (iu, su, iv, sv) in env_ref.UV_TABLE.items():
        v = np.zeros((len(gx), 3))
        v[:, f // 2] = 1.0 if f % 2 == 0 else -1.0
        v[:, iu] = su * (2.0 * gx / (S - 1) - 1.0)  # uc = su * d[iu]
        v[:, iv] = sv * (2.0 * gy / (S - 1) - 1.0)
        dirs.append(v)
        face.append(np.full(len(gx), f))
    return _unit32(np.concatenate(dirs)), np.concatenate(face), np.tile(gx, 6), np.tile(gy, 6)


def direction_sets(S):
    """{name: (dirs, either_face)} of the sets a map of face size S is looked up with."""
    sets = {"A": (dirs_uniform(), False), "B": (dirs_ties(), False), "C": (dirs_axes(), False),
            "D": (dirs_near_seams(), True)}
    if S <= 16:
        sets["E"] = (dirs_texel_grid(S)[0], False)
    return sets


def face_shares(dirs):
    _, _, face = env_ref.lookup(dirs, coordinate_map(2))
    return np.bincount(face, minlength=6) / len(face)


# ---- a scene no test direction hits: the direct-miss tests need one uploaded -----------------------------------
FAR_ORIGIN = (0.0, 0.0, 0.0)


def far_scene():
    """One millimetre-sized triangle 1 200 units away in a direction no set contains."""
    c = np.array([1000.0, 337.0, -571.0])
    p = np.array([c, c + [1e-3, 0, 0], c + [0, 1e-3, 0]], f32)
    return {"positions": p, "indices": np.array([[0, 1, 2]], np.uint32), "tri_geom_first": np.array([0, 1], np.uint32),
            "spheres": np.zeros((0, 4), f32), "geom_material": np.array([0], np.uint32)}


# ---- the mirror room ------------------------------------------------------------------------------------------
# Three mirrors meeting in the corner (-4, 0, -4): plane axis, its coordinate, and the extents of the other two axes
MIRRORS = ((1, 0.0, {0: (-4.0, 4.0), 2: (-4.0, 4.0)}),   # the floor y = 0
           (0, -4.0, {1: (0.0, 8.0), 2: (-4.0, 4.0)}),   # the wall x = -4
           (2, -4.0, {0: (-4.0, 4.0), 1: (0.0, 8.0)}))   # the wall z = -4
MIRROR_ALBEDO = (0.5, 0.25, 1.0)  # metallic 1: the throughput per bounce, exact powers of two
ROOM_ORIGIN = (2.5, 3.0, 2.0)
BORDER = 1e-3
ROOM_N_STAGED, ROOM_N_UNSTAGED = 4, 16  # tessellations (powers of two: every vertex and normal exact in float32)


def room_scene(N):
    """The three mirrors, each N x N quads of two triangles, as one geometry of material 0."""
    pos, idx = [], []
    for axis, at, ext in MIRRORS:
        (a, (a0, a1)), (b, (b0, b1)) = sorted(ext.items())
        ga, gb = np.meshgrid(np.linspace(a0, a1, N + 1), np.linspace(b0, b1, N + 1), indexing="ij")
        p = np.zeros(((N + 1) * (N + 1), 3))
        p[:, axis], p[:, a], p[:, b] = at, ga.ravel(), gb.ravel()
        i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        v00 = (i * (N + 1) + j).ravel()
        v10, v01, v11 = v00 + N + 1, v00 + 1, v00 + N + 2
        t = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)])
        idx.append(t + sum(len(q) for q in pos))
        pos.append(p)
    p = np.concatenate(pos)
    assert (p.astype(f32) == p).all()
    t = np.concatenate(idx).astype(np.uint32)
    return {"positions": p.astype(f32), "indices": t, "tri_geom_first": np.array([0, len(t)], np.uint32),
            "spheres": np.zeros((0, 4), f32), "geom_material": np.array([0], np.uint32)}


def room_normals_exact(scene):
    """Whether the float32 unit normal of every triangle, cross(e1, e2) * (1 / sqrt(l2)) with each operation
    rounded, is exactly an axis: then reflect() about it is exact."""
    p, t = scene["positions"], scene["indices"].astype(np.int64)
    e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    n = np.cross(e1, e2).astype(f32)
    l2 = (n * n).sum(axis=1, dtype=f32)
    u = n * (f32(1.0) / np.sqrt(l2))[:, None]
    return bool(((np.abs(u) == 1.0).sum(axis=1) == 1).all() and ((u == 0.0).sum(axis=1) == 2).all())


def room_rays(n=20000, seed=21):
    """Unit float32 directions from ROOM_ORIGIN towards seeded interior points of the three mirrors: 0.6 of them
    anywhere on a mirror, the others within 2.5 of the corner, every target at least 0.05 from the mirror's
    border.  Candidates whose later hits (or passes beside a mirror) come within 0.01 of a border are not aimed at
    an interior either and are left out while the set is drawn, so the model itself drops no ray of the set."""
    g = np.random.default_rng(seed)
    m = n + n // 8
    which = g.integers(0, 3, m)
    wide = g.random(m) < 0.6
    tg = np.empty((m, 3))
    for k, (axis, at, ext) in enumerate(MIRRORS):
        sel = which == k
        tg[sel, axis] = at
        for a, (lo, hi) in ext.items():
            top = np.where(wide[sel], hi - 0.05, lo + 2.5)
            tg[sel, a] = g.uniform(lo + 0.05, top)
    d = _unit32(tg - np.array(ROOM_ORIGIN))
    d = d[~mirror_paths(ROOM_ORIGIN, d, border=0.01)[2]]
    assert len(d) >= n
    return d[:n]


def mirror_paths(origin, dirs, border=BORDER):
    """The float64 model of the paths of rays through the mirror room, by ray-plane arithmetic.

    Returns (k, final, drop): the number of mirrors each ray meets (0..3), its direction after the last of them
    (the float32 input with the mirrors' components negated: exact) and whether a hit, or a pass beside a
    mirror, lies within `border` of a mirror's border (the corner lines are borders)."""
    d32 = np.asarray(dirs, f32).reshape(-1, 3)
    n = len(d32)
    d = d32.astype(f64)
    o = np.broadcast_to(np.asarray(origin, f64), (n, 3)).copy()
    final = d32.copy()
    k = np.zeros(n, np.int64)
    drop = np.zeros(n, bool)
    alive = np.ones(n, bool)
    last = np.full(n, -1)
    for step in range(4):
        best_t = np.full(n, np.inf)
        best_m = np.full(n, -1)
        near_t = np.full(n, np.inf)  # the nearest plane crossing within `border` of a mirror's border
        for mi, (axis, at, ext) in enumerate(MIRRORS):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (at - o[:, axis]) / d[:, axis]
            ok = alive & (last != mi) & np.isfinite(t) & (t > 0)
            margin = np.full(n, np.inf)
            for a, (lo, hi) in ext.items():
                c = o[:, a] + t * d[:, a]
                margin = np.minimum(margin, np.minimum(c - lo, hi - c))
            hit = ok & (margin > 0) & (t < best_t)
            best_t = np.where(hit, t, best_t)
            best_m = np.where(hit, mi, best_m)
            close = ok & (np.abs(margin) < border)
            near_t = np.where(close, np.minimum(near_t, t), near_t)
        drop |= alive & np.isfinite(near_t) & (near_t <= best_t)
        hitting = alive & (best_m >= 0)
        if not hitting.any():
            break
        assert step < 3, "a ray met a fourth mirror"
        for mi, (axis, at, ext) in enumerate(MIRRORS):
            m = hitting & (best_m == mi)
            o[m] = o[m] + best_t[m, None] * d[m]
            o[m, axis] = at
            d[m, axis] = -d[m, axis]
            final[m, axis] = -final[m, axis]
        k[hitting] += 1
        last = np.where(hitting, best_m, last)
        alive = hitting
    return k, final, drop


def room_expectation(origin, dirs, faces, intensity, max_clamp, max_depth):
    """(value, tol, k, drop) of the radiance of rays through the mirror room under a cubemap, no light and no
    emission: albedo^k * model(final direction), exactly 0 when the path's k mirrors use up max_depth segments."""
    k, final, drop = mirror_paths(origin, dirs)
    val, tol, _ = env_ref.lookup(final, faces, intensity, max_clamp, du=env_ref.du_after(k))
    thr = np.asarray(MIRROR_ALBEDO, f64)[None, :] ** k[:, None]
    ended = (k >= max_depth)[:, None]
    return np.where(ended, 0.0, val * thr), np.where(ended, 0.0, tol * thr), k, drop


def room_oracle(origin, dirs, faces, state, max_depth):
    """The float32 oracle's lookup in room_expectation's place: oracle.env of the model's final directions times
    the (exact) throughput; what holds the oracle to the bound after mirror bounces."""
    import oracle

    k, final, _ = mirror_paths(origin, dirs)
    thr = np.asarray(MIRROR_ALBEDO, f64)[None, :] ** k[:, None]
    return np.where((k >= max_depth)[:, None], 0.0, oracle.env(final, faces, state[0], state[1]).astype(f64) * thr)
