"""Shared inputs of the closest-point tests (test_points_cpu.py, test_gpu_points.py): fixed-seed point sets per query
scene (refit_common.SCENES), the host twin's answers and the float64 reference's, each computed once per process and
read-only, and the bounds both tests hold results to.

Point sets of a scene (rows p.xyz, max_dist), in this order in points(name):
  box      1536 points uniform in the scene's bounds grown by half about their centre, max_dist = inf;
  near     1536 surface samples (a primitive by default_rng, a uniform point on it) moved along the unit normal by
           +-10^e, e uniform in [-6, 0], max_dist = inf;
  feature  the vertices, edge midpoints and centroid of the first 512 triangles (float64, cast to float32), and of
           every sphere the centre and the six axis poles, max_dist = inf;
  far      64 points 10^3 away from the centre in uniform directions, max_dist = inf;
  radius   the first 64 box points six times, with max_dist = 0, inf, -1, NaN, and nextafter below and above the
           host twin's dist for that point;
  nonfinite 18 points: +inf, -inf and NaN in each coordinate of two box points, max_dist = inf.

For an adversarial_common case (ADVERSARIAL: tiny with 0, 1, 2, 5 and 9 primitives of each kind, equal, degenerate,
scale, offset, deep, and the staging case one triangle above the staged count) the points are its rays' origins and
origin + d, max_dist = inf.

Bounds.  eps = 2^-24; M of a point is max(|p|_inf, the scene's largest absolute coordinate).
  PAD = 16 eps M     csrc/closest_point.h's kCpPad, the margin of node_bound: the twin never reports closer than
                     the float64 truth by more than this (lower side).
  UPPER_RECORDED     max (dist - dist64) / (eps M) measured over these sets on both scenes with the host twin
                     (profiles/point_query_measurements.txt); the tests assert 4 x this value (upper side)."""
import functools

import numpy as np

import adversarial_common as A
import oracle
import points_ref as PR
import refit_common as R
import sptr

EPS = 2.0 ** -24
PAD = 16.0
UPPER_RECORDED = 1.35
SET_NAMES = ("box", "near", "feature", "far", "radius", "nonfinite")
FIELDS = ("geom", "prim", "dist2", "dist", "point", "uv", "ng")
NBOX = NNEAR = 1536


def flat(sc):
    return sptr.FlatScene(sc["positions"], sc["indices"], sc["tri_geom_first"], sc["spheres"], sc["geom_material"])


def scene_magnitude(sc):
    m = 0.0
    if len(sc["indices"]):
        m = float(np.abs(sc["positions"].astype(np.float64)[np.unique(sc["indices"].astype(np.int64))]).max())
    if len(sc["spheres"]):
        s = sc["spheres"].astype(np.float64)
        m = max(m, float((np.abs(s[:, :3]) + s[:, 3:4]).max()))
    return m


def magnitudes(sc, pts):
    """M per point (float64); non-finite coordinates give inf or nan."""
    with np.errstate(invalid="ignore"):
        return np.maximum(np.abs(np.asarray(pts, np.float64)[:, :3]).max(axis=1), scene_magnitude(sc))


def _pack(p, max_dist=np.inf):
    out = np.zeros((len(p), 4), np.float32)
    out[:, :3] = p
    out[:, 3] = max_dist
    return out


def _near(sc, rng, n):
    idx = sc["indices"].astype(np.int64)
    pos = sc["positions"].astype(np.float64)
    live = np.flatnonzero((A.stored_normals(sc) != 0.0).any(axis=1)) if len(idx) else np.zeros(0, np.int64)
    sph = sc["spheres"].astype(np.float64)
    which = rng.integers(0, len(live) + len(sph), n)
    off = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, 0.0, n)
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    out = np.zeros((n, 3))
    for k in range(n):
        if which[k] < len(live):
            a, b, c = pos[idx[live[which[k]]]]
            q = (1.0 - r1[k]) * a + r1[k] * (1.0 - r2[k]) * b + r1[k] * r2[k] * c
            nrm = np.cross(b - a, c - a)
            out[k] = q + off[k] * nrm / np.linalg.norm(nrm)
        else:
            s = sph[which[k] - len(live)]
            out[k] = s[:3] + (s[3] + off[k]) * dirs[k]
    return out


def _features(sc):
    idx = sc["indices"].astype(np.int64)[:512]
    p = sc["positions"].astype(np.float64)[idx]  # (T, 3, 3)
    parts = []
    if len(idx):
        a, b, c = p[:, 0], p[:, 1], p[:, 2]
        parts += [a, b, c, 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a), (a + b + c) / 3.0]
    s = sc["spheres"].astype(np.float64)
    if len(s):
        parts.append(s[:, :3])
        for ax in range(3):
            for sg in (-1.0, 1.0):
                q = s[:, :3].copy()
                q[:, ax] += sg * s[:, 3]
                parts.append(q)
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, 3))


@functools.lru_cache(maxsize=None)
def query_scene(name):
    cfg = next(c for c in R.SCENES if c[0] == name)
    return oracle.builtin_scene(cfg[0], cfg[1], cfg[2])


@functools.lru_cache(maxsize=None)
def point_sets(name):
    """{set name: (n, 4) float32, read-only} of the query scene `name`."""
    sc = query_scene(name)
    rng = np.random.default_rng(41)
    c, _, lo, hi = A.bounds(sc)
    half = 0.5 * (hi - lo)
    sets = {"box": _pack(rng.uniform(c - 1.5 * half, c + 1.5 * half, (NBOX, 3))),
            "near": _pack(_near(sc, rng, NNEAR)), "feature": _pack(_features(sc))}
    d = rng.normal(size=(64, 3))
    sets["far"] = _pack(c + 1e3 * d / np.linalg.norm(d, axis=1, keepdims=True))
    base = sets["box"][:64]
    dist = sptr.host_query_points(flat(sc), base, fields=("dist",))["dist"]
    rad = [_pack(base[:, :3], v) for v in (0.0, np.inf, -1.0, np.nan)]
    for to in (np.float32(0.0), np.float32(np.inf)):
        r = base.copy()
        r[:, 3] = np.nextafter(dist, to)
        rad.append(r)
    sets["radius"] = np.concatenate(rad, axis=0)
    bad = []
    for k in range(2):
        for ax in range(3):
            for v in (np.inf, -np.inf, np.nan):
                q = sets["box"][100 + k].copy()
                q[ax] = v
                bad.append(q)
    sets["nonfinite"] = np.stack(bad)
    assert tuple(sets) == SET_NAMES
    for a in sets.values():
        a.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def points(name):
    """((n, 4) float32 of all sets in order, {set name: slice})."""
    sets = point_sets(name)
    where, at = {}, 0
    for k, a in sets.items():
        where[k] = slice(at, at + len(a))
        at += len(a)
    allp = np.concatenate(list(sets.values()), axis=0)
    allp.setflags(write=False)
    return allp, where


def _frozen(res):
    for a in res.values():
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def twin(name):
    """The host twin's answers for points(name)."""
    return _frozen(sptr.host_query_points(flat(query_scene(name)), points(name)[0]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """points_ref.nearest for points(name) (every row, whatever its max_dist)."""
    return _frozen(PR.nearest(query_scene(name), points(name)[0]))


_TINY = [3 * A.COUNTS.index(n) + kind for n in (0, 1, 2, 5, 9) for kind in range(3)]
ADVERSARIAL = ([("tiny", i) for i in _TINY] + [("equal", i) for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17)]
               + [("degenerate", i) for i in range(4)] + [("scale", i) for i in range(3)] + [("offset", i) for i in range(3)]
               + [("deep", 0), ("deep", 1), ("staging", 2)])
ADVERSARIAL_IDS = [f"{f}{k}" for f, k in ADVERSARIAL]


def case_points(case):
    r = case.rays.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.concatenate([r[:, 0:3], r[:, 0:3] + r[:, 3:6]], axis=0)
    out = _pack(p)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_twin(fam, k):
    """(adversarial case, its points, the host twin's answers)."""
    case = A.family(fam)[k]
    pts = case_points(case)
    return case, pts, _frozen(sptr.host_query_points(flat(case.scene), pts))


def check_against_reference(sc, pts, got, ref, what, upper_eps=4.0 * UPPER_RECORDED, sliver=False):
    """The CPU test's bounds for rows with finite coordinates and max_dist = inf; prints the measured figures.
    Returns (max lower-side excess, max upper-side excess) in eps M."""
    p64 = np.asarray(pts, np.float64)
    sel = np.isfinite(p64[:, :3]).all(axis=1) & np.isposinf(p64[:, 3]) & np.isfinite(ref["dist"])
    M = magnitudes(sc, pts)[sel]
    d, d64 = got["dist"].astype(np.float64)[sel], ref["dist"][sel]
    assert np.isfinite(d).all(), what
    low = (d64 - d) / (EPS * M)
    up = (d - d64) / (EPS * M)
    print(f"{what}: {int(sel.sum())} points; closer than float64 by at most {low.max(initial=0.0):.3f} eps M (bound {PAD}), "
          f"farther by at most {up.max(initial=0.0):.3f} eps M (p99.9 {np.quantile(up, 0.999) if len(up) else 0.0:.3f})")
    assert (low <= PAD).all(), what
    if sliver:  # grows with the nearest triangle's conditioning: bounded by its smallest height
        assert (d - d64 <= np.maximum(ref["height"][sel], upper_eps * EPS * M)).all(), what
    else:
        assert (up <= upper_eps).all(), what
    return float(low.max(initial=0.0)), float(up.max(initial=0.0))
