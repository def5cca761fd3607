"""Shared checks of the ray-query tests (test_query_cpu.py, test_gpu_query.py): the barycentrics of a
triangle hit.

Convention (include/sptr_hip.h, sptr_query_rays): with the triangle's vertices v0, v1, v2 in the order of the
uploaded index triple, e1 = v0 - v1, e2 = v2 - v0, Ng = cross(e2, e1), C = v0 - o, R = cross(C, d),
den = dot(Ng, d): u = sign(den) dot(R, e2) / |den|, v = sign(den) dot(R, e1) / |den|, and the hit point is
(1 - u - v) v0 + u v1 + v v2.  These are Embree's Moeller-Trumbore terms, the ones the traversal's triangle
test evaluates in float32 with fused multiply-adds (tri_hit4).

Reference: the same terms in float64 on the float32 inputs (u64, v64, den64).  Bound on the float32 result:
  max(|u - u64|, |v - v64|) <= 16 * 2^-24 * |v0 - o| |d| max(|e1|, |e2|) / |den64| + 4 * 2^-24,
the forward error of the two cross and dot products (each term of dot(R, e) is at most |C| |d| |e|, and a
handful of roundings of that size go into it) over the denominator, plus the roundings of the quotient; the
factor 16 leaves about 3 in hand.  Also u, v in [0, 1] and u + v <= 1 + 2^-22 (the test accepts U + V <= |den|
before the two divisions round)."""
import numpy as np

f32, f64 = np.float32, np.float64
MISS = 0xFFFFFFFF
EPS = 2.0 ** -24


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _norm(a):
    return np.sqrt(_dot(a, a))


def triangle_hits(tri_geom_first, geom, prim):
    """(mask of the rays that hit a triangle, their indices into the uploaded triangle list)."""
    first = np.asarray(tri_geom_first, np.int64)
    geom = np.asarray(geom, np.int64)
    mask = (geom != MISS) & (geom < len(first) - 1)
    return mask, first[geom[mask]] + np.asarray(prim, np.int64)[mask]


def reference_uv(positions, indices, rays, tri):
    """float64 on the float32 inputs: u64, v64, den64, the bound above, and the distance between the two
    forms of the hit point, (1 - u - v) v0 + u v1 + v v2 and o + t d (which pins the vertex convention)."""
    p = np.asarray(positions, f32).astype(f64)
    i = np.asarray(indices, np.int64)[tri]
    v0, v1, v2 = p[i[:, 0]], p[i[:, 1]], p[i[:, 2]]
    r = np.asarray(rays, f32).astype(f64)
    o, d = r[:, 0:3], r[:, 3:6]
    e1, e2 = v0 - v1, v2 - v0
    ng = _cross(e2, e1)
    c = v0 - o
    rr = _cross(c, d)
    den = _dot(ng, d)
    s = np.sign(den)
    u = s * _dot(rr, e2) / np.abs(den)
    v = s * _dot(rr, e1) / np.abs(den)
    t = s * _dot(ng, c) / np.abs(den)
    bound = 16.0 * EPS * _norm(c) * _norm(d) * np.maximum(_norm(e1), _norm(e2)) / np.abs(den) + 4.0 * EPS
    point = (1.0 - u - v)[:, None] * v0 + u[:, None] * v1 + v[:, None] * v2
    gap = _norm(point - (o + t[:, None] * d))
    # in exact arithmetic the two points coincide; in float64 they differ by the float64 twin of the bound
    # above (u, v and t carry it) times the lengths they multiply, plus the roundings of the coordinates
    gap_bound = (64.0 * 2.0 ** -53 * _norm(c) * _norm(d) * np.maximum(_norm(e1), _norm(e2)) / np.abs(den)
                 * (_norm(e1) + _norm(e2) + _norm(d)) + 64.0 * 2.0 ** -53 * (_norm(o) + _norm(v0) + np.abs(t) * _norm(d)))
    return u, v, den, bound, gap / gap_bound


def _fma(a, b, c):
    """float32 fused multiply-add: the float64 product of two float32 values is exact."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _e_dot(a, b):
    return _fma(a[:, 0], b[:, 0], _fma(a[:, 1], b[:, 1], a[:, 2] * b[:, 2]))


def _e_cross(a, b):
    return np.stack([_fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), _fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])),
                     _fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], axis=1)


def emulated_uv(positions, indices, rays, tri):
    """(u, v) float32 in the kernel's operation order (tri_record, tri_hit4's U, V, den, IEEE division)."""
    p = np.asarray(positions, f32)
    i = np.asarray(indices, np.int64)[tri]
    v0, v1, v2 = p[i[:, 0]], p[i[:, 1]], p[i[:, 2]]
    r = np.asarray(rays, f32)
    o, d = r[:, 0:3], r[:, 3:6]
    e1, e2 = v0 - v1, v2 - v0
    ng = _e_cross(e2, e1)
    rr = _e_cross(v0 - o, d)
    den = _e_dot(ng, d)
    neg = np.signbit(den)
    aden = np.abs(den)
    uu, vv = _e_dot(rr, e2), _e_dot(rr, e1)
    return np.where(neg, -uu, uu) / aden, np.where(neg, -vv, vv) / aden


def check_barycentrics(u, v, positions, indices, rays, tri, what=""):
    """u, v: float32 barycentrics of the triangle hits (rays[k] hit triangle tri[k]).  Prints the worst ratio
    to the bound and asserts the module docstring's rules."""
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    u64, v64, den, bound, gap = reference_uv(positions, indices, rays, tri)
    err = np.maximum(np.abs(u.astype(f64) - u64), np.abs(v.astype(f64) - v64))
    ratio = float((err / bound).max()) if len(tri) else 0.0
    print(f"{what}: {len(tri)} triangle hits, worst |uv - uv64| / bound {ratio:.3f}, worst u + v - 1 "
          f"{float((u.astype(f64) + v.astype(f64) - 1.0).max()) if len(tri) else 0.0:.2e}, "
          f"worst distance of the two float64 hit points over its bound {float(gap.max()) if len(tri) else 0.0:.3f}")
    assert len(tri) > 0
    assert (den != 0.0).all()
    assert (u >= 0.0).all() and (u <= 1.0).all() and (v >= 0.0).all() and (v <= 1.0).all()
    assert (u.astype(f64) + v.astype(f64) <= 1.0 + 2.0 ** -22).all()
    assert (err <= bound).all()
    assert (gap <= 1.0).all()  # (1 - u - v) v0 + u v1 + v v2 = o + t d: the vertex convention
    return ratio
