"""Float64 reference of closest-point queries, written from the geometry: no tree, no device, not the library's
arithmetic.  The distance from a point to a triangle is the smallest of the distances to its three edge segments
(clamped projections) and, where the orthogonal projection onto the triangle's plane falls inside the triangle
(its weights from the normal equations), the distance to the plane.  The distance to a sphere is | |p - c| - r |.

A triangle the build leaves out of the tree (a stored float32 normal of exactly zero, adversarial_common.
stored_normals) takes no part.  nearest() returns, per point, the best distance with its (geom, prim), the
runner-up distance over the other primitives, and the best triangle's smallest height (0 for a sphere)."""
import numpy as np

import adversarial_common as A

MISS = 0xFFFFFFFF
CHUNK = 128


def _seg(p, a, b):
    """(P, T) distances from points p (P, 1, 3) to segments a -> b (1, T, 3)."""
    ab = b - a
    den = (ab * ab).sum(-1)
    t = ((p - a) * ab).sum(-1) / np.where(den > 0.0, den, 1.0)
    t = np.where(den > 0.0, np.clip(t, 0.0, 1.0), 0.0)
    d = p - (a + t[..., None] * ab)
    return np.sqrt((d * d).sum(-1))


def tri_distances(p, a, b, c):
    """(P, T) float64 distances from points (P, 3) to triangles a, b, c (T, 3)."""
    p = p[:, None, :]
    a, b, c = a[None], b[None], c[None]
    d = np.minimum(np.minimum(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a))
    ab, ac, ap = b - a, c - a, p - a
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    ok = nn > 0.0
    # the projection's weights from the normal equations (nn is their determinant: Lagrange's identity)
    d00, d01, d11 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1)
    d20, d21 = (ap * ab).sum(-1), (ap * ac).sum(-1)
    den = np.where(ok, nn, 1.0)
    v = (d11 * d20 - d01 * d21) / den
    w = (d00 * d21 - d01 * d20) / den
    inside = ok & (v >= 0.0) & (w >= 0.0) & (v + w <= 1.0)
    h = (ap * n).sum(-1) / den  # signed height in units of |n|
    return np.where(inside, np.minimum(d, np.abs(h) * np.sqrt(nn)), d)


def smallest_heights(scene):
    """Per triangle: twice the area over the longest edge, float64."""
    p = scene["positions"].astype(np.float64)[scene["indices"].astype(np.int64)]
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    longest = np.maximum(np.maximum(np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1)), np.linalg.norm(a - c, axis=1))
    return area2 / np.where(longest > 0.0, longest, 1.0)


def nearest(scene, points):
    """dict: dist, second (float64; +inf where there is none), geom, prim (uint32; MISS where the scene holds no
    live primitive), height (float64) for points (n, >= 3)."""
    pts = np.asarray(points, np.float64)[:, :3]
    n = len(pts)
    idx = scene["indices"].astype(np.int64)
    pos = scene["positions"].astype(np.float64)
    first = scene["tri_geom_first"].astype(np.int64)
    ntg = len(first) - 1
    live = (A.stored_normals(scene) != 0.0).any(axis=1) if len(idx) else np.zeros(0, bool)
    tri = np.flatnonzero(live)
    a, b, c = pos[idx[tri, 0]], pos[idx[tri, 1]], pos[idx[tri, 2]]
    geom_t = np.searchsorted(first, tri, side="right") - 1 if len(tri) else np.zeros(0, np.int64)
    prim_t = tri - first[geom_t] if len(tri) else np.zeros(0, np.int64)
    sph = scene["spheres"].astype(np.float64)
    geom = np.concatenate([geom_t, ntg + np.arange(len(sph))]).astype(np.int64)
    prim = np.concatenate([prim_t, np.zeros(len(sph), np.int64)])
    height = np.concatenate([smallest_heights(scene)[tri] if len(tri) else np.zeros(0), np.zeros(len(sph))])
    out = {"dist": np.full(n, np.inf), "second": np.full(n, np.inf), "geom": np.full(n, MISS, np.uint32),
           "prim": np.full(n, MISS, np.uint32), "height": np.zeros(n)}
    if len(geom) == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, n, CHUNK):
            p = pts[s:s + CHUNK]
            parts = []
            if len(tri):
                parts.append(tri_distances(p, a, b, c))
            if len(sph):
                parts.append(np.abs(np.linalg.norm(p[:, None, :] - sph[None, :, :3], axis=2) - sph[None, :, 3]))
            d = np.concatenate(parts, axis=1)
            d = np.where(np.isnan(d), np.inf, d)
            k = np.argmin(d, axis=1)
            rows = np.arange(len(p))
            out["dist"][s:s + CHUNK] = d[rows, k]
            out["geom"][s:s + CHUNK] = geom[k]
            out["prim"][s:s + CHUNK] = prim[k]
            out["height"][s:s + CHUNK] = height[k]
            if d.shape[1] > 1:
                d[rows, k] = np.inf
                out["second"][s:s + CHUNK] = d.min(axis=1)
    return out
