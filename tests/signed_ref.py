"""Float64 reference of signed distance queries, written from the geometry: not from csrc/pseudonormal.h, no tree, no
device.

Welding: corners of live triangles (a stored float32 normal that is not exactly zero, adversarial_common.
stored_normals) are one vertex iff they belong to one geometry and their float32 positions compare equal in every
component (-0 == +0; a NaN equals nothing).  Pseudonormals (Baerentzen & Aanaes 2005): unit face normals
(b - a) x (c - a); N_v = sum over the vertex's corners of angle * n with the angle from math.atan2(|u x v|, u.v);
N_e = sum of n over the live triangles that share the unordered pair of welded vertices.  An edge is open with one
incidence, irregular unless it has exactly two that traverse it in opposite directions.

Inside / outside: the generalised winding number of one geometry's triangles (Van Oosterom & Strackee 1983: the solid
angle of a triangle from 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), summed, over 4 pi) and the
geometry's orientation (the sign of its signed volume sum a.(b x c) / 6: +1 when the normals point outward).  The
reference sign of a point whose nearest primitive (points_ref.nearest) is a triangle of geometry g is
orientation_g * (-1 if |w_g(p)| > 0.5 else +1); for a sphere it is negative iff |p - c| < r."""
import math

import numpy as np

import adversarial_common as A
import points_ref as PR


def tri_geoms(scene):
    first = scene["tri_geom_first"].astype(np.int64)
    nt = len(scene["indices"])
    return np.searchsorted(first, np.arange(nt), side="right") - 1 if nt else np.zeros(0, np.int64)


def live_mask(scene):
    return (A.stored_normals(scene) != 0.0).any(axis=1) if len(scene["indices"]) else np.zeros(0, bool)


def weld(scene):
    """(T, 3) int64 welded vertex id per corner (-1 for corners of triangles that are not live), and their number."""
    idx = scene["indices"].astype(np.int64)
    pos = scene["positions"]
    geom, live = tri_geoms(scene), live_mask(scene)
    ids = np.full((len(idx), 3), -1, np.int64)
    table = {}
    n = 0
    for t in range(len(idx)):
        if not live[t]:
            continue
        for k in range(3):
            x, y, z = (float(v) for v in pos[idx[t, k]])
            if x != x or y != y or z != z:  # a NaN equals nothing: a vertex of its own
                ids[t, k] = n
                n += 1
                continue
            key = (int(geom[t]), x + 0.0, y + 0.0, z + 0.0)  # (-0.0 + 0.0 is +0.0; the tuple compares by float equality)
            if key not in table:
                table[key] = n
                n += 1
            ids[t, k] = table[key]
    return ids, n


def pseudonormals(scene):
    """dict: nv, ne (T, 3, 3) float64 per corner k and edge k (0 = v0v1, 1 = v0v2, 2 = v1v2), zeros for triangles
    that are not live; welded_vertices, edges, open_edges, irregular_edges."""
    idx = scene["indices"].astype(np.int64)
    p = scene["positions"].astype(np.float64)[idx] if len(idx) else np.zeros((0, 3, 3))
    live = live_mask(scene)
    ids, nw = weld(scene)
    T = len(idx)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) if T else np.zeros((0, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        nhat = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    vsum = np.zeros((nw, 3))
    edges = {}
    pairs = ((0, 1), (0, 2), (1, 2))
    for t in range(T):
        if not live[t]:
            continue
        for k in range(3):
            o = [j for j in range(3) if j != k]
            u, v = p[t, o[0]] - p[t, k], p[t, o[1]] - p[t, k]
            ang = math.atan2(float(np.linalg.norm(np.cross(u, v))), float(np.dot(u, v)))
            if np.isfinite(nhat[t]).all():
                vsum[ids[t, k]] += ang * nhat[t]
        for k, (i, j) in enumerate(pairs):
            a, b = ids[t, i], ids[t, j]
            if a == b:
                continue
            e = edges.setdefault((min(a, b), max(a, b)), [np.zeros(3), 0, 0])
            if np.isfinite(nhat[t]).all():
                e[0] = e[0] + nhat[t]
            e[1 if (a < b) != (k == 1) else 2] += 1  # (the boundary runs edge 1 as v2 -> v0)
    nv, ne = np.zeros((T, 3, 3)), np.zeros((T, 3, 3))
    for t in range(T):
        if not live[t]:
            continue
        for k in range(3):
            nv[t, k] = vsum[ids[t, k]]
        for k, (i, j) in enumerate(pairs):
            a, b = ids[t, i], ids[t, j]
            if a != b:
                ne[t, k] = edges[(min(a, b), max(a, b))][0]
    return {"nv": nv, "ne": ne, "welded_vertices": nw, "edges": len(edges),
            "open_edges": sum(1 for e in edges.values() if e[1] + e[2] == 1),
            "irregular_edges": sum(1 for e in edges.values() if not (e[1] == 1 and e[2] == 1))}


def winding(scene, g, pts):
    """The generalised winding number of geometry g's triangles at pts (n, >= 3): float64 (n,)."""
    first = scene["tri_geom_first"].astype(np.int64)
    idx = scene["indices"].astype(np.int64)[first[g]:first[g + 1]]
    tri = scene["positions"].astype(np.float64)[idx]  # (T, 3, 3)
    q = np.asarray(pts, np.float64)[:, :3]
    w = np.zeros(len(q))
    for s in range(0, len(q), 256):
        a = tri[None, :, 0] - q[s:s + 256, None]
        b = tri[None, :, 1] - q[s:s + 256, None]
        c = tri[None, :, 2] - q[s:s + 256, None]
        la, lb, lc = (np.linalg.norm(v, axis=2) for v in (a, b, c))
        num = (a * np.cross(b, c)).sum(2)
        den = la * lb * lc + (a * b).sum(2) * lc + (b * c).sum(2) * la + (c * a).sum(2) * lb
        w[s:s + 256] = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * math.pi)
    return w


def orientation(scene, g):
    """+1 when geometry g's normals point outward (a positive signed volume), -1 inward, 0 for no volume."""
    first = scene["tri_geom_first"].astype(np.int64)
    tri = scene["positions"].astype(np.float64)[scene["indices"].astype(np.int64)[first[g]:first[g + 1]]]
    return float(np.sign((tri[:, 0] * np.cross(tri[:, 1], tri[:, 2])).sum()))


def reference_sign(scene, pts, near):
    """Per point the reference sign (+1, -1; 0 where the nearest primitive is a miss or its geometry has no
    orientation), given near = points_ref.nearest(scene, pts)."""
    ntg = len(scene["tri_geom_first"]) - 1
    q = np.asarray(pts, np.float64)[:, :3]
    out = np.zeros(len(q))
    geom = near["geom"].astype(np.int64)
    for g in np.unique(geom[near["geom"] != PR.MISS]):
        sel = np.flatnonzero(geom == g)
        if g < ntg:
            w = winding(scene, int(g), q[sel])
            out[sel] = orientation(scene, int(g)) * np.where(np.abs(w) > 0.5, -1.0, 1.0)
        else:
            s = scene["spheres"].astype(np.float64)[g - ntg]
            out[sel] = np.where(np.linalg.norm(q[sel] - s[:3], axis=1) < s[3], -1.0, 1.0)
    return out


def _closest_on_triangle(p, a, b, c):
    """(squared distance, q, feature) of the point of triangle abc nearest to p, float64: the best of the three clamped
    edge projections (feature 1, 2, 3 = ab, ac, bc inside the edge; 4, 5, 6 = a, b, c at an end) and, where it falls
    inside the triangle, the projection onto the plane (feature 0)."""
    best = None
    for k, (u, v, lo, hi) in enumerate(((a, b, 0, 1), (a, c, 0, 2), (b, c, 1, 2))):
        d = v - u
        den = float(np.dot(d, d))
        t = min(max(float(np.dot(p - u, d)) / den, 0.0), 1.0) if den > 0.0 else 0.0
        q = u + t * d
        cand = (float(np.dot(p - q, p - q)), q, 4 + lo if t == 0.0 else 4 + hi if t == 1.0 else 1 + k)
        if best is None or cand[0] < best[0]:
            best = cand
    ab, ac, ap = b - a, c - a, p - a
    n = np.cross(ab, ac)
    nn = float(np.dot(n, n))
    if nn > 0.0:
        d00, d01, d11, d20, d21 = np.dot(ab, ab), np.dot(ab, ac), np.dot(ac, ac), np.dot(ap, ab), np.dot(ap, ac)
        v, w = (d11 * d20 - d01 * d21) / nn, (d00 * d21 - d01 * d20) / nn
        if v >= 0.0 and w >= 0.0 and v + w <= 1.0:
            q = a + v * ab + w * ac
            d2 = float(np.dot(p - q, p - q))
            if d2 < best[0]:
                best = (d2, q, 0)
    return best


def reference_cos(scene, pts, near, tables):
    """Per point |cos(p - q, N)| in float64 with nothing from the library: q and the feature it lies on are the nearest
    point of the primitive near = points_ref.nearest(scene, pts) names, N the face normal or the float64 pseudonormal
    of that feature (tables = pseudonormals(scene)).  1 for a sphere (p - q is radial); 0 where it is not defined (a
    vanishing p - q or N, a non-finite point, a miss)."""
    ntg = len(scene["tri_geom_first"]) - 1
    first = scene["tri_geom_first"].astype(np.int64)
    idx = scene["indices"].astype(np.int64)
    pos = scene["positions"].astype(np.float64)
    q64 = np.asarray(pts, np.float64)[:, :3]
    out = np.zeros(len(q64))
    for i in range(len(q64)):
        g = int(near["geom"][i])
        if near["geom"][i] == PR.MISS or not np.isfinite(q64[i]).all():
            continue
        if g >= ntg:
            out[i] = 1.0
            continue
        t = int(first[g]) + int(near["prim"][i])
        a, b, c = pos[idx[t]]
        _, q, f = _closest_on_triangle(q64[i], a, b, c)
        N = np.cross(b - a, c - a) if f == 0 else tables["ne"][t, f - 1] if f < 4 else tables["nv"][t, f - 4]
        d = q64[i] - q
        den = float(np.linalg.norm(d) * np.linalg.norm(N))
        if den > 0.0 and np.isfinite(den):
            out[i] = abs(float(np.dot(d, N))) / den
    return out


def other_geom_distance(scene, pts, geom):
    """Per point the distance (float64) to the nearest live primitive whose geomID differs from geom[i]; +inf if none."""
    ntg = len(scene["tri_geom_first"]) - 1
    q = np.asarray(pts, np.float64)[:, :3]
    idx = scene["indices"].astype(np.int64)
    pos = scene["positions"].astype(np.float64)
    tg, live = tri_geoms(scene), live_mask(scene)
    sph = scene["spheres"].astype(np.float64)
    best = np.full((len(q), ntg + len(sph)), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(ntg):
            tri = np.flatnonzero(live & (tg == g))
            if len(tri) == 0:
                continue
            for s in range(0, len(q), PR.CHUNK):
                d = PR.tri_distances(q[s:s + PR.CHUNK], pos[idx[tri, 0]], pos[idx[tri, 1]], pos[idx[tri, 2]])
                best[s:s + PR.CHUNK, g] = np.where(np.isnan(d), np.inf, d).min(axis=1)
        for j in range(len(sph)):
            d = np.abs(np.linalg.norm(q - sph[j, :3], axis=1) - sph[j, 3])
            best[:, ntg + j] = np.where(np.isnan(d), np.inf, d)
    own = np.asarray(geom, np.int64)
    ok = (own >= 0) & (own < best.shape[1])
    best[np.flatnonzero(ok), own[ok]] = np.inf
    return best.min(axis=1) if best.shape[1] else np.full(len(q), np.inf)
