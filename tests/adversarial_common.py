"""Shared inputs of the adversarial-geometry tests (test_adversarial_cpu.py, test_gpu_adversarial.py): scene
and ray generators for the branches of the BVH build and of the traversals that well-conditioned scenes never
reach, and the rule by which a result is compared with the CPU oracle's brute force
(oracle.Prepared(scene, bvh=False): every primitive tested against every ray in the reference's float32
arithmetic, no tree of any kind).

Everything is deterministic: default_rng with fixed seeds, float64 arithmetic cast to float32, arrays
read-only.  A family is a list of cases (name, flat scene, rays (n, 8) float32 o3 d3 tnear tfar).

Rays used by most families, for a scene with box centre c and half diagonal R (a unit box when empty):
  grid_rays  64 x 64 pixel-centre rays of a pinhole at c + 4 R (0.3, 0.5, 1) / |.| looking at c, the image
             plane spanning 2.2 R;
  box_rays   n rays from default_rng(seed): origins uniform in the box scaled by 3 about c, aimed at targets
             uniform in the box scaled by 1.2.

Families (the smallest sizes at which the named branch is still reached):
  tiny       0, 1, 2, 3, 4, 5, 8, 9, 16, 17 primitives from default_rng(100 + n), as triangles only, spheres
             only (num_verts == 0, no triangle geometry) and mixed (n // 2 triangles, the rest spheres): the
             NP == 0 upload, the N == 1 and N <= leaf_max leaf roots, wide nodes with fewer than 4 children,
             the N >= 3 treelet gate.  grid_rays + box_rays(4096).
  equal      key ties: K coincident triangles, K identical spheres, K concentric spheres of radius
             (64 + i) / 256, K in 2, 17, 64, 65, 300 (delta()'s 64 + clz(i ^ j)); an 8 x 8-cell planar
             grid at z = 0 (zero centroid extent in one axis); 24 primitives whose box centres are
             (i / 4, 0, 0) (two axes); a fan of 40 triangles whose box centres are all exactly 0 (three).
  degenerate exactly degenerate triangles (stored normal exactly 0: a repeated index (i, i, j) or (i, j, i),
             or v0 and v1 / v0 and v2 at one position under distinct indices) mixed into default_emitter,
             alone with one sphere, and alone: excluded_prims must equal their number (7) in the first two.
             A fourth case adds a triangle (i, j, j) and two collinear ones with distinct vertices: their
             normal cross(e2, e1) is a rounding residue, not always 0, so no count is asserted there.
  axis       a 6 x 6-cell grid at z = 0 under rays d = (0, 0, -1) and (0, 0, 1) through every vertex, edge
             midpoint and cell centre (the half-integer lattice), and in-plane rays d = (1, 0, 0), once with
             +0.0 and once with -0.0 in the zero components; the closed box [0, 1]^3 of 2 x 2 quads per face
             under rays running inside its face planes and rays starting on a face plane.
  scale      default_emitter and refit_common's rays with positions, spheres and origins times 2^-30 and
             2^30 (exact), next to the unscaled case.
  offset     the same translated by 2^10, 2^16 and 2^20 along (1, 1, 1) (float64 sum, cast to float32).
  deep       see deep_tree(): a chain of 63 levels, and one of 30 (deep_short).
  staging    T small triangles from default_rng(800) in [-2, 2]^3, every 16th a long sliver across the axes
             (what split references split), for T one below, at and one above the largest count the byte
             estimate of build_lbvh stages into LDS; and the same with 8 exactly degenerate triangles added,
             around the count where the estimate over NP (all uploaded) and over N (without them) disagree.
  interval   default_emitter; 300 of refit_common's rays with an oracle hit at t0, each with tfar and tnear
             in {nextafter(t0, 0), t0, nextafter(t0, inf)}, tfar < tnear, tfar == 0, d = (0, 0, 0), and the
             direction times 2^-10 and 2^10; plus rays (x, 1.75 + h, z) + t (0, -1, 0) whose hit distance on the
             cube's top face y = 1.75 is exactly the dyadic h, for which the ends of (tnear, tfar] are exact.
  indexing   four triangle geometries of 5, 0, 7, 0 triangles over vertices of which every third is unused,
             then 3 spheres; geometry g has material g.
  spheres    8 spheres and one of radius 0: origins inside, origins at the float32 point nearest the surface,
             axis-parallel and random tangent rays, rays through the zero-radius sphere's centre.  And five
             zero-radius spheres at (k, 2, 3), three at (1, 2, 3): axis-parallel rays through every centre along
             +-x, +-y, +-z from 3 away (with +0.0 and with -0.0), which hit exactly (disc = 0) at t = 3 or
             nearer, and the same rays moved half a unit aside, which miss.

Comparison rule (compare): t bit-equal for every ray, misses (+inf) included; occluded equal for every ray
(both are a minimum / an existence over the same primitives and cannot depend on the order of traversal).
Where (geomID, primID) equal the oracle's, Ng is bit-equal; where they differ, t is still bit-equal and the
named primitive is really hit at that t (the oracle on a scene of that one primitive).  A t or occluded
mismatch is excused only when a float64 recomputation puts the hit (the reference's, or the device's where
the reference misses) within query_common's error bound of a triangle edge, or within the analogous bound of
a sphere's tangent (|disc| <= 16 * 2^-24 * (b^2 + 4 |a c|)); at most refit_common.CAP of a case's rays may
be excused.  The expected number is zero."""
import functools
import os
import re

import numpy as np

import oracle
import query_common as Q
import refit_common as R

f32, f64 = np.float32, np.float64
MISS = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17)
TIE_KS = (2, 17, 64, 65, 300)
FAMILIES = ("tiny", "equal", "degenerate", "axis", "scale", "offset", "deep", "staging", "interval", "indexing",
            "spheres")


def header_constant(name: str) -> int:
    """An integer constant of csrc/sptr_internal.h (kStack, kLdsSceneBytes), evaluated from its text."""
    text = open(os.path.join(ROOT, "simple-path-tracer_amd", "csrc", "sptr_internal.h")).read()
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9* ]+);", text)
    assert m, name
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f)
    return v


class Case:
    def __init__(self, name, scene, rays, ndeg=0, unsure=0, all_deg=False, **meta):
        self.name, self.scene, self.rays = name, scene, rays
        self.ndeg = ndeg          # exactly degenerate triangles by construction (None: not known)
        self.unsure = unsure      # further triangles whose stored normal may or may not be exactly 0
        self.all_deg = all_deg    # every primitive is an exactly degenerate triangle
        self.meta = meta

    @property
    def num_tris(self):
        return len(self.scene["indices"])

    @property
    def num_spheres(self):
        return len(self.scene["spheres"])


def make_scene(positions, indices, spheres, first=None, materials=None) -> dict:
    p = np.asarray(positions, f64).reshape(-1, 3).astype(f32)
    i = np.asarray(indices, np.int64).reshape(-1, 3).astype(np.uint32)
    s = np.asarray(spheres, f64).reshape(-1, 4).astype(f32)
    if first is None:
        first = [0, len(i)] if len(i) else [0]
    g = np.asarray(first, np.uint32)
    m = np.arange(len(g) - 1 + len(s), dtype=np.uint32) % 6 if materials is None else np.asarray(materials, np.uint32)
    out = {"positions": p, "indices": i, "tri_geom_first": g, "spheres": s, "geom_material": m}
    for a in out.values():
        a.setflags(write=False)
    return out


def transformed(scene, positions=None, spheres=None) -> dict:
    out = dict(scene)
    if positions is not None:
        out["positions"] = np.ascontiguousarray(positions, f32)
    if spheres is not None:
        out["spheres"] = np.ascontiguousarray(spheres, f32)
    for a in out.values():
        a.setflags(write=False)
    return out


def bounds(scene):
    """(centre, half diagonal, lower corner, upper corner) of the referenced vertices and the spheres, float64;
    a unit box when empty; a flat box is given a thickness."""
    p = scene["positions"].astype(f64)[np.unique(scene["indices"].astype(np.int64))] if len(scene["indices"]) else np.zeros((0, 3))
    s = scene["spheres"].astype(f64)
    lo = np.concatenate([p, s[:, :3] - s[:, 3:4]], axis=0)
    hi = np.concatenate([p, s[:, :3] + s[:, 3:4]], axis=0)
    if len(lo) == 0:
        return np.zeros(3), np.sqrt(3.0) / 2.0, np.full(3, -0.5), np.full(3, 0.5)
    lo, hi = lo.min(axis=0), hi.max(axis=0)
    half = np.maximum(0.5 * (hi - lo), 1e-3 * max(1e-30, float(np.abs(hi - lo).max())))
    half = np.where(half > 0.0, half, 0.5)
    c = 0.5 * (lo + hi)
    return c, float(np.linalg.norm(half)), c - half, c + half


def _rays(o, d, tnear=0.0, tfar=np.inf):
    r = np.zeros((len(o), 8), f32)
    r[:, 0:3] = o
    r[:, 3:6] = d
    r[:, 6] = tnear
    r[:, 7] = tfar
    return r


def grid_rays(scene, n=64):
    c, rad, _, _ = bounds(scene)
    eye = c + 4.0 * rad * np.array([0.3, 0.5, 1.0]) / np.linalg.norm([0.3, 0.5, 1.0])
    fw = (c - eye) / np.linalg.norm(c - eye)
    ex = np.cross(fw, [0.0, 1.0, 0.0])
    ex /= np.linalg.norm(ex)
    ey = np.cross(ex, fw)
    u = ((np.arange(n) + 0.5) / n - 0.5) * 2.2 * rad
    tg = c + u[None, :, None] * ex + u[:, None, None] * ey
    d = (tg - eye).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _rays(np.broadcast_to(eye, d.shape), d)


def box_rays(scene, n, seed):
    c, _, lo, hi = bounds(scene)
    rng = np.random.default_rng(seed)
    o = rng.uniform(c + 3.0 * (lo - c), c + 3.0 * (hi - c), (n, 3))
    tg = rng.uniform(c + 1.2 * (lo - c), c + 1.2 * (hi - c), (n, 3))
    d = tg - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _rays(o, d)


def _finish(rays):
    rays = np.ascontiguousarray(rays, f32)
    rays.setflags(write=False)
    return rays


def standard_rays(scene, n, seed):
    return _finish(np.concatenate([grid_rays(scene), box_rays(scene, n, seed)], axis=0))


# ----------------------------------------------------------------------------------------------- tiny
def _random_tris(rng, n, spread=1.0, size=0.5):
    c = rng.uniform(-spread, spread, (n, 1, 3))
    return (c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3), np.arange(3 * n).reshape(n, 3)


def _random_spheres(rng, n, spread=1.0):
    return np.concatenate([rng.uniform(-spread, spread, (n, 3)), rng.uniform(0.2, 0.5, (n, 1))], axis=1)


def tiny():
    out = []
    for n in COUNTS:
        for kind in ("tri", "sph", "mix"):
            rng = np.random.default_rng(100 + n)
            nt = {"tri": n, "sph": 0, "mix": n // 2}[kind]
            pos, idx = _random_tris(rng, nt)
            if kind == "mix" and nt == 0:
                pos = rng.uniform(-1.0, 1.0, (3, 3))  # vertices, but no triangle
            sc = make_scene(pos, idx, _random_spheres(rng, n - nt))
            out.append(Case(f"tiny_{kind}{n}", sc, standard_rays(sc, 4096, 200 + n)))
    return out


# ---------------------------------------------------------------------------------------------- equal
def _centred_tri(c, a, b, d):
    """A triangle whose box is c -+ (a, b, d): the box centre is exactly c for dyadic entries."""
    c = np.asarray(c, f64)
    return np.array([c + [-a, -b, -d], c + [a, b, -d], c + [a, -b, d]])


def planar_grid(n):
    """n x n unit cells at z = 0, two triangles each; vertex (i, j) is index j * (n + 1) + i."""
    g = np.arange(n + 1, dtype=f64)
    pos = np.stack([np.tile(g, n + 1), np.repeat(g, n + 1), np.zeros((n + 1) ** 2)], axis=1)
    idx = []
    for j in range(n):
        for i in range(n):
            v = j * (n + 1) + i
            idx += [[v, v + 1, v + n + 2], [v, v + n + 2, v + n + 1]]
    return make_scene(pos, idx, np.zeros((0, 4)))


def equal():
    out = []
    tri = np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, -0.2], [0.0, 0.7, 0.3]])
    for k in TIE_KS:
        sc = make_scene(np.tile(tri, (k, 1)), np.arange(3 * k).reshape(k, 3), np.zeros((0, 4)))
        out.append(Case(f"equal_tris{k}", sc, standard_rays(sc, 2048, 300 + k)))
        sc = make_scene(np.zeros((0, 3)), np.zeros((0, 3)), np.tile([0.25, -0.5, 0.125, 0.75], (k, 1)))
        out.append(Case(f"equal_spheres{k}", sc, standard_rays(sc, 2048, 400 + k)))
        rad = (64.0 + np.arange(k)) / 256.0  # dyadic, as the centre: c -+ r and their mean are exact
        sc = make_scene(np.zeros((0, 3)), np.zeros((0, 3)),
                        np.concatenate([np.tile([0.25, -0.5, 0.125], (k, 1)), rad[:, None]], axis=1))
        out.append(Case(f"equal_concentric{k}", sc, standard_rays(sc, 2048, 500 + k)))
    sc = planar_grid(8)
    out.append(Case("equal_flat1", sc, standard_rays(sc, 4096, 601)))
    rng = np.random.default_rng(602)
    pos, sph = [], []
    for i in range(24):
        if i % 4 == 3:
            sph.append([i / 4.0, 0.0, 0.0, 0.1 + 0.05 * (i % 3)])
        else:
            a, b, d = rng.integers(1, 9, 3) / 64.0
            pos.append(_centred_tri([i / 4.0, 0.0, 0.0], a, b, d))
    pos = np.concatenate(pos)
    sc = make_scene(pos, np.arange(len(pos)).reshape(-1, 3), sph)
    out.append(Case("equal_flat2", sc, standard_rays(sc, 4096, 603)))
    pos = []
    for i in range(40):
        a, b, d = rng.integers(1, 33, 3) / 64.0
        sg = [1 - 2 * ((i >> k) & 1) for k in range(3)]
        pos.append(_centred_tri([0.0, 0.0, 0.0], a, b, d) * sg)
    pos = np.concatenate(pos)
    sc = make_scene(pos, np.arange(len(pos)).reshape(-1, 3), np.zeros((0, 4)))
    out.append(Case("equal_flat3", sc, standard_rays(sc, 4096, 604)))
    return out


def box_centres(scene):
    """The float32 box centres 0.5f * (lo + hi) of every primitive, as k_ref_bounds / k_morton form them."""
    p = scene["positions"][scene["indices"].astype(np.int64)] if len(scene["indices"]) else np.zeros((0, 3, 3), f32)
    lo, hi = p.min(axis=1), p.max(axis=1)
    s = scene["spheres"]
    lo = np.concatenate([lo, s[:, :3] - s[:, 3:4]], axis=0).astype(f32)
    hi = np.concatenate([hi, s[:, :3] + s[:, 3:4]], axis=0).astype(f32)
    return f32(0.5) * (lo + hi)


def morton_keys(scene):
    """k_morton's 63-bit keys in numpy (float32 arithmetic), without the degenerate bit."""
    c = box_centres(scene)
    lo = c.min(axis=0)
    ext = (c.max(axis=0) - lo).astype(f32)
    keys = np.zeros(len(c), np.uint64)
    for k in range(3):
        t = ((c[:, k] - lo[k]) / ext[k]).astype(f32) if ext[k] > 0 else np.full(len(c), 0.5, f32)
        q = np.minimum(np.maximum(t * f32(2097152.0), f32(0.0)), f32(2097151.0)).astype(np.uint64)
        for b in range(21):
            keys |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - k)
    return keys


# ----------------------------------------------------------------------------------------- degenerate
def _mixed():
    return transformed(oracle.builtin_scene("default_emitter"))


def _mixed_rays():
    return R.rays(oracle.camera(aspect=R.W / R.H))


def _degenerates(nv):
    """Vertices (appended after nv existing ones) and index triples: 7 exactly degenerate triangles, then 3
    whose stored normal is a rounding residue ((i, j, j) and two collinear ones)."""
    v = np.array([[0.3, 0.9, 0.2], [-0.8, 1.4, 0.6], [1.1, 0.4, -0.7], [0.3, 0.9, 0.2], [1.1, 0.4, -0.7],
                  [0.1, 0.2, 0.3], [0.3, 0.5, 0.7], [0.7, 1.1, 1.5], [0.2, 0.4, 0.6]])
    i = np.array([[0, 0, 1], [1, 2, 1], [2, 2, 2], [0, 3, 1], [3, 0, 2], [2, 1, 4], [4, 2, 0],
                  [0, 1, 1], [5, 6, 7], [5, 8, 6]]) + nv
    return v, i, 7, 3


def degenerate():
    base = _mixed()
    nv = len(base["positions"])
    v, i, nd, nu = _degenerates(nv)
    first = base["tri_geom_first"].copy()
    first[-1] += len(i)  # the last triangle geometry takes them
    sc = make_scene(np.concatenate([base["positions"], v]), np.concatenate([base["indices"], i]), base["spheres"], first,
                    base["geom_material"])
    residue = Case("degenerate_residue", sc, _mixed_rays(), ndeg=None)  # (no count: see the module docstring)
    first = base["tri_geom_first"].copy()
    first[-1] += nd
    sc = make_scene(np.concatenate([base["positions"], v]), np.concatenate([base["indices"], i[:nd]]), base["spheres"],
                    first, base["geom_material"])
    out = [Case("degenerate_mixed", sc, _mixed_rays(), ndeg=nd)]
    v, i, nd, nu = _degenerates(0)
    sc = make_scene(v, i[:nd], [[0.2, 0.8, 0.1, 0.6]])
    out.append(Case("degenerate_sphere", sc, standard_rays(sc, 4096, 701), ndeg=nd))
    sc = make_scene(v, i[:nd], np.zeros((0, 4)))
    out.append(Case("degenerate_alone", sc, standard_rays(sc, 4096, 702), ndeg=nd, all_deg=True))
    out.append(residue)
    return out


def stored_normals(scene):
    """Ng = cross(e2, e1), e1 = v0 - v1, e2 = v2 - v0, with the fused form the records store (float32)."""
    p = scene["positions"][scene["indices"].astype(np.int64)]
    return Q._e_cross(p[:, 2] - p[:, 0], p[:, 0] - p[:, 1])


# ----------------------------------------------------------------------------------------------- axis
def _signed_zero(rays, negative):
    r = rays.copy()
    if negative:
        d = r[:, 3:6]
        d[d == 0.0] = -0.0
    return r


def axis():
    out = []
    grid = planar_grid(6)
    h = np.arange(13) / 2.0
    x, y = np.meshgrid(h, h)
    pts = np.stack([x.ravel(), y.ravel()], axis=1)
    n = len(pts)
    down = _rays(np.concatenate([pts, np.full((n, 1), 3.0)], axis=1), np.tile([0.0, 0.0, -1.0], (n, 1)))
    up = _rays(np.concatenate([pts, np.full((n, 1), -2.0)], axis=1), np.tile([0.0, 0.0, 1.0], (n, 1)))
    inpl = _rays(np.stack([np.full(13, -1.0), h, np.zeros(13)], axis=1), np.tile([1.0, 0.0, 0.0], (13, 1)))
    off = _rays(np.stack([np.full(13, -1.0), h, np.full(13, 0.5)], axis=1), np.tile([1.0, 0.0, 0.0], (13, 1)))
    rr = np.concatenate([down, up, inpl, off, box_rays(grid, 1024, 801)], axis=0)
    # the closed box [0, 1]^3, 2 x 2 quads per face
    pos, idx = [], []
    for ax in range(3):
        for side in (0.0, 1.0):
            u, v = [a for a in range(3) if a != ax]
            base = len(pos)
            for j in range(3):
                for i in range(3):
                    q = np.zeros(3)
                    q[ax], q[u], q[v] = side, i / 2.0, j / 2.0
                    pos.append(q)
            for j in range(2):
                for i in range(2):
                    a = base + j * 3 + i
                    idx += [[a, a + 1, a + 4], [a, a + 4, a + 3]]
    box = make_scene(pos, idx, np.zeros((0, 4)))
    o, d = [], []
    for ax in range(3):
        u, v = [a for a in range(3) if a != ax]
        for side in (0.0, 1.0):
            for c in (0.0, 0.25, 0.5, 1.0):
                # inside the face plane x_ax = side, along u at height v = c, from outside and from inside
                for start in (-1.0, 0.25):
                    q, e = np.zeros(3), np.zeros(3)
                    q[ax], q[u], q[v] = side, start, c
                    e[u] = 1.0
                    o.append(q)
                    d.append(e)
            for c in ((0.25, 0.25), (0.5, 0.5), (0.3, 0.8), (1.0, 0.5), (0.0, 0.0)):
                # starting on the face plane: along the normal both ways, and obliquely inwards
                for e in ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.5, 0.3, 0.2) if side == 0.0 else (-0.5, 0.3, 0.2)):
                    q, w = np.zeros(3), np.zeros(3)
                    q[ax], q[u], q[v] = side, c[0], c[1]
                    w[ax], w[u], w[v] = e
                    o.append(q)
                    d.append(w / np.linalg.norm(w))
    br = np.concatenate([_rays(np.array(o), np.array(d)), box_rays(box, 1024, 802)], axis=0)
    for neg in (False, True):
        tag = "neg" if neg else "pos"
        out.append(Case(f"axis_grid_{tag}", grid, _finish(_signed_zero(rr, neg)), lattice=2 * n))
        out.append(Case(f"axis_box_{tag}", box, _finish(_signed_zero(br, neg))))
    return out


# ------------------------------------------------------------------------------------- scale / offset
def scale():
    base, rays = _mixed(), _mixed_rays()
    out = []
    for k in (0, -30, 30):
        f = f32(2.0) ** f32(k)
        rr = rays.copy()
        rr[:, 0:3] *= f
        sc = transformed(base, base["positions"] * f, base["spheres"] * f)
        out.append(Case(f"scale_{k}", sc, _finish(rr), k=k))
    return out


def offset():
    base, rays = _mixed(), _mixed_rays()
    out = []
    for k in (10, 16, 20):
        t = 2.0 ** k
        rr = rays.copy()
        rr[:, 0:3] = (rays[:, 0:3].astype(f64) + t).astype(f32)
        sph = base["spheres"].astype(f64)
        sph[:, :3] += t
        sc = transformed(base, (base["positions"].astype(f64) + t).astype(f32), sph.astype(f32))
        out.append(Case(f"offset_{k}", sc, _finish(rr), ndeg=None))  # (snapping to the coarse grid may flatten triangles)
    return out


# ----------------------------------------------------------------------------------------------- deep
DEEP_LEVELS = 21   # b = 0 .. 20: all 63 bits of the key
DEEP_RING = 17     # ring triangles per cluster; with the spar 18, more than the largest leaf (16)
DEEP_CLUSTER = DEEP_RING + 1
DEEP_SPAR = 0.04   # a spar's distance from the axis, in units of |x(s_j)|
DEEP_W = np.array([1.0, 1.2, 1.5])
DEEP_S = (0.58, 0.46, 0.375)  # position of cluster (b, a) along the axis, times 2^-b


def deep_tree(levels=DEEP_LEVELS, name="deep"):
    """(deep_short is the same construction with b = 0 .. 9: 30 clusters, a chain short enough for the BVH4
    stack bound, so that the wide walks' stacks spill as well.)
    A tree whose depth comes from geometry, not from primitive count.  The scene lies in [0, 1]^3 (an
    anchor triangle with box centre exactly 0 and one with box centre exactly (1, 1, 1) fix the Morton grid),
    around the axis x(s) = s (1, 1.2, 1.5), 0 < s < 1 — the space diagonal of the 1 x 1.2 x 1.5 box.  With
    the Morton bits taken from the top (x, y, z of level b = 0, then of b = 1, ...), cluster j = 3 b + a sits
    at s_j = (0.58, 0.46, 0.375)[a] * 2^-b: there every more significant bit is 0 and bit j is 1 (for a = 1:
    x = 0.46 < 1/2 <= 0.552 = y, in units of 2^-b, and so on), so the sorted keys split off cluster 0 at the
    root, cluster 1 below it, ...: a chain of 63 levels, both children internal (each cluster has 18
    triangles, more than the largest leaf), at a spacing of 2^-1/3 per level on average, 2^-1 per three.
    Cluster j is a ring of 17 triangles of circumradius 0.0001 |x(s_j)| in the plane through x(s_j)
    perpendicular to the axis, at distance theta_j |x(s_j)| from it, theta_j = 0.008 (1 + 0.04 j), at angles
    2 pi i / 17 + 0.37 j: every centroid stays inside the cluster's Morton cell, the ring's box contains
    x(s_j), and the axis touches no triangle.  Seen from the origin the rings have distinct angular radii
    theta_j, 0.00032 apart, against a triangle's 0.0001: a ray from the origin through a triangle of ring j
    passes between the triangles of every other ring.
    Each cluster also holds one spar, its 18th triangle: a sliver along the other diagonal of the box
    x(s_j) -+ 1.1 x(s_j), from x + 1.1 (x_0, -x_1, -x_2) to x + 1.1 (-x_0, x_1, x_2), moved 0.04 |x(s_j)| off the
    axis along (0, 1.5, -1.2) / |.| (perpendicular to both), 0.003 |x(s_j)| wide.  Its box centre stays in the
    cluster's cell and its box contains every smaller cluster: the spars' boxes are nested, so the chain is
    also what a surface-area heuristic prefers (a node costs the area of its largest member, and the chain
    charges every member once), and the treelet passes of the single-primitive-leaf builds leave it deep;
    without the spars they regroup the thin rings and the depth falls from 68 to 25.  Seen from the origin a
    spar stays 0.04 from the axis or more, beyond the largest ring (0.028).

    Rays: the axis ray from the origin (the small end); for every cluster j, rays from the origin through
    the centroids of its triangles 0, 1, 2, and the same lines shot back from twice the distance (tfar ends
    them before the origin).  A
    nearest-first walk from the small end descends the chain pushing the far child (cluster 0, 1, ...), so
    the hit in cluster j is found after that entry, at stack slot ~j, is popped: beyond the 12 LDS entries
    for j >= 12.  Then grid_rays and box_rays(2048)."""
    w = DEEP_W
    wl = np.linalg.norm(w)
    n1 = np.cross(w, [0.0, 0.0, 1.0])
    n1 /= np.linalg.norm(n1)
    n2 = np.cross(w, n1) / wl
    spar_off = np.array([0.0, w[2], -w[1]]) / np.hypot(w[1], w[2])  # perpendicular to the axis and to a spar
    pos = []
    e = 2.0 ** -24
    anchor = np.array([[-e, -e, -e], [e, e, -e], [e, -e, e]])
    pos += [anchor, 1.0 + anchor * 2.0 ** 14]
    targets = []
    for j in range(3 * levels):
        b, a = divmod(j, 3)
        s = DEEP_S[a] * 2.0 ** -b
        dist = s * wl
        for i in range(DEEP_RING):
            phi = 2.0 * np.pi * i / DEEP_RING + 0.37 * j
            c = s * w + dist * 0.008 * (1.0 + 0.04 * j) * (np.cos(phi) * n1 + np.sin(phi) * n2)
            psi = phi + 2.0 * np.pi * np.arange(3)[:, None] / 3.0
            tri = c + dist * 0.0001 * (np.cos(psi) * n1 + np.sin(psi) * n2)
            pos.append(tri)
            if i < 3:
                targets.append(c)
        # the cluster's spar: end to end across the box x(s_j) -+ 1.1 x(s_j), moved off the axis by DEEP_SPAR
        x = s * w
        mid = x + DEEP_SPAR * dist * spar_off
        pos.append(np.array([mid + 1.1 * x * [1.0, -1.0, -1.0], mid + 1.1 * x * [-1.0, 1.0, 1.0],
                             mid + 0.003 * dist * spar_off]))
    pos = np.concatenate(pos)
    sc = make_scene(pos, np.arange(len(pos)).reshape(-1, 3), np.zeros((0, 4)))
    tg = np.array(targets)
    d = tg / np.linalg.norm(tg, axis=1, keepdims=True)
    level = _rays(np.zeros_like(tg), d)
    back = _rays(2.0 * tg, -d, tfar=1.5 * np.linalg.norm(tg, axis=1))
    axis_ray = _rays(np.zeros((1, 3)), (w / wl)[None, :])
    rr = np.concatenate([axis_ray, level, back, grid_rays(sc), box_rays(sc, 2048, 901)], axis=0)
    return Case(name, sc, _finish(rr), levels=len(tg), clusters=3 * levels)


def deep():
    return [deep_tree(), deep_tree(10, "deep_short")]


# -------------------------------------------------------------------------------------------- staging
def staged_bytes(nodes_over, tri_refs, spheres, refs_over):
    """build_lbvh's estimate of the LDS-staged bytes: BVH2 nodes of 64 B over nodes_over primitives, 48 B
    per triangle record, 16 B per sphere, the references padded to 16 B."""
    return max(nodes_over - 1, 0) * 64 + tri_refs * 48 + spheres * 16 + (refs_over + 3) // 4 * 16


def staging_counts():
    """(T, D): the largest triangle count staged into LDS; and for 8 degenerate extras the largest count of
    real triangles for which the estimate over N = T' still fits while the one over NP = T' + 8 does not."""
    lim = header_constant("kLdsSceneBytes")
    t = max(n for n in range(1, 2000) if staged_bytes(n, n, 0, n) <= lim)
    d = max(n for n in range(1, 2000) if staged_bytes(n, n + 8, 0, n) <= lim)
    assert staged_bytes(d + 8, d + 8, 0, d + 8) > lim
    return t, d


def staging():
    t, d = staging_counts()
    rng = np.random.default_rng(800)
    pos, idx = _random_tris(rng, t + 1, spread=2.0, size=0.3)
    pos = pos.reshape(-1, 3, 3)
    for k in range(0, t + 1, 16):  # slivers across the axes: a box far larger than the triangle
        c = pos[k, 0]
        pos[k, 1] = c + [1.5, 1.4, 1.3]
        pos[k, 2] = c + [1.5, 1.45, 1.3]
    out = []
    for n in (t - 1, t, t + 1):
        sc = make_scene(pos[:n].reshape(-1, 3), idx[:n], np.zeros((0, 4)))
        out.append(Case(f"staging_{n}", sc, standard_rays(sc, 4096, 810), above=n > t))
    dv, di, nd, _ = _degenerates(0)
    for n in (d - 1, d, d + 1):
        sc = make_scene(np.concatenate([pos[:n].reshape(-1, 3), dv]), np.concatenate([idx[:n], di[:nd] + 3 * n]),
                        np.zeros((0, 4)))
        assert nd == 7
        # an eighth: (i, i, i)
        sc = make_scene(sc["positions"], np.concatenate([sc["indices"], [[0, 0, 0]]]), np.zeros((0, 4)))
        out.append(Case(f"staging_{n}_deg8", sc, standard_rays(sc, 4096, 811), ndeg=8, above=True))
    return out


# ------------------------------------------------------------------------------------------- interval
def interval():
    base, rays = _mixed(), _mixed_rays()
    P = oracle.Prepared(base, bvh=False)
    g, _, t, _ = P.intersect(rays)
    pick = np.flatnonzero(g != MISS)
    pick = pick[:: max(1, len(pick) // 300)][:300]
    r0, t0 = rays[pick], t[pick]
    lo, hi = np.nextafter(t0, f32(0.0)), np.nextafter(t0, f32(np.inf))
    parts, tags = [], []

    def add(tag, rr):
        parts.append(rr)
        tags.append((tag, len(rr)))

    for tag, v in (("tfar-", lo), ("tfar=", t0), ("tfar+", hi)):
        rr = r0.copy()
        rr[:, 7] = v
        add(tag, rr)
    for tag, v in (("tnear-", lo), ("tnear=", t0), ("tnear+", hi)):
        rr = r0.copy()
        rr[:, 6] = v
        add(tag, rr)
    rr = r0.copy()
    rr[:, 6], rr[:, 7] = t0, f32(0.5) * t0
    add("tfar<tnear", rr)
    rr = r0.copy()
    rr[:, 7] = 0.0
    add("tfar=0", rr)
    rr = r0.copy()
    rr[:, 3:6] = 0.0
    add("d=0", rr)
    for k in (-10, 10):
        rr = r0.copy()
        rr[:, 3:6] *= f32(2.0) ** f32(k)
        add(f"d*2^{k}", rr)
    # exact ends: straight down onto the cube's top face from a dyadic height
    rng = np.random.default_rng(950)
    h = rng.integers(1, 32, 600) / 8.0
    o = np.stack([rng.integers(-5, 6, 600) / 8.0, 1.75 + h, 2.0 + rng.integers(-5, 6, 600) / 8.0], axis=1)
    dn = _rays(o, np.tile([0.0, -1.0, 0.0], (600, 1)))
    gg, _, tt, _ = P.intersect(dn)
    ex = (gg != MISS) & (gg < len(base["tri_geom_first"]) - 1) & (tt == h.astype(f32))
    dn, he = dn[ex][:200], h[ex][:200].astype(f32)
    for tag, col, v in (("exact tfar-", 7, np.nextafter(he, f32(0.0))), ("exact tfar=", 7, he),
                        ("exact tnear-", 6, np.nextafter(he, f32(0.0))), ("exact tnear=", 6, he)):
        rr = dn.copy()
        rr[:, col] = v
        add(tag, rr)
    spans, at = {}, 0
    for tag, n in tags:
        spans[tag] = slice(at, at + n)
        at += n
    return [Case("interval", base, _finish(np.concatenate(parts, axis=0)), spans=spans, t0=t0, exact_h=he)]


# ------------------------------------------------------------------------------------------- indexing
def indexing():
    rng = np.random.default_rng(1000)
    pos, idx = _random_tris(rng, 12, spread=1.5)
    full = rng.uniform(-1.5, 1.5, (54, 3))  # every third vertex (k % 3 == 2 of the padded list) is unused
    used = np.array([k for k in range(54) if k % 3 != 2])
    full[used] = pos
    sc = make_scene(full, used[idx], _random_spheres(rng, 3, 1.5), first=[0, 5, 5, 12, 12], materials=np.arange(7))
    return [Case("indexing", sc, standard_rays(sc, 4096, 1001))]


# -------------------------------------------------------------------------------------------- spheres
def spheres():
    rng = np.random.default_rng(1100)
    sph = np.concatenate([_random_spheres(rng, 8, 2.0), [[0.5, 0.25, -0.75, 0.0]]], axis=0)
    sc = make_scene(np.zeros((0, 3)), np.zeros((0, 3)), sph)
    s32 = sc["spheres"].astype(f64)
    o, d = [], []
    for c in s32[:8]:
        u = rng.normal(size=(24, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        v = rng.normal(size=(24, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        o += [c[:3] + 0.3 * c[3] * u[:8], c[:3] + c[3] * u[8:16], c[:3] + c[3] * u[8:16]]  # inside; on the surface
        d += [v[:8], v[8:16], -u[8:16]]
        # tangents: axis-parallel at distance exactly r, and a random tangent direction at a random point
        for ax in range(3):
            q, e = c[:3].copy(), np.zeros(3)
            q[(ax + 1) % 3] += c[3]
            q[ax] -= 5.0
            e[ax] = 1.0
            o.append(q[None, :])
            d.append(e[None, :])
        tdir = np.cross(u[16:24], v[16:24])
        tdir /= np.linalg.norm(tdir, axis=1, keepdims=True)
        o.append(c[:3] + c[3] * u[16:24] - 4.0 * tdir)
        d.append(tdir)
    z = s32[8, :3]
    u = rng.normal(size=(16, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o.append(z - 3.0 * u)
    d.append(u)
    rr = np.concatenate([_rays(np.concatenate(o), np.concatenate(d)), standard_rays(sc, 4096, 1101)], axis=0)
    out = [Case("spheres", sc, _finish(rr))]
    # zero-radius spheres on a line, and three at one point: wide nodes of zero extent in two and in three axes
    for name, cen in (("spheres_line", [[k, 2.0, 3.0] for k in range(5)]), ("spheres_point", [[1.0, 2.0, 3.0]] * 3)):
        pts = make_scene(np.zeros((0, 3)), np.zeros((0, 3)), np.concatenate([cen, np.zeros((len(cen), 1))], axis=1))
        o, d = [], []
        for c in cen:
            for ax in range(3):
                for sg in (1.0, -1.0):
                    q, e = np.array(c, f64), np.zeros(3)
                    q[ax] -= 3.0 * sg
                    e[ax] = sg
                    o.append(q)
                    d.append(e)
        par = _rays(np.array(o), np.array(d))
        off = par.copy()  # the same rays half a unit aside: clear misses (a random ray that passes a point within
        off[:, 0:3] += 0.5 * np.roll(np.abs(par[:, 3:6]), 1, axis=1)  # float32's noise "hits" its zero radius)
        out.append(Case(name, pts, _finish(np.concatenate([par, _signed_zero(par, True), off])), parallel=len(par)))
    return out


_BUILDERS = {"tiny": tiny, "equal": equal, "degenerate": degenerate, "axis": axis, "scale": scale, "offset": offset,
             "deep": deep, "staging": staging, "interval": interval, "indexing": indexing, "spheres": spheres}


@functools.lru_cache(maxsize=None)
def family(name: str):
    return tuple(_BUILDERS[name]())


@functools.lru_cache(maxsize=None)
def _reference(fam: str, k: int):
    c = family(fam)[k]
    P = oracle.Prepared(c.scene, bvh=False)
    hits, occ = P.intersect(c.rays), P.occluded(c.rays)
    for a in hits + (occ,):
        a.setflags(write=False)
    return hits, occ


def reference(fam: str, k: int):
    """(geom, prim, t, ng), occluded of case k of the family by the oracle's brute force: computed once."""
    return _reference(fam, k)


# --------------------------------------------------------------------------------------- comparison
def one_primitive(scene, geom, prim):
    """The scene holding just primitive (geom, prim) of `scene`."""
    ng = len(scene["tri_geom_first"]) - 1
    if geom < ng:
        tri = int(scene["tri_geom_first"][geom]) + int(prim)
        return make_scene(scene["positions"][scene["indices"][tri].astype(np.int64)], [[0, 1, 2]], np.zeros((0, 4)))
    return make_scene(np.zeros((0, 3)), np.zeros((0, 3)), scene["spheres"][geom - ng][None, :])


def marginal(scene, rays, geom, prim):
    """Per ray: whether its hit of (geom, prim) is, in float64 on the float32 inputs, within the float32
    error bound of a triangle edge (min(u, v, 1 - u - v) within query_common's bound of 0) or of a sphere's
    tangent (|disc| <= 16 * 2^-24 * (b^2 + 4 |a c|)); False where geom is a miss."""
    out = np.zeros(len(rays), bool)
    ntg = len(scene["tri_geom_first"]) - 1
    hit = geom != MISS
    tri = hit & (geom < ntg)
    if tri.any():
        idx = scene["tri_geom_first"].astype(np.int64)[geom[tri]] + prim[tri].astype(np.int64)
        with np.errstate(all="ignore"):
            u, v, den, bound, _ = Q.reference_uv(scene["positions"], scene["indices"], rays[tri], idx)
            out[tri] = ~(np.minimum(np.minimum(u, v), 1.0 - u - v) > bound)
    sp = hit & ~tri
    if sp.any():
        s = scene["spheres"].astype(f64)[geom[sp].astype(np.int64) - ntg]
        r = rays[sp].astype(f64)
        oc = r[:, 0:3] - s[:, :3]
        a = Q._dot(r[:, 3:6], r[:, 3:6])
        b = 2.0 * Q._dot(oc, r[:, 3:6])
        c = Q._dot(oc, oc) - s[:, 3] ** 2
        out[sp] = np.abs(b * b - 4.0 * a * c) <= 16.0 * Q.EPS * (b * b + 4.0 * np.abs(a * c))
    return out


def compare(case, got_hits, got_occ, ref_hits, ref_occ, what):
    """The module docstring's rule; got_hits / got_occ may be None.  Prints the counts; returns the number of
    excused rays."""
    n = len(case.rays)
    excused = np.zeros(n, bool)
    bad_t = bad_o = ids_n = 0
    if got_hits is not None:
        gg, gp, gt, gn = got_hits
        rg, rp, rt, rn = ref_hits
        t_ne = gt.view(np.uint32) != rt.view(np.uint32)
        if t_ne.any():
            k = np.flatnonzero(t_ne)
            m = marginal(case.scene, case.rays[k], np.where(rg[k] != MISS, rg[k], gg[k]), np.where(rg[k] != MISS, rp[k], gp[k]))
            excused[k[m]] = True
            bad_t = int((~m).sum())
            for q in k[~m][:8]:
                print(f"  {what}: ray {q} {case.rays[q]}: t {gt[q]!r} ({gg[q]}, {gp[q]}) vs reference {rt[q]!r} ({rg[q]}, {rp[q]})")
        ids = ((gg != rg) | (gp != rp)) & ~t_ne
        ids_n = int(ids.sum())
        same = ~ids & ~t_ne
        ng_ne = same & (gn.view(np.uint32) != rn.view(np.uint32)).any(axis=1)
        # a ray naming another primitive: that primitive alone must be hit at the same t
        wrong = 0
        if ids_n:
            assert (gg[ids] != MISS).all()
            pairs = np.unique(np.stack([gg[ids], gp[ids]], axis=1), axis=0)
            for g, p in pairs:
                sel = np.flatnonzero(ids & (gg == g) & (gp == p))
                _, _, t1, _ = oracle.Prepared(one_primitive(case.scene, int(g), int(p)), bvh=False).intersect(case.rays[sel])
                wrong += int((t1.view(np.uint32) != gt[sel].view(np.uint32)).sum())
    else:
        ng_ne, wrong = np.zeros(n, bool), 0
    if got_occ is not None:
        o_ne = got_occ != ref_occ
        if o_ne.any():
            k = np.flatnonzero(o_ne)
            # the occluder in question: the reference's closest hit with the ray's own interval
            rg, rp, _, _ = oracle.Prepared(case.scene, bvh=False).intersect(case.rays[k])
            m = marginal(case.scene, case.rays[k], rg, rp)
            excused[k[m]] = True
            bad_o = int((~m).sum())
            for q in k[~m][:8]:
                print(f"  {what}: ray {q} {case.rays[q]}: occluded {got_occ[q]} vs reference {ref_occ[q]}")
    hits = int((ref_hits[0] != MISS).sum())
    print(f"{what}: {n} rays, {hits} reference hits; t mismatches {bad_t}, occluded mismatches {bad_o}, "
          f"excused as marginal in float64 {int(excused.sum())}; {ids_n} name another primitive at a bit-equal t "
          f"({wrong} of them not hit there), {int(ng_ne.sum())} differ in Ng alone")
    assert bad_t == 0 and bad_o == 0, what
    assert excused.sum() <= R.CAP * n, what
    assert wrong == 0, what
    assert not ng_ne.any(), what
    return int(excused.sum())
