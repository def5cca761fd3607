"""Shared inputs of the signed-distance tests (test_signed_cpu.py, test_gpu_signed.py): small meshes built in numpy
with welded vertex, edge, open and irregular counts known by construction, their point sets, the host twin's answers
and the float64 reference's (signed_ref.py), each computed once per process and read-only, and the rule that says
which rows the sign comparison may leave out.

Meshes (MESHES: name -> (scene, {welded_vertices, edges, open_edges, irregular_edges})):
  star, star_unindexed, star_inverted, star_inverted_unindexed
           the unit cube [-0.5, 0.5]^3 with a pyramid on every face: apexes 2 above five faces and 0.35 below the sixth (a
           dent); 24 triangles, 14 vertices, 36 edges, closed.  Unindexed: every triangle with its own three
           vertices (72 positions), so only welding by position closes it.  Inverted: every triangle's last two
           indices swapped (the normals point inward).
  wedge    a tetrahedron whose faces at the edge (-1,0,0)-(1,0,0) meet at 15 degrees; 4 vertices, 6 edges.
  two_cubes  [0,1]^3 and [1,2]x[0,1]^2 as two geometries that share a face's four positions: they must not weld,
           so each stays closed: 16 vertices, 36 edges, none open.
  sheet    two triangles of the unit square in the plane z = 0: 4 vertices, 5 edges, 4 of them open.
  pole     an octahedron and one exactly degenerate triangle (top, top, +x) at its top vertex: the triangle is not
           live and takes no part: 6 vertices, 12 edges.
The sheet has no volume: its reference sign is the side of its plane.

Point sets of a mesh, 512 rows each (p.xyz, max_dist = inf): box (uniform in the bounds grown by half, each
half-extent at least a quarter of the largest so that a flat mesh has points well off its plane) and near
(points_common._near: surface samples moved along the normal by +-10^e, e uniform in [-6, 0]).

Rows the sign comparison may leave out (sign_rows), with eps = 2^-24 and M of points_common.magnitudes:
  - the float64 distance is below 64 eps M (DESIGN 6l puts the computed q within 19 eps M in norm);
  - |cos(p - q, N)| < 1e-3 in float64: q, the feature it lies on and N are the reference's own (signed_ref.
    reference_cos: the nearest point of the reference's nearest primitive and the float64 pseudonormal of its feature),
    so that which rows are compared does not depend on the code under test;
  - the nearest primitive of another geometry is within 64 eps M of the nearest, and the result names another
    geometry than the reference.
Caps on the rows left out: box sets 1 %, near sets 25 %.  Every other row must agree."""
import functools

import numpy as np

import adversarial_common as A
import points_common as P
import points_ref as PR
import signed_ref as SR
import sptr

NSET = 512
CLOSE = 64.0          # eps M
COS_MIN = 1e-3
CAP = {"box": 0.01, "near": 0.25}
FIELDS = P.FIELDS + ("signed_dist", "normal", "feature")
MISS = 0xFFFFFFFF


def _unindexed(sc):
    idx = sc["indices"].astype(np.int64)
    return A.make_scene(sc["positions"][idx].reshape(-1, 3), np.arange(3 * len(idx)).reshape(-1, 3), sc["spheres"],
                        first=sc["tri_geom_first"])


def _inverted(sc):
    return A.make_scene(sc["positions"], sc["indices"][:, [0, 2, 1]], sc["spheres"], first=sc["tri_geom_first"])


def _cube(lo, hi, base=0):
    """8 corners and 12 outward-wound triangles of the box [lo, hi]."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)])
    quads = ((0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5))  # -z +z -y +y -x +x
    tris = []
    for q in quads:
        tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return v, np.array(tris) + base, quads


def _star():
    v, _, quads = _cube((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    pos, tris = [p for p in v], []
    for f, q in enumerate(quads):
        c = v[list(q)].mean(axis=0)  # the face centre: half the unit outward normal of this cube
        apex = c + 2.0 * c * (2.0 if f != 3 else -0.35)
        pos.append(apex)
        for i in range(4):
            tris.append((q[i], q[(i + 1) % 4], 8 + f))
    return A.make_scene(np.array(pos), np.array(tris), np.zeros((0, 4)))


def _wedge():
    h = np.tan(np.radians(7.5))
    pos = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, h], [0.0, 1.0, -h]])
    tris = [(0, 1, 2), (1, 0, 3), (0, 2, 3), (1, 3, 2)]
    cen = pos.mean(axis=0)
    out = []
    for a, b, c in tris:  # outward: the normal points away from the centroid
        n = np.cross(pos[b] - pos[a], pos[c] - pos[a])
        out.append((a, b, c) if np.dot(n, pos[a] - cen) > 0 else (a, c, b))
    return A.make_scene(pos, np.array(out), np.zeros((0, 4)))


def _two_cubes():
    v0, t0, _ = _cube((0, 0, 0), (1, 1, 1))
    v1, t1, _ = _cube((1, 0, 0), (2, 1, 1), base=8)
    return A.make_scene(np.concatenate([v0, v1]), np.concatenate([t0, t1]), np.zeros((0, 4)), first=[0, 12, 24])


def _sheet():
    return A.make_scene([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 1, 2], [0, 2, 3]], np.zeros((0, 4)))


def _pole():
    pos = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    tris = []
    for i in range(4):
        a, b = i, (i + 1) % 4
        tris += [(a, b, 4), (b, a, 5)]
    tris.insert(3, (4, 4, 0))  # exactly degenerate, at the top
    return A.make_scene(pos, np.array(tris), np.zeros((0, 4)))


def _counts(v, e, o=0, i=0):
    return {"welded_vertices": v, "edges": e, "open_edges": o, "irregular_edges": i}


@functools.lru_cache(maxsize=None)
def meshes():
    star = _star()
    return {
        "star": (star, _counts(14, 36)),
        "star_unindexed": (_unindexed(star), _counts(14, 36)),
        "star_inverted": (_inverted(star), _counts(14, 36)),
        "star_inverted_unindexed": (_unindexed(_inverted(star)), _counts(14, 36)),
        "wedge": (_wedge(), _counts(4, 6)),
        "two_cubes": (_two_cubes(), _counts(16, 36)),
        "sheet": (_sheet(), _counts(4, 5, 4, 4)),
        "pole": (_pole(), _counts(6, 12)),
    }


MESH_NAMES = ("star", "star_unindexed", "star_inverted", "star_inverted_unindexed", "wedge", "two_cubes", "sheet", "pole")
QUERY_SCENES = ("default_emitter", "sphere_mesh")
ALL_NAMES = MESH_NAMES + QUERY_SCENES


def scene(name):
    return P.query_scene(name) if name in QUERY_SCENES else meshes()[name][0]


@functools.lru_cache(maxsize=None)
def point_sets(name):
    """{"box", "near": (n, 4) float32, read-only}: points_common's sets for a query scene, 512 rows each for a mesh."""
    if name in QUERY_SCENES:
        s = P.point_sets(name)
        return {"box": s["box"], "near": s["near"]}
    base = name.replace("_unindexed", "").replace("_inverted", "")  # the star's variants share the star's points
    if base != name:
        return point_sets(base)
    sc = scene(name)
    rng = np.random.default_rng(43)
    c, _, lo, hi = A.bounds(sc)
    half = 0.5 * (hi - lo)
    half = np.maximum(half, 0.25 * half.max())  # (a flat mesh gets a box with points well off its plane)
    sets = {"box": P._pack(rng.uniform(c - 1.5 * half, c + 1.5 * half, (NSET, 3))), "near": P._pack(P._near(sc, rng, NSET))}
    for a in sets.values():
        a.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def all_points(name):
    """Every row the GPU test compares: points_common.points(name) for a query scene (all six sets), box + near for a
    mesh."""
    if name in QUERY_SCENES:
        return P.points(name)[0]
    s = point_sets(name)
    out = np.concatenate([s["box"], s["near"]], axis=0)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin(name, flip=False):
    return P._frozen(sptr.host_query_signed_distance(P.flat(scene(name)), all_points(name), flip_triangles=flip))


@functools.lru_cache(maxsize=None)
def twin_set(name, which, flip=False):
    return P._frozen(sptr.host_query_signed_distance(P.flat(scene(name)), point_sets(name)[which], flip_triangles=flip))


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """(points_ref.nearest, reference sign) of one set."""
    sc, pts = scene(name), point_sets(name)[which]
    near = PR.nearest(sc, pts)
    if name == "sheet":  # no volume: the side of its plane, which its normals (+z) point to
        sign = np.where(np.asarray(pts, np.float64)[:, 2] < 0.0, -1.0, 1.0)
    else:
        sign = SR.reference_sign(sc, pts, near)
    sign.setflags(write=False)
    return P._frozen(near), sign


@functools.lru_cache(maxsize=None)
def _tables64(name):
    return SR.pseudonormals(scene(name))


def sign_rows(sc, pts, got, near, tables):
    """(rows to compare, rows left out) as boolean masks over pts, by the rule in this module's docstring.  got: a
    signed query's result (its geom alone is read, to narrow the third condition); near: points_ref.nearest of the
    same points; tables: signed_ref.pseudonormals(sc)."""
    M = P.magnitudes(sc, pts)
    hit = got["geom"] != MISS
    close = near["dist"] < CLOSE * P.EPS * M
    grazing = SR.reference_cos(sc, pts, near, tables) < COS_MIN
    other = SR.other_geom_distance(sc, pts, near["geom"].astype(np.int64))
    contested = (other - near["dist"] <= CLOSE * P.EPS * M) & (got["geom"] != near["geom"])
    out = hit & (close | grazing | contested)
    return hit & ~out, out


def check_signs(name, which, got, what, rows=slice(None)):
    """Asserts the rule for one set (or its rows `rows`, with got holding those rows): the rows left out stay under the
    cap, every other row has the reference's sign.  Prints the figures.  Returns (compared, left out, wrong)."""
    sc, pts = scene(name), point_sets(name)[which][rows]
    near, ref = reference(name, which)
    near, ref = {k: v[rows] for k, v in near.items()}, ref[rows]
    keep, out = sign_rows(sc, pts, got, near, _tables64(name))
    sign = np.where(np.signbit(got["signed_dist"]), -1.0, 1.0)
    wrong = keep & (sign != ref)
    print(f"{what} {name}/{which}: {int(keep.sum())} rows compared, {int(out.sum())} left out "
          f"({out.sum() / len(pts):.1%}, cap {CAP[which]:.0%}), {int(wrong.sum())} wrong; "
          f"{int((ref < 0).sum())} reference rows are negative")
    assert keep.sum() + out.sum() == len(pts), f"{what} {name}/{which}: a row missed"
    assert out.sum() <= CAP[which] * len(pts), f"{what} {name}/{which}: too many rows left out"
    assert not wrong.any(), f"{what} {name}/{which}: rows {np.flatnonzero(wrong)[:8]} have the wrong sign"
    return int(keep.sum()), int(out.sum()), int(wrong.sum())


def direction_error(got, ref):
    """Largest angle (rad, float64) between rows of got and ref (..., 3), over rows whose reference is not ~0; and the
    largest |got| where the reference is ~0, relative to the largest reference norm."""
    g, r = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    rn, gn = np.linalg.norm(r, axis=1), np.linalg.norm(g, axis=1)
    big = rn > 1e-6 * max(1e-300, rn.max(initial=0.0))
    cr = np.linalg.norm(np.cross(g[big], r[big]), axis=1)
    ang = np.arctan2(cr, (g[big] * r[big]).sum(1))
    small = float(gn[~big].max(initial=0.0) / max(1e-300, rn.max(initial=0.0)))
    return float(ang.max(initial=0.0)), small
