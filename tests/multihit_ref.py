"""Reference of the multi-hit query (sptr_query_multi_hit), with no tree and no device.

For every primitive (g, p) of a flat scene the oracle's brute force on the scene of that one primitive
(oracle.Prepared(adversarial_common.one_primitive(scene, g, p), bvh=False).intersect(rays)) gives that primitive's
candidate hit per ray in the reference's float32 arithmetic.  A sphere gets a second call, for the rays that hit,
with each ray's tnear replaced by the first t: the second candidate, reported with prim = 1.  Per ray all
candidates are sorted by (t, geom, prim), t compared as float and the ids as unsigned, and cut.

lists(scene, rays) keeps the first KMAX + 1 = 17 candidates of every ray (one more than any K, for the marginal
count of tests/test_multihit_cpu.py); cut(ref, K) is the expected output for max_hits = K, filled tail included."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import adversarial_common as A
import oracle

MISS = 0xFFFFFFFF
KMAX = 16
KEEP = KMAX + 1
f32 = np.float32


def _primitives(scene):
    first = scene["tri_geom_first"].astype(np.int64)
    ntg = len(first) - 1
    out = [(g, p) for g in range(ntg) for p in range(int(first[g + 1] - first[g]))]
    return out + [(ntg + s, 0) for s in range(len(scene["spheres"]))], ntg


def _one(scene, rays, g, p, sphere):
    """Candidates of primitive (g, p): (ray index, t, geom, prim, ng) arrays."""
    P = oracle.Prepared(A.one_primitive(scene, g, p), bvh=False)
    gg, _, t, ng = P.intersect(rays)
    k = np.flatnonzero(gg != MISS)
    parts = [(k, t[k], np.full(len(k), g, np.uint32), np.full(len(k), p, np.uint32), ng[k])]
    if sphere and len(k):
        again = rays[k].copy()
        again[:, 6] = t[k]
        g2, _, t2, n2 = P.intersect(again)
        k2 = np.flatnonzero(g2 != MISS)
        parts.append((k[k2], t2[k2], np.full(len(k2), g, np.uint32), np.ones(len(k2), np.uint32), n2[k2]))
    return parts


def lists(scene, rays, threads=None):
    """dict: total (n,) candidates per ray; geom, prim (n, 17) uint32, t (n, 17), ng (n, 17, 3) float32: the
    first 17 candidates of each ray in key order, the rest filled as the query fills its tail."""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    n = len(rays)
    prims, ntg = _primitives(scene)
    threads = threads or min(8, os.cpu_count() or 1)
    with ThreadPoolExecutor(threads) as pool:  # (the brute-force loops run outside the interpreter lock)
        res = list(pool.map(lambda gp: _one(scene, rays, gp[0], gp[1], gp[0] >= ntg), prims))
    parts = [x for r in res for x in r]
    out = {"total": np.zeros(n, np.uint32), "geom": np.full((n, KEEP), MISS, np.uint32),
           "prim": np.full((n, KEEP), MISS, np.uint32), "t": np.full((n, KEEP), np.inf, f32),
           "ng": np.zeros((n, KEEP, 3), f32)}
    if parts:
        ray = np.concatenate([x[0] for x in parts])
        t = np.concatenate([x[1] for x in parts])
        geom = np.concatenate([x[2] for x in parts])
        prim = np.concatenate([x[3] for x in parts])
        ng = np.concatenate([x[4] for x in parts])
        order = np.lexsort((prim, geom, t, ray))  # by ray, then (t, geom, prim)
        ray, t, geom, prim, ng = ray[order], t[order], geom[order], prim[order], ng[order]
        out["total"] = np.bincount(ray, minlength=n).astype(np.uint32)
        start = np.concatenate([[0], np.cumsum(out["total"].astype(np.int64))])[:-1]
        rank = np.arange(len(ray)) - start[ray]
        keep = rank < KEEP
        r, j = ray[keep], rank[keep]
        out["geom"][r, j], out["prim"][r, j], out["t"][r, j], out["ng"][r, j] = geom[keep], prim[keep], t[keep], ng[keep]
    for a in out.values():
        a.setflags(write=False)
    return out


def cut(ref, K):
    """The expected count, geom, prim, t, ng of max_hits = K."""
    count = np.minimum(ref["total"], K).astype(np.uint32)
    out = {"count": count}
    for name in ("geom", "prim", "t", "ng"):
        out[name] = np.ascontiguousarray(ref[name][:, :K])
    return out


def tie_at(ref, j):
    """Per ray: slots j and j + 1 both hold a hit, at float-equal t."""
    return (ref["geom"][:, j + 1] != MISS) & (ref["t"][:, j] == ref["t"][:, j + 1])


def marginal_rays(scene, rays, ref, K):
    """Per ray: whether one of its first K + 1 reference candidates is marginal (adversarial_common.marginal)."""
    flag = np.zeros(len(rays), bool)
    for j in range(K + 1):
        flag |= A.marginal(scene, rays, ref["geom"][:, j], ref["prim"][:, j])
    return flag
