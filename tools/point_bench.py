#!/usr/bin/env python3
"""Closest-point query measurement: sptr_query_points with device pointers, sort off and on
alternating in one process.

Scenes: C2's (default_emitter, staged into LDS) and the sphere mesh --mesh STACKS SLICES (default 1250 4000, the
10M-triangle mesh walked from HBM through the BVH4).  Point sets, made on the device with torch.manual_seed(13),
max_dist = inf:
  near : a uniform triangle (or sphere, by their share of the primitives), a uniform point on it, moved along the
         unit normal by +-10^e, e uniform in [-6, 0];
  box  : uniform in the scene's bounds grown by half about their centre;
  far  : 10^3 away from the centre in uniform directions.
Per scene, set and n = 2^k for k in --log2n (default 21 24): one warm-up of each order, then --reps (default 3)
repetitions of unsorted, sorted alternating; the times are ms_sort + ms_walk of sptr_point_query_info (device events).
Printed per order: every repetition, the median, the spread (max - min), Mpoints/s at the median, and the node visits
and primitive tests per point of one further SPTR_POINT_COUNT query; and whether the sorted and the unsorted outputs
are equal byte for byte.  There is no CPU fallback: without a GPU the Renderer raises."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-path-tracer_amd"))
import sptr  # noqa: E402

DEV = "cuda:0"


def bounds(flat):
    lo, hi = [], []
    if len(flat.indices):
        p = flat.positions[np.unique(flat.indices)]
        lo.append(p.min(axis=0))
        hi.append(p.max(axis=0))
    if len(flat.spheres):
        s = flat.spheres.astype(np.float64)
        lo.append((s[:, :3] - s[:, 3:4]).min(axis=0))
        hi.append((s[:, :3] + s[:, 3:4]).max(axis=0))
    lo, hi = np.min(lo, axis=0).astype(np.float64), np.max(hi, axis=0).astype(np.float64)
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


def unit(n):
    d = torch.randn(n, 3, device=DEV, dtype=torch.float64)
    return d / d.norm(dim=1, keepdim=True)


def make_points(flat, kind, n):
    c, half = bounds(flat)
    c, half = torch.tensor(c, device=DEV), torch.tensor(half, device=DEV)
    if kind == "box":
        p = c + 1.5 * half * (2.0 * torch.rand(n, 3, device=DEV, dtype=torch.float64) - 1.0)
    elif kind == "far":
        p = c + 1e3 * unit(n)
    else:
        nt, ns = len(flat.indices), len(flat.spheres)
        off = torch.where(torch.rand(n, device=DEV) < 0.5, -1.0, 1.0).double() * 10.0 ** (-6.0 * torch.rand(n, device=DEV, dtype=torch.float64))
        which = torch.randint(0, nt + ns, (n,), device=DEV)
        p = torch.zeros(n, 3, device=DEV, dtype=torch.float64)
        if nt:
            pos = torch.from_numpy(flat.positions.astype(np.float64)).to(DEV)
            idx = torch.from_numpy(flat.indices.astype(np.int64)).to(DEV)
            t = torch.clamp(which, max=nt - 1)
            a, b, cc = pos[idx[t, 0]], pos[idx[t, 1]], pos[idx[t, 2]]
            r1, r2 = torch.rand(n, 1, device=DEV, dtype=torch.float64).sqrt(), torch.rand(n, 1, device=DEV, dtype=torch.float64)
            nrm = torch.cross(b - a, cc - a, dim=1)
            nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-300)
            p = (1.0 - r1) * a + r1 * (1.0 - r2) * b + r1 * r2 * cc + off[:, None] * nrm
        if ns:
            sph = torch.from_numpy(flat.spheres.astype(np.float64)).to(DEV)
            s = sph[torch.clamp(which - nt, min=0)]
            ps = s[:, :3] + (s[:, 3:4] + off[:, None]) * unit(n)
            p = torch.where((which >= nt)[:, None], ps, p)
    out = torch.empty(n, 4, device=DEV, dtype=torch.float32)
    out[:, :3] = p.float()
    out[:, 3] = float("inf")
    return out.contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, nargs="+", default=[21, 24])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", nargs="+", default=["default_emitter", "sphere_mesh"])
    ap.add_argument("--mesh", type=int, nargs=2, default=[1250, 4000])
    ap.add_argument("--sets", nargs="+", default=["near", "box", "far"])
    a = ap.parse_args()
    torch.manual_seed(13)
    for name in a.scenes:
        p0, p1 = (a.mesh if name == "sphere_mesh" else (0, 0))
        flat = sptr.builtin_scene(name, p0, p1)
        r = sptr.Renderer(0)
        r.upload_scene(flat)
        lay = r.scene_layout()
        prims = lay["num_tris"] + lay["num_spheres"]
        print(f"# scene {name} {p0} {p1}: {lay['num_tris']} triangles, {lay['num_spheres']} spheres, BVH{lay['bvh_width']}, "
              f"lds_bytes {lay['lds_bytes']}", flush=True)
        for kind in a.sets:
            for k in a.log2n:
                n = 1 << k
                pts = make_points(flat, kind, n)
                torch.cuda.synchronize()
                outs = {False: None, True: None}
                ms = {False: [], True: []}

                def run(sort, count=False):
                    outs[sort] = r.query_points(pts, sort=sort, out=outs[sort], count=count)
                    return r.point_query_info()

                for sort in (False, True):
                    run(sort)
                for _ in range(a.reps):
                    for sort in (False, True):
                        info = run(sort)
                        ms[sort].append(info["ms_sort"] + info["ms_walk"])
                same = all(torch.equal(outs[False][f].view(torch.int32), outs[True][f].view(torch.int32)) for f in outs[False])
                for sort in (False, True):
                    info = run(sort, count=True)
                    x = ms[sort]
                    med = float(np.median(x))
                    print(json.dumps({"scene": name, "set": kind, "log2n": k, "sorted": int(sort), "ms": [round(t, 4) for t in x],
                                      "median": round(med, 4), "spread": round(max(x) - min(x), 4),
                                      "ms_sort_last": round(info["ms_sort"], 4), "mpoints_per_s": round(n / (med * 1e3), 1),
                                      "visits_per_point": round(info["node_visits"] / n, 2),
                                      "tests_per_point": round(info["prim_tests"] / n, 2), "primitives": prims,
                                      "sorted_equals_unsorted": same}), flush=True)
                del pts, outs
        r.close()


if __name__ == "__main__":
    main()
