#!/usr/bin/env python3
"""Ray-query measurement: sptr_query_rays with device pointers, sorted against unsorted.

Scenes: C2's (default_emitter, staged into LDS) and C5's (the 10M-triangle sphere mesh, walked from HBM).
Ray sets, generated on the device from a seed, n rays each:
  camera : the 1920x1080 pixel-centre rays of the default camera, tiled to n;
  ao     : origins = the first hits of the camera rays, 1e-3 along the normal facing the camera, directions
           uniform on the hemisphere about it, tfar inf (the hits tiled to n);
  random : origins uniform in the scene's bounding box, aimed at uniform targets in it.
Per scene, set, size and query kind (closest / any hit): each shape is warmed up, then sort=False and
sort=True alternate inside this one process, --reps times each; ms_sort and ms_trace are the device times
sptr_query_info reports (events around the key + radix-sort launches and around the trace launch).  Printed
per variant: the repetitions, their median and spread (max - min), and Mrays/s over the median total.  The
sorted and unsorted outputs are compared at the measured size (they must be equal byte for byte).

--legacy: instead, one sptr_intersect and one sptr_occluded call per scene and set on the same rays (host
arrays, k_query), for a kernel-trace run of its own:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/query_bench.py --legacy --sizes 21
There is no CPU fallback: without a GPU the Renderer raises."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-path-tracer_amd"))
import sptr  # noqa: E402
import workloads  # noqa: E402

W, H = 1920, 1080
DEV = "cuda:0"


def camera_rays(cam: np.ndarray, n: int) -> torch.Tensor:
    """camera_dir((x + 0.5) / W, (y + 0.5) / H) in float32 on the device, tiled to n rays."""
    c = torch.tensor(cam, dtype=torch.float32, device=DEV)
    fw, rt, up, hw, hh = c[3:6], c[6:9], c[9:12], c[12], c[13]
    u = (torch.arange(W, dtype=torch.float32, device=DEV) + 0.5) / W
    v = (torch.arange(H, dtype=torch.float32, device=DEV) + 0.5) / H
    nx = ((u - 0.5) * 2.0)[None, :, None]
    ny = (-(v - 0.5) * 2.0)[:, None, None]
    d = (fw + (nx * hw) * rt) + (ny * hh) * up
    d = (d / d.norm(dim=2, keepdim=True)).reshape(-1, 3)
    idx = torch.arange(n, device=DEV) % (W * H)
    r = torch.zeros((n, 8), dtype=torch.float32, device=DEV)
    r[:, 0:3] = c[0:3]
    r[:, 3:6] = d[idx]
    r[:, 7] = float("inf")
    return r.contiguous()


def ao_rays(r: "sptr.Renderer", cam_rays: torch.Tensor, n: int, gen: torch.Generator) -> torch.Tensor:
    first = r.query_rays(cam_rays[:W * H].contiguous(), sort=False, fields=("t", "ng"))
    hit = torch.isfinite(first["t"])
    o, d = cam_rays[:W * H, 0:3][hit], cam_rays[:W * H, 3:6][hit]
    nn = first["ng"][hit]
    nn = nn / nn.norm(dim=1, keepdim=True)
    nn = torch.where(((nn * d).sum(dim=1) > 0)[:, None], -nn, nn)
    p = o + first["t"][hit][:, None] * d + 1e-3 * nn
    idx = torch.arange(n, device=DEV) % p.shape[0]
    p, nn = p[idx], nn[idx]
    w = torch.randn((n, 3), generator=gen, device=DEV, dtype=torch.float32)
    w = w / w.norm(dim=1, keepdim=True)
    w = torch.where(((w * nn).sum(dim=1) < 0)[:, None], -w, w)
    out = torch.zeros((n, 8), dtype=torch.float32, device=DEV)
    out[:, 0:3] = p
    out[:, 3:6] = w
    out[:, 7] = float("inf")
    return out.contiguous()


def random_rays(flat: "sptr.FlatScene", n: int, gen: torch.Generator) -> torch.Tensor:
    lo = flat.positions.min(axis=0) if len(flat.positions) else np.full(3, np.inf)
    hi = flat.positions.max(axis=0) if len(flat.positions) else np.full(3, -np.inf)
    if len(flat.spheres):
        lo = np.minimum(lo, (flat.spheres[:, 0:3] - flat.spheres[:, 3:4]).min(axis=0))
        hi = np.maximum(hi, (flat.spheres[:, 0:3] + flat.spheres[:, 3:4]).max(axis=0))
    lo_t = torch.tensor(lo, dtype=torch.float32, device=DEV)
    ext = torch.tensor(hi - lo, dtype=torch.float32, device=DEV)
    o = lo_t + ext * torch.rand((n, 3), generator=gen, device=DEV, dtype=torch.float32)
    tg = lo_t + ext * torch.rand((n, 3), generator=gen, device=DEV, dtype=torch.float32)
    d = tg - o
    d = d / d.norm(dim=1, keepdim=True)
    out = torch.zeros((n, 8), dtype=torch.float32, device=DEV)
    out[:, 0:3] = o
    out[:, 3:6] = d
    out[:, 7] = float("inf")
    return out.contiguous()


def measure(r, rays, any_hit, reps):
    fields = None if any_hit else ("geom", "prim", "t", "ng", "uv")
    out = {}
    for sort in (False, True):  # warm-up of both shapes, and the equality of their results
        out[sort] = r.query_rays(rays, any_hit=any_hit, sort=sort, fields=fields)
        r.query_info()
    equal = all(torch.equal(out[False][k].view(torch.uint8), out[True][k].view(torch.uint8)) for k in out[False])
    ms = {False: [], True: []}
    for _ in range(reps):
        for sort in (False, True):
            r.query_rays(rays, any_hit=any_hit, sort=sort, fields=fields, out=out[sort])
            info = r.query_info()
            assert info["sorted"] == int(sort)
            ms[sort].append((info["ms_sort"], info["ms_trace"]))
    return ms, equal


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="21,24", help="log2 of the batch sizes")
    ap.add_argument("--scenes", default="c2,c5")
    ap.add_argument("--sets", default="camera,ao,random")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--legacy", action="store_true", help="one sptr_intersect / sptr_occluded call per shape instead")
    a = ap.parse_args()
    sizes = [1 << int(s) for s in a.sizes.split(",")]
    results = []
    for name in a.scenes.split(","):
        wl = workloads.WORKLOADS[name]
        r = sptr.Renderer(0)
        flat = workloads.setup(r, wl)
        lay = r.scene_layout()
        print(f"# scene {name}: {lay['num_tris']} triangles, {lay['num_spheres']} spheres, BVH{lay['bvh_width']}, "
              f"lds_bytes {lay['lds_bytes']}", flush=True)
        cam = workloads.camera(wl).as_array()
        for n in sizes:
            gen = torch.Generator(device=DEV)
            gen.manual_seed(a.seed)
            base = camera_rays(cam, n)
            for rset in a.sets.split(","):
                rays = {"camera": lambda: base, "ao": lambda: ao_rays(r, base, n, gen),
                        "random": lambda: random_rays(flat, n, gen)}[rset]()
                torch.cuda.synchronize()
                if a.legacy:
                    host = rays.cpu().numpy()
                    r.intersect(host[:4096])  # (code objects loaded before the traced calls)
                    hits = r.intersect(host)
                    occ = r.occluded(host)
                    print(f"legacy {name} {rset} n=2^{n.bit_length() - 1}: {int((hits[0] != 0xFFFFFFFF).sum())} hits, "
                          f"{int(occ.sum())} occluded", flush=True)
                    continue
                for any_hit in (False, True):
                    ms, equal = measure(r, rays, any_hit, a.reps)
                    row = {"scene": name, "set": rset, "n": n, "kind": "any" if any_hit else "closest",
                           "sorted_equals_unsorted": equal}
                    for sort in (False, True):
                        tot = sorted(s + t for s, t in ms[sort])
                        med = tot[len(tot) // 2]
                        key = "sort" if sort else "nosort"
                        row[key] = {"ms_sort": [round(s, 4) for s, _ in ms[sort]], "ms_trace": [round(t, 4) for _, t in ms[sort]],
                                    "ms_total_median": round(med, 4), "ms_total_spread": round(tot[-1] - tot[0], 4),
                                    "mrays_per_s": round(n / (med * 1e3), 1)}
                    results.append(row)
                    print(json.dumps(row), flush=True)
                del rays
        r.close()
    if not a.legacy:
        print("# scene set n kind | nosort ms (spread) Mrays/s | sort: ms_sort + ms_trace = ms (spread) Mrays/s | equal")
        for x in results:
            ns, so = x["nosort"], x["sort"]
            print(f"{x['scene']} {x['set']:6s} 2^{x['n'].bit_length() - 1} {x['kind']:7s} | {ns['ms_total_median']:9.3f} "
                  f"({ns['ms_total_spread']:.3f}) {ns['mrays_per_s']:9.1f} | {sorted(so['ms_sort'])[len(so['ms_sort']) // 2]:8.3f} + "
                  f"{sorted(so['ms_trace'])[len(so['ms_trace']) // 2]:8.3f} = {so['ms_total_median']:9.3f} ({so['ms_total_spread']:.3f}) "
                  f"{so['mrays_per_s']:9.1f} | {x['sorted_equals_unsorted']}")


if __name__ == "__main__":
    main()
