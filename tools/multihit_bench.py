#!/usr/bin/env python3
"""Multi-hit query measurement: sptr_query_multi_hit with device pointers for K = 1, 4, 5, 16 beside
sptr_query_rays closest-hit on the same rays in the same process.

Scenes: the tests' two (tests/refit_common.py): default_emitter, staged into LDS, and the 30x70 sphere mesh with
set_bvh_width(4), the BVH4 walked from L2.  Rays: 2^--log2n (default 22) rays built as the tests' shape_rays builds
them: default_rng(11), origins uniform in [-6,6]x[0,5]x[-6,8] aimed at targets uniform in [-3,3]x[0,3]x[-3,5].
Every variant is warmed up, then the variants alternate inside each of --reps repetitions; the times are the device
ms_trace of sptr_query_info / sptr_multi_hit_info (events around the trace launch; nothing is sorted).  Variants:
  closest   : one sptr_query_rays batch, all five outputs (the existing code: the yardstick);
  closest x4: what a caller had before, 4 successive closest-hit batches with tnear advanced to the last t (the sum
              of the four ms_trace).  Its result is not the multi-hit result: ties and coincident faces are lost, a
              triangle can be found twice, and a sphere's exit is found only because tnear moved;
  multi K   : one sptr_query_multi_hit batch, count and all five per-hit outputs;
  multi K, count only: the same batch with every per-hit output NULL: the walk and the list without the records.
Printed per variant: every repetition, the median, the spread (max - min) and the ratio of the medians to closest.
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

SCENES = [("default_emitter", 0, 0, 0), ("sphere_mesh", 30, 70, 4)]
KS = (1, 4, 5, 16)  # 5: the first K of the larger list capacity, beside 4, the last of the smaller
DEV = "cuda:0"


def make_rays(n):
    rng = np.random.default_rng(11)
    o = rng.uniform([-6.0, 0.0, -6.0], [6.0, 5.0, 8.0], (n, 3))
    tg = rng.uniform([-3.0, 0.0, -3.0], [3.0, 3.0, 5.0], (n, 3))
    d = tg - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rr = np.zeros((n, 8), np.float32)
    rr[:, 0:3] = o
    rr[:, 3:6] = d
    rr[:, 7] = np.inf
    return torch.from_numpy(rr).to(DEV).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = 1 << a.log2n
    rays = make_rays(n)
    step = rays.clone()
    torch.cuda.synchronize()
    for name, p0, p1, width in SCENES:
        r = sptr.Renderer(0)
        r.set_bvh_width(width)
        r.upload_scene(sptr.builtin_scene(name, p0, p1))
        lay = r.scene_layout()
        print(f"# scene {name}: {lay['num_tris']} triangles, {lay['num_spheres']} spheres, BVH{lay['bvh_width']}, "
              f"lds_bytes {lay['lds_bytes']}, n = 2^{a.log2n} rays", flush=True)
        outs = {}

        def closest(src=rays, key="closest"):
            outs[key] = r.query_rays(src, sort=False, out=outs.get(key))
            return r.query_info()["ms_trace"]

        def closest_x4():
            step.copy_(rays)
            total = 0.0
            for _ in range(4):
                total += closest(step, "step")
                step[:, 6] = outs["step"]["t"]  # a miss: tnear = inf, the next batch misses again
            return total

        def multi(K, fields=None):
            key = K if fields is None else (K, "count")
            outs[key] = r.query_multi_hit(rays, K, sort=False, fields=fields, out=outs.get(key))
            return r.multi_hit_info()["ms_trace"]

        variants = [("closest", closest), ("closest x4", closest_x4)] + [(f"multi K={K}", lambda K=K: multi(K)) for K in KS]
        variants += [(f"multi K={K}, count only", lambda K=K: multi(K, ())) for K in KS]
        for _, fn in variants:  # warm-up of every shape
            fn()
        ms = {v: [] for v, _ in variants}
        for _ in range(a.reps):
            for v, fn in variants:
                ms[v].append(fn())
        for K in KS:
            r.query_multi_hit(rays[:4096].contiguous(), K, sort=False)
            info = r.multi_hit_info()
            print(f"# K={K}: list capacity {info['list_capacity']}, LDS bytes per block {info['lds_bytes']}, "
                  f"hits listed {int(outs[K]['count'].to(torch.int64).sum())} of {n} rays", flush=True)
        t1 = outs[1]["t"][:, 0].contiguous()
        same = bool(torch.equal(t1.view(torch.int32), outs["closest"]["t"].view(torch.int32)))
        print(f"# K=1 t equals closest-hit t bit for bit: {same}")
        base = float(np.median(ms["closest"]))
        for v, _ in variants:
            x = ms[v]
            med = float(np.median(x))
            print(json.dumps({"scene": name, "variant": v, "ms_trace": [round(t, 4) for t in x], "median": round(med, 4),
                              "spread": round(max(x) - min(x), 4), "ratio_to_closest": round(med / base, 3),
                              "mrays_per_s": round(n / (med * 1e3), 1)}), flush=True)
        outs.clear()
        r.close()


if __name__ == "__main__":
    main()
