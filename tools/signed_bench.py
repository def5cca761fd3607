#!/usr/bin/env python3
"""Signed distance measurement, with tools/point_bench.py's method: device pointers, device events,
one warm-up, then --reps repetitions; every repetition, the median and the spread (max - min) are printed.

--build: per scene the device ms of the pseudonormal table build (sptr_signed_info ms_build) next to that upload's
  BVH build_ms, over --reps uploads, with the table's counts and bytes.  Scenes: default_emitter, the 30 x 70 sphere
  mesh and the sphere mesh --mesh STACKS SLICES (default 1250 4000, the 10M-triangle mesh).
--query: on default_emitter, point_bench's box set, n = 2^k for k in --log2n (default 21 24): the sign pass
  (ms_sign) against the walk (ms_walk) of sptr_query_signed_distance.
--points: on default_emitter, box set, n = 2^21: the walk time of plain sptr_query_points (for the comparison of this
  tree with its parent, which has no other mode of this tool).
There is no CPU fallback: without a GPU the Renderer raises."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-path-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sptr  # noqa: E402
from point_bench import make_points  # noqa: E402


def stats(x):
    return {"ms": [round(t, 4) for t in x], "median": round(float(np.median(x)), 4), "spread": round(max(x) - min(x), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--query", action="store_true")
    ap.add_argument("--points", action="store_true")
    ap.add_argument("--log2n", type=int, nargs="+", default=[21, 24])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mesh", type=int, nargs=2, default=[1250, 4000])
    ap.add_argument("--no-big", action="store_true", help="--build without the --mesh scene")
    a = ap.parse_args()
    torch.manual_seed(13)
    if a.build:
        scenes = [("default_emitter", 0, 0), ("sphere_mesh", 30, 70)] + ([] if a.no_big else [("sphere_mesh", *a.mesh)])
        for name, p0, p1 in scenes:
            flat = sptr.builtin_scene(name, p0, p1)
            r = sptr.Renderer(0)
            r.set_signed_distance(True)
            tb, bb = [], []
            for _ in range(a.reps + 1):
                r.upload_scene(flat)
                info = r.signed_info()
                tb.append(info["ms_build"])
                bb.append(r.scene_info()["build_ms"])
            print(json.dumps({"scene": f"{name} {p0} {p1}", "triangles": info["num_tris"], "table_build": stats(tb[1:]),
                              "bvh_build_ms": stats(bb[1:]), "table_bytes": info["table_bytes"],
                              **{k: info[k] for k in sptr._SIGNED_COUNTS}}), flush=True)
            r.close()
    if a.query or a.points:
        flat = sptr.builtin_scene("default_emitter", 0, 0)
        r = sptr.Renderer(0)
        r.set_signed_distance(a.query)
        r.upload_scene(flat)
        for k in (a.log2n if a.query else [21]):
            n = 1 << k
            pts = make_points(flat, "box", n)
            torch.cuda.synchronize()
            if a.query:
                out, walk, sign = None, [], []
                for i in range(a.reps + 1):
                    out = r.query_signed_distance(pts, sort=False, out=out, flip_triangles=True)
                    walk.append(r.point_query_info()["ms_walk"])
                    sign.append(r.signed_info()["ms_sign"])
                neg = int(torch.signbit(out["signed_dist"]).sum())
                print(json.dumps({"scene": "default_emitter", "set": "box", "log2n": k, "walk": stats(walk[1:]),
                                  "sign": stats(sign[1:]), "negative": neg}), flush=True)
            if a.points:
                out, walk = None, []
                for i in range(a.reps + 1):
                    out = r.query_points(pts, sort=False, out=out)
                    walk.append(r.point_query_info()["ms_walk"])
                print(json.dumps({"scene": "default_emitter", "set": "box", "log2n": k, "query_points_walk": stats(walk[1:])}),
                      flush=True)
            del pts, out
        r.close()


if __name__ == "__main__":
    main()
