#!/usr/bin/env python3
"""Ray-render measurement: sptr_render_rays with device pointers against the same frame as a
1-spp sptr_render.

Scenes: C2's (default_emitter, staged into LDS) and C5's (the 10M-triangle sphere mesh, walked from HBM).  The
rays are the 1920x1080 primary rays of the default camera at accumulation index 1 (sptr_primary_rays), held in
device tensors, without seeds (ray i then draws what pixel i draws), at depth 6 and 1 sample.  Per scene both
shapes are warmed up, then the ray call and the render call (launch mode 0, frame_begin 1) alternate inside
this one process, --reps times each.  Reported: the device times of the ray calls (sptr_ray_render_info: events
around the chunks' launches) and of the render calls (sptr_stats.ms_total), the median and spread (max - min)
of each, their ratio, the query counts of both, and whether the ray call's radiance equals the frame's
accumulation bit for bit.  The ray path carries no cull and no fused launches and writes 32 B more per ray, so
a ratio above 1 is expected.  There is no CPU fallback: without a GPU the Renderer raises."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="c2,c5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=6)
    a = ap.parse_args()
    rows = []
    for name in a.scenes.split(","):
        wl = workloads.WORKLOADS[name]
        r = sptr.Renderer(0)
        workloads.setup(r, wl)
        r.set_launch_mode(0)
        lay = r.scene_layout()
        print(f"# scene {name}: {lay['num_tris']} triangles, {lay['num_spheres']} spheres, BVH{lay['bvh_width']}, "
              f"lds_bytes {lay['lds_bytes']}", flush=True)
        cam = sptr.camera_lookat(aspect=W / H)
        dirs, _ = r.primary_rays(cam, W, H, 1)
        host = np.zeros((W * H, 8), np.float32)
        host[:, 0:3] = cam.as_array()[:3]
        host[:, 3:6] = dirs.reshape(-1, 3)
        rays = torch.from_numpy(host).to(DEV).contiguous()
        out = torch.empty((W * H, 3), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        # warm-up of both shapes (the render first: the ray path then takes the wave buffers it allocated)
        st = r.render(cam, W, H, spp=1, max_depth=a.depth)
        frame = r.read_accum().reshape(-1, 3)
        r.render_rays(rays, max_depth=a.depth, out=out)
        info = r.ray_render_info()
        equal = bool(np.array_equal(out.cpu().numpy().view(np.uint32), frame.view(np.uint32)))
        ms_rays, ms_frame = [], []
        for _ in range(a.reps):
            r.render_rays(rays, max_depth=a.depth, out=out)
            info = r.ray_render_info()
            ms_rays.append(info["ms"])
            st = r.render(cam, W, H, spp=1, max_depth=a.depth)
            ms_frame.append(st.ms_total)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        row = {"scene": name, "rays": W * H, "depth": a.depth, "chunks": info["chunks"],
               "ms_render_rays": [round(x, 4) for x in ms_rays], "ms_render_rays_median": round(med(ms_rays), 4),
               "ms_render_rays_spread": round(max(ms_rays) - min(ms_rays), 4),
               "ms_render": [round(x, 4) for x in ms_frame], "ms_render_median": round(med(ms_frame), 4),
               "ms_render_spread": round(max(ms_frame) - min(ms_frame), 4),
               "ratio": round(med(ms_rays) / med(ms_frame), 3) if med(ms_frame) > 0 else None,
               "queries_render_rays": [info["closest"], info["shadow"]],
               "queries_render": [int(st.rays_closest), int(st.rays_shadow)],
               "radiance_equals_accum": equal}
        rows.append(row)
        print(json.dumps(row), flush=True)
        r.close()
    print("# scene | render_rays ms median (spread) | render ms median (spread) | ratio | equal")
    for x in rows:
        print(f"{x['scene']} | {x['ms_render_rays_median']:.3f} ({x['ms_render_rays_spread']:.3f}) | "
              f"{x['ms_render_median']:.3f} ({x['ms_render_spread']:.3f}) | {x['ratio']} | {x['radiance_equals_accum']}")


if __name__ == "__main__":
    main()
