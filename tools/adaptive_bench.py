#!/usr/bin/env python3
"""Adaptive-sampling measurement: sptr_render_adaptive against sptr_render at equal error.

Scenes: C2's (default_emitter) and C4's (default), both at 1920x1080, depth 6.
  baseline  : sptr_render, 64 spp, launch mode 0 (device ms: sptr_stats.ms_total);
  candidate : render_adaptive, max 64, min 16, step 16 (device ms: sptr_adaptive_info.ms, first launch to last,
              which includes the host's read of the selection words between passes);
  reference : a uniform 1024-spp accumulation under a seed offset of 2^20, so that neither image shares a sample
              with it.
Error of an image: relative L1 of its linear per-pixel mean (S / n) against the reference's mean,
sum |m - ref| / sum |ref|, over the pixels finite in both (the reference's non-finite pixels are counted and printed).
Thresholds: a sweep from coarse to fine (untimed) gives every threshold's error; the first threshold whose error is
within --match (default 2 %) of the uniform 64-spp image's "matches" it, and that threshold with its two neighbours
in the sweep is the bracket that is timed.  Both variants are warmed up, then baseline and the three candidates
alternate inside this one process, --reps times each; printed are every repetition, the median and the spread
(max - min), the wall-clock ms of the same calls, the mean samples per pixel, the fraction of pixels active in each
pass (from the count map: a pixel is active in pass k > 1 iff it ends with at least min + (k - 1) step samples) and
the errors.  There is no CPU fallback: without a GPU the Renderer raises."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-path-tracer_amd"))
import sptr  # noqa: E402

W, H, DEPTH = 1920, 1080, 6
SPP, MIN, STEP = 64, 16, 16
SWEEP = (0.32, 0.16, 0.08, 0.04, 0.02, 0.01, 0.005, 0.0025, 0.00125, 0.0)
REF_SPP, REF_OFFSET = 1024, 1 << 20


def rel_l1(mean, ref):
    """Over the pixels that are finite in both images (a path may return a non-finite radiance)."""
    m = mean.astype(np.float64)
    ok = np.isfinite(ref).all(axis=2) & np.isfinite(m).all(axis=2)
    return float(np.abs(m[ok] - ref[ok]).sum() / np.abs(ref[ok]).sum())


def adaptive(r, cam, thr):
    t0 = time.perf_counter()
    info = r.render_adaptive(cam, W, H, thr, MIN, SPP, STEP, max_depth=DEPTH)
    info["wall_ms"] = (time.perf_counter() - t0) * 1e3
    return info


def uniform(r, cam):
    t0 = time.perf_counter()
    st = r.render(cam, W, H, spp=SPP, max_depth=DEPTH)
    return {"ms": st.ms_total, "wall_ms": (time.perf_counter() - t0) * 1e3}


def adaptive_mean(r):
    n = r.read_sample_counts()
    return r.read_accum() / n[..., None].astype(np.float32), n


def med(v):
    return f"median {statistics.median(v):.3f} spread {max(v) - min(v):.3f} [{' '.join(f'{x:.3f}' for x in v)}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="default_emitter,default")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--match", type=float, default=0.02)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"adaptive_bench: {W}x{H} depth {DEPTH}; baseline sptr_render {SPP} spp (launch mode 0); candidate render_adaptive "
        f"min {MIN} max {SPP} step {STEP}; reference {REF_SPP} spp under seed offset {REF_OFFSET}; reps {a.reps}")
    r = sptr.Renderer(0)
    r.set_launch_mode(0)
    cam = sptr.camera_lookat(aspect=W / H)
    for scene in a.scenes.split(","):
        say()
        say(f"== scene {scene} ({'C2' if scene == 'default_emitter' else 'C4'} scene)")
        sptr.setup_default(r, scene)
        r.set_seed_offset(REF_OFFSET)
        r.render(cam, W, H, spp=REF_SPP, max_depth=DEPTH)
        ref = r.read_accum().astype(np.float64) / REF_SPP
        r.set_seed_offset(0)
        say(f"reference: {int((~np.isfinite(ref).all(axis=2)).sum())} of {W * H} pixels are not finite and are left out")
        uniform(r, cam)
        e_uni = rel_l1(r.read_accum() / np.float32(SPP), ref)
        say(f"uniform {SPP} spp: relL1 {e_uni:.6f}")
        errs = []
        for thr in SWEEP:
            info = adaptive(r, cam, thr)
            m, n = adaptive_mean(r)
            errs.append(rel_l1(m, ref))
            say(f"sweep threshold {thr:<8g} relL1 {errs[-1]:.6f} ({errs[-1] / e_uni:.3f} x uniform)  mean spp {n.mean():.2f}  "
                f"passes {info['passes']}  ms {info['ms']:.3f}")
        k = next(i for i, e in enumerate(errs) if e <= e_uni * (1.0 + a.match))
        lo = max(0, min(k - 1, len(SWEEP) - 3))
        bracket = SWEEP[lo:lo + 3]
        say(f"first threshold within {a.match:.0%} of the uniform error: {SWEEP[k]:g}; timed bracket {bracket}")
        for thr in bracket:  # warm-up of every shape
            adaptive(r, cam, thr)
        uniform(r, cam)
        t_uni, w_uni = [], []
        t_ad = {thr: [] for thr in bracket}
        w_ad = {thr: [] for thr in bracket}
        shape = {}
        for _ in range(a.reps):
            u = uniform(r, cam)
            t_uni.append(u["ms"])
            w_uni.append(u["wall_ms"])
            for thr in bracket:
                info = adaptive(r, cam, thr)
                t_ad[thr].append(info["ms"])
                w_ad[thr].append(info["wall_ms"])
                if thr not in shape:
                    m, n = adaptive_mean(r)
                    passes = info["passes"]
                    frac = [1.0] + [float((n >= MIN + (p - 1) * STEP).mean()) for p in range(2, passes + 1)]
                    shape[thr] = (rel_l1(m, ref), float(n.mean()), frac, info)
        say(f"baseline  uniform {SPP} spp          device ms {med(t_uni)}")
        say(f"                                    wall ms   {med(w_uni)}   relL1 {e_uni:.6f}  mean spp {SPP:.2f}")
        for thr in bracket:
            e, spp, frac, info = shape[thr]
            say(f"candidate threshold {thr:<8g}       device ms {med(t_ad[thr])}")
            say(f"                                    wall ms   {med(w_ad[thr])}   relL1 {e:.6f} ({e / e_uni:.3f} x uniform)  "
                f"mean spp {spp:.2f}")
            say(f"                                    active fraction per pass {' '.join(f'{f:.3f}' for f in frac)}; passes "
                f"{info['passes']} chunks {info['chunks']} rays {info['rays_closest']}+{info['rays_shadow']}; "
                f"speed-up over the baseline (device medians) {statistics.median(t_uni) / statistics.median(t_ad[thr]):.3f}")
    r.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
