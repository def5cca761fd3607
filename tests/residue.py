"""Full-size parity bound and residue classifier shared by the GPU suites (test infrastructure).

The GPU and the oracle agree bit for bit on most pixels of a full-size frame; the rest (a few dozen
of 2-8 M) differ by an ulp-level amount somewhere on a path.  `full_size_parity` bounds how many may
differ and checks that every one of them falls in a named class, each verified pixel by pixel against
the oracle re-rendering the pixel with the GPU's value of the suspected operation (oracle.device_math).
"""
import os

import numpy as np

import oracle

THREADS = min(16, os.cpu_count() or 1)
# about twice the differing pixels measured in r04-r05 (C3 2, C5 26 at 1080p; C4 50 at 4K x 16), and a
# relative L1 over an order above the measured <= 4e-7
MAX_DIFF_1080P, MAX_DIFF_4K, MAX_REL_L1_FULL = 64, 256, 1e-5

_SINCOS = {}


def log_parity(name, rec):
    """Measured fractions, printed and (SPTR_PARITY_LOG=<dir>) written as JSON for profiles/."""
    import json

    print(name, json.dumps(rec))
    d = os.environ.get("SPTR_PARITY_LOG")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"{name}.json"), "w") as f:
            json.dump(rec, f, indent=1)


def device_sincos(renderer):
    """The GPU's (sin, cos) of the cosine sample's phi for all 2^24 values of r1 (cached, 128 MB)."""
    if "tab" not in _SINCOS:
        _SINCOS["tab"] = renderer.cosine_sincos_table()
    return _SINCOS["tab"]


def resolve_device_gamma(renderer, sums, n):
    """The tile task's resolve (GLRenderer.cpp:411-431) of float32 sums, in float32 op for op, with the
    GPU's pow(c, 1/2.2): the RGB8 the GPU would show for these sums."""
    f = np.float32
    c = sums.astype(f) / f(n)
    c = np.clip((c * (f(2.51) * c + f(0.03))) / (c * (f(2.43) * c + f(0.59)) + f(0.14)), f(0), f(1))
    g = np.clip(renderer.gamma_pow(c), f(0), f(1))
    return (g * f(255)).astype(np.uint8)


def _path_tie(renderer, P, cam, W, H, S, mats, lts, env_faces, x, y):
    """(tie, record): the oracle's rays of pixel (x, y), all S samples, through both BVHs' queries."""
    kinds, rays = [], []
    for a in range(1, S + 1):
        k, r = P.path_rays(cam.as_array(), W, H, mats, lts, x, y, a, env_faces=env_faces)
        kinds.append(k)
        rays.append(r)
    k, r = np.concatenate(kinds), np.concatenate(rays)
    c, sh = r[k == 0], r[k == 1]
    g, pr, t, _ = renderer.intersect(c)
    og, opr, ot, _ = P.intersect(c)
    same_t = t.view(np.uint32) == ot.view(np.uint32)
    both_miss = (g == 0xFFFFFFFF) & (og == 0xFFFFFFFF)
    tie = int((((g != og) | (pr != opr)) & same_t & ~both_miss).sum()) if len(c) else 0
    other = int((~same_t & ~both_miss).sum()) if len(c) else 0
    occ = int((renderer.occluded(sh) != P.occluded(sh)).sum()) if len(sh) else 0
    return tie > 0, {"xy": (x, y), "closest_rays": int(len(c)), "ties": tie, "t_mismatch": other,
                     "shadow_rays": int(len(sh)), "occlusion_mismatch": occ}


def full_size_parity(name, renderer, P, cam, W, H, S, rgb, acc, orgb, oacc, tie_fn=None, env_faces=None,
                     lights=None, materials=None, log=print):
    """§8(c) at the timed size, bounded at the measured residue: at most MAX_DIFF_* differing RGB8 pixels
    and relative L1 <= MAX_REL_L1_FULL over every finite pixel; and every differing pixel is explained
    by one named class, checked pixel by pixel:
      resolve   — identical linear sums; the oracle's sums resolved with the GPU's pow(c, 1/2.2) give
                  the GPU's RGB8 (glibc vs ocml powf, GLRenderer.cpp:416-430);
      sincos    — the oracle re-rendering the pixel with the GPU's sin/cos of the cosine sample's phi
                  (wf_math.h:51-72) reproduces the GPU's sums bit for bit;
      pow_chain — ... with, in addition, the GPU's double squaring chains for pow(x, 5 / 8 / 64)
                  (Material.cpp:32-117's Schlick term, EnvironmentManager.cpp:35-61's sun lobes);
      bvh_tie   — replaying the oracle path's rays (every sample's closest-hit and shadow rays, in trace
                  order) through the GPU's and the oracle's queries finds a closest hit at the same t on
                  another primitive (the two BVHs are built apart, so a tie may resolve either way;
                  a shared cube edge), or tie_fn(ys, xs) holds (the 10M-triangle mesh: a camera sample's
                  first hit on a pole fan row, either side).
    Nothing may be left unexplained.  materials / lights default to the presets and the sun."""
    exact = (rgb == orgb).all(axis=2)
    gfin, ofin = np.isfinite(acc).all(axis=2), np.isfinite(oacc).all(axis=2)
    assert np.array_equal(gfin, ofin), "non-finite masks differ"
    assert (~gfin).sum() <= max(3, 1e-6 * W * H), "non-finite pixels"
    fin = gfin
    rel_all = float(np.abs(acc[fin] - oacc[fin]).sum() / max(1e-12, np.abs(oacc[fin]).sum()))
    rec = {"pixels": W * H, "spp": S, "exact_all": float(exact.mean()), "rel_l1_all": rel_all,
           "differing_pixels": int((~exact).sum())}
    ys, xs = np.nonzero(~exact & fin)
    cls = {"resolve": 0, "sincos": 0, "pow_chain": 0, "bvh_tie": 0, "unexplained": 0}
    if len(ys):
        u32 = np.uint32
        g_sum, o_sum = acc[ys, xs], oacc[ys, xs]
        same_lin = (g_sum.view(u32) == o_sum.view(u32)).all(axis=1)
        resolve = same_lin & (resolve_device_gamma(renderer, o_sum, S) == rgb[ys, xs]).all(axis=1)
        ps = (ys * W + xs).astype(np.uint32)
        mats = oracle.preset_materials(False) if materials is None else materials
        lts = oracle.default_lights() if lights is None else lights
        tab = device_sincos(renderer)
        matched = {}
        for key, chains in (("sincos", False), ("pow_chain", True)):
            with oracle.device_math(tab, pow_chains=chains):
                dacc, _, _ = P.render(cam.as_array(), W, H, mats, lts, frames=S, threads=THREADS, env_faces=env_faces,
                                      pixels=ps)
            matched[key] = (dacc[ys, xs].view(u32) == g_sum.view(u32)).all(axis=1)
        sincos = ~resolve & matched["sincos"]
        powc = ~resolve & ~sincos & matched["pow_chain"]
        tie = np.zeros(len(ys), bool) if tie_fn is None else np.asarray(tie_fn(ys, xs), bool)
        tie &= ~(resolve | sincos | powc)
        for i in np.nonzero(~(resolve | sincos | powc | tie))[0]:
            tie[i], why = _path_tie(renderer, P, cam, W, H, S, mats, lts, env_faces, int(xs[i]), int(ys[i]))
            if why:
                rec.setdefault("path_checks", []).append(why)
        rest = ~(resolve | sincos | powc | tie)
        cls = {"resolve": int(resolve.sum()), "sincos": int(sincos.sum()), "pow_chain": int(powc.sum()),
               "bvh_tie": int(tie.sum()), "unexplained": int(rest.sum())}
        if rest.any():
            rec["unexplained_xy"] = [(int(x), int(y)) for x, y in zip(xs[rest], ys[rest])][:16]
    rec["classes"] = cls
    log(name, rec)
    limit = MAX_DIFF_4K if W * H > 1920 * 1080 else MAX_DIFF_1080P
    assert rec["differing_pixels"] <= limit, rec
    assert rel_all <= MAX_REL_L1_FULL, rec
    assert cls["unexplained"] == 0, rec
    return rec
