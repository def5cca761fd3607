"""A float64 model of the wavefront path's scatter step, in numpy only: what continue_path and the emission line
(csrc/kernels_wavefront.hip) and the oracle's trace_path (oracle/wf_oracle.cpp) are both held to.

Written from the formulas of WavefrontPathTracerCPU::traceRay (wf_pt_cpu.cpp:61-255), wf_math.h:35-100 and
Material::isTransparent / getTransparency (Material.h:62-73), not from either restatement.  Scenes are analytic:
rectangles (a corner p and two orthogonal edge vectors u, v; normal cross(u, v)) and spheres (centre, radius), each
with a material row (albedo3 metallic roughness emission3 ior ...); no BVH, no lights (they never steer a path, and
tests/light_ref.py holds their term).  Per bounce, for bounce = 0 .. max_depth - 1 (wf_pt_cpu.cpp:94-248):

  nearest hit with t > 0; none: rad += thr * env(direction), the path ends        (wf_pt_cpu.cpp:98-103)
  P = o + t d;  n = unit normal, negated when dot(n, d) > 0                        (:106-116)
  rad += thr * emission when the emission is not black                             (:121-124)
  metallic > 0.5:  d' = reflect(d, n) = d - 2 dot(n, d) n, thr *= albedo * metallic, o' = P + 1e-4 n   (:151-164)
  metallic < 0.1 and ior > 1.3 (Material.h:62-65):                                 (:166-222)
      cosine = -dot(d, n) (>= 0 after the face-forwarding, so eta = 1 / ior on inside hits too)
      tr = clamp((ior - 1) / 0.7f, 0, 0.95f);  r0 = ((1 - ior) / (1 + ior))^2
      F = r0 + (1 - r0) (1 - clamp(|cosine|, 0, 1))^5;  xi = rand01
      xi < F:  reflect, thr *= 1 - tr, o' = P + 1e-4 n
      else     k = 1 - eta^2 (1 - cosine^2);  k < 0: reflect, thr unchanged, o' = P + 1e-4 n
               else d' = eta d + (eta cosine - sqrt(k)) n, thr *= tr, o' = P - 1e-4 n
  otherwise (diffuse):                                                             (:225-247, wf_math.h:51-72)
      r1 = rand01, r2 = rand01;  phi = 2 pi_f r1;  x = sqrt(r2) cos(phi), y = sqrt(r2) sin(phi), z = sqrt(max(0, 1 - r2))
      t = normalize(cross(n, (0, 0, 1))) when |n.z| < 0.999f, else normalize(cross(n, (0, 1, 0)));  b = cross(t, n)
      d' = normalize(t x + b y + n z);  xi = rand01;  s = max(albedo)
      bounce > 2:  xi >= s ends the path, else thr *= albedo / max(s, 1e-6);   bounce <= 2: thr *= albedo
      o' = P + 1e-4 n
  rand01: state = wang_hash(state), (state & 0xFFFFFF) / 2^24                      (wf_math.h:35-49)

float32 constants of the source (0.7f, 0.95f, 0.999f, pi_f, 1e-4f, 1e-6f) enter as their float32 values; materials
are float32 inputs.  Everything else is float64.

trace() returns per ray the radiance, the number of segments traced, the branch record and a `fragile` flag: a path
is fragile when a float32 evaluation could decide differently from float64, namely
  - a hit, or a pass beside a rectangle, within BORDER of the rectangle's edge, or a ray passing within BORDER of a
    sphere's silhouette, no farther along the ray than the hit taken (as env_common.mirror_paths does); a crossing of a
    rectangle or a sphere with |t| < T_MIN;
  - a hit whose computed point may lie more than P_MARGIN (a quarter of the 1e-4 offset) off the surface along the
    normal, so that the next ray could start on the wrong side: 4 eps (|o| + t) for a rectangle, and for a sphere
    (3 L + 8 L^2 / h) eps h / r, the error of t derived below times the cosine of incidence;
  - |xi - F| < F_MARGIN + 5 (e_d + e_n) eps (dF / dcos <= 5);
  - ||n.z| - 0.999f| < NZ_MARGIN + e_n eps;
  - a final direction whose two largest components are within SEAM_MARGIN + 2 e_d eps of each other (relative): the
    cubemap lookup would take another face.
The roulette compare is exact on both sides (xi is k / 2^24, s is a float32 input, and float32 >= float32 is float64
>= float64), so it is never fragile.

Tolerance.  eps = 2^-24.  e_d is a bound on the Euclidean error of the float32 unit direction, e_n that of the
unit normal, both in units of eps; a perturbation e of a unit direction moves the cubemap's u by at most
sqrt(3) e (|d(uc / ma)| <= 2 e / ma, ma >= 1 / sqrt(3), halved), so the lookup is asked for

  du = env_ref.DU_DIRECT + 2 e_d eps

and tol = thr * lookup_bound(du) + REL eps * radiance.  e_d starts at E_PRIMARY = 4 (a unit float32 direction
renormalised by another correctly rounded sequence: <= 2 eps per renormalisation).  Per scatter kind:

  plane normal     E_PLANE = 16: cross of two float32 edge vectors at right angles, each component within 6 eps of
                   |u||v| (two products, one difference, the edge subtractions), so 6 sqrt(3) < 11 on the unit
                   vector, plus 4 for its normalisation, rounded up.
  sphere normal    (first segment only, the origin exact)  n = (P - c) / r with P = o + t d.  With L = |o - c| and
                   h = sqrt(disc) = r cos(incidence): the discriminant b^2 - 4 a c carries <= 16 eps L^2 (b, a, c
                   each a rounded sum of three products of magnitudes <= L^2), so t carries 3 L + 8 L^2 / h; the
                   incoming e_d moves P by t e_d across the ray and by t e_d r / h along it; the sums forming P and
                   P - c carry 4 (|o| + |c| + r).  e_n = (3 L + 8 L^2 / h + t e_d (1 + r / h) + 4 (|o| + |c| + r))
                   / r + 2: it grows with |P| / r and towards the silhouette.
  reflect          d - 2 dot(n, d) n is an isometry in d and moves by <= 4 |dn|; the dot (3 eps), two products and a
                   difference per component (<= 10 eps each, 18 on the vector), safe_normalize (4), rounded up:
                   e_d' = e_d + 4 e_n + 24.
  refract          eta = 1 / ior < 0.77 and k >= 1 - eta^2 > 0.4: |d sqrt(k)| <= eta^2 |dcos| / sqrt(k) < |dcos|,
                   |dcos| <= e_d + e_n, |eta cos - sqrt(k)| <= 1, so the exact map moves by <= eta e_d +
                   (1 + eta) (e_d + e_n) + e_n < 3 e_d + 3 e_n; roundings: eta 1, cos 3, k 6, sqrt 6, coefficient 12,
                   16 per component (28 on the vector), safe_normalize 4, rounded up: e_d' = 3 e_d + 3 e_n + 40.
  cosine sample    does not depend on d.  n' = safe_normalize(n): e_n + 4.  t = normalize(cross(n', axis)) divides by
                   s = sqrt(n.x^2 + n.y^2) >= 0.044 on the z branch and by sqrt(n.x^2 + n.z^2) >= 0.999 on the y
                   branch: e_t = (e_n + 4) / s + 4;  e_b = e_t + e_n + 10.  phi = 2 pi_f r1 carries 2 pi eps < 7, the
                   library's sin and cos 4 ulp <= 4 eps (the OpenCL bound; glibc's is 1 ulp), the products with
                   sqrt(r2) 2 more: x, y within 13 eps, z within 1.  t x + b y + n' z then moves by <= e_t + e_b +
                   e_n + 4 + 27, its three products and two sums 9 per component (16), two safe_normalize 8:
                   e_d' = 2 e_t + 2 e_n + 72.
  REL              the relative error of thr and of the sums, in eps, added over the path's bounces: 4 per mirror,
                   refraction or diffuse bounce (the factor's own rounding <= 2, the product 1, an emission product
                   and sum 1), 48 per Fresnel reflection (1 - tr with tr within 2 eps of a value <= 0.95: 2 eps on
                   >= 0.05 is 40 eps relative), plus 4 for the final product and sum.

Where a term is not derived, that is after a sphere is hit from an origin that is itself a computed point (a position
error carried into the normal), the ray is marked `underived` and trace() takes du from the caller:
needed_du() gives the smallest du that covers a given output on those rays, and the tests grant 4 x the oracle's
worst needed du on the CPU for that set, not below 16 eps (the rule of tests/test_gpu_light_parity.py).  The
fragile margins of such a ray take e_d = e_n = E_UNDERIVED = 1024 (6e-5: the largest du the oracle needs on such
rays, about 2000 eps, is 2 e_d eps at e_d of about 1000); its tolerance does not depend on that figure.
"""
import numpy as np

import env_ref

f32, f64, u32 = np.float32, np.float64, np.uint32
EPS = 2.0 ** -24
BORDER = 1e-3
T_MIN = 2e-5
P_MARGIN = 2.5e-5
F_MARGIN = 1e-6
NZ_MARGIN = 1e-5
SEAM_MARGIN = 1e-5
E_PRIMARY = 4.0
E_PLANE = 16.0
E_UNDERIVED = 1024.0
DU_FLOOR = 16 * EPS
C_07, C_095, C_0999, C_PI, C_OFF, C_TINY = (f64(f32(v)) for v in (0.7, 0.95, 0.999, np.pi, 1e-4, 1e-6))

NONE, MIRROR, FRESNEL, REFRACT, TIR, DIFFUSE_Z, DIFFUSE_Y = range(7)  # the branch record's `kind`
KIND_NAMES = ("none", "mirror", "fresnel_reflect", "refract", "tir", "diffuse_z", "diffuse_y")
RR_NONE, RR_SURVIVE, RR_KILL = range(3)

MUTANTS = ("sincos_swapped", "b_is_cross_n_t", "onb_never_switched", "sqrt_swapped", "xi_first", "roulette_from_2",
           "roulette_no_division", "eta_is_ior", "schlick_x4", "tr_unclamped", "refract_origin_plus",
           "fresnel_reflect_times_tr", "metal_albedo_only", "emission_after", "no_face_forward")


def wang_hash(a):
    """wang_hash (wf_math.h:35-43) in uint32 numpy arithmetic."""
    a = np.asarray(a, u32).copy()
    with np.errstate(over="ignore"):
        a = (a ^ u32(61)) ^ (a >> u32(16))
        a = a * u32(9)
        a = a ^ (a >> u32(4))
        a = a * u32(0x27D4EB2D)
        a = a ^ (a >> u32(15))
    return a


def rand01(state):
    """default_rand01 (wf_math.h:45-49): (the new state, the value) for an array of states."""
    s = wang_hash(state)
    return s, (s & u32(0x00FFFFFF)).astype(f64) / 16777216.0


def _dot(a, b):
    return (a * b).sum(axis=1)


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(_dot(v, v))[:, None]


def _intersect(scene, o, d, alive, e_d, border):
    """Nearest hit with t > 0 of every live ray: (hit, t, unit normal, material, sphere?, sphere terms, fragile)."""
    n = len(o)
    best_t = np.full(n, np.inf)
    best_n = np.zeros((n, 3))
    best_m = np.full(n, -1)
    best_s = np.zeros(n, bool)
    sph_en = np.zeros(n)        # the derived e_n of a sphere hit (for an exact origin)
    near_t = np.full(n, np.inf)  # the nearest crossing within `border` of an edge or a silhouette
    tiny = np.zeros(n, bool)
    risky = np.zeros(n, bool)    # the hit taken may be computed more than P_MARGIN off its surface
    with np.errstate(divide="ignore", invalid="ignore"):
        for p, u, v, mat in scene["rects"]:
            p, u, v = (np.asarray(a, f64) for a in (p, u, v))
            assert abs(u @ v) <= 1e-12 * np.sqrt((u @ u) * (v @ v))
            nr = np.cross(u, v)
            den = d @ nr
            t = ((p - o) @ nr) / den
            ok = alive & np.isfinite(t) & (t > 0)
            q = o + t[:, None] * d - p
            a, b = (q @ u) / (u @ u), (q @ v) / (v @ v)
            margin = np.minimum(np.minimum(a, 1 - a) * np.sqrt(u @ u), np.minimum(b, 1 - b) * np.sqrt(v @ v))
            tiny |= alive & np.isfinite(t) & (np.abs(t) < T_MIN) & (margin > -border)
            hit = ok & (margin > 0) & (t < best_t)
            best_t = np.where(hit, t, best_t)
            risky = np.where(hit, 4 * EPS * (np.sqrt(_dot(o, o)) + t) > P_MARGIN, risky)
            best_n[hit] = nr / np.sqrt(nr @ nr)
            best_m = np.where(hit, mat, best_m)
            best_s &= ~hit
            near_t = np.where(ok & (np.abs(margin) < border), np.minimum(near_t, t), near_t)
        for c, r, mat in scene["spheres"]:
            c = np.asarray(c, f64)
            oc = o - c
            b = _dot(oc, d)
            L2 = _dot(oc, oc)
            disc = b * b - (L2 - r * r)
            h = np.sqrt(np.maximum(disc, 0.0))
            t1, t2 = -b - h, -b + h
            t = np.where(t1 > 0, t1, t2)
            ok = alive & (disc >= 0) & (t > 0)
            tiny |= alive & (disc >= 0) & ((np.abs(t1) < T_MIN) | (np.abs(t2) < T_MIN))
            hit = ok & (t < best_t)
            best_t = np.where(hit, t, best_t)
            P = o + t[:, None] * d
            best_n[hit] = ((P - c) / r)[hit]
            best_m = np.where(hit, mat, best_m)
            best_s |= hit
            L = np.sqrt(L2)
            en = (3 * L + 8 * L2 / h + t * e_d * (1 + r / h) + 4 * (np.sqrt(_dot(o, o)) + np.sqrt(c @ c) + r)) / r + 2
            sph_en = np.where(hit, en, sph_en)
            risky = np.where(hit, (3 * L + 8 * L2 / h) * EPS * (h / r) > P_MARGIN, risky)
            # the silhouette: the ray's line passes within `border` of the sphere's surface, ahead of the origin
            dist = np.sqrt(np.maximum(L2 - b * b, 0.0))
            close = alive & (np.abs(dist - r) < border) & (-b > 0)
            near_t = np.where(close, np.minimum(near_t, np.maximum(t1, 0.0)), near_t)
    hit = alive & (best_m >= 0)
    fragile = alive & ((np.isfinite(near_t) & (near_t <= best_t)) | tiny | risky)
    return hit, best_t, best_n, best_m, best_s, sph_en, fragile


def trace(scene, origins, dirs, states, env, max_depth, mutant=None, du_underived=None, border=BORDER):
    """The paths of rays (origins (3,) or (n, 3), float32 unit dirs (n, 3), rng states (n,) uint32) through `scene`
    ({"rects": [(p, u, v, material)], "spheres": [(c, r, material)], "materials": (m, 12) float32}) under
    env = (faces, intensity, max_clamp).

    Returns a dict: value (n, 3) and tol (n, 3) float64, segments (n,) the closest-hit queries of each path,
    fragile (n,), underived (n,) (tol there takes du_underived, or is inf without one), and the record per bounce
    (n, max_depth): kind, back (a back-side hit), emit (emission added), rr (roulette: none / survive / kill);
    env_scale (n, 3) and rel (n,) are what needed_du() works from.  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    faces, intensity, max_clamp = env
    d = np.asarray(dirs, f64).reshape(-1, 3)
    n = len(d)
    d = _unit(d)
    o = np.broadcast_to(np.asarray(origins, f64), (n, 3)).copy()
    state = np.asarray(states, u32).reshape(n).copy()
    mats = np.asarray(scene["materials"], f32).astype(f64)
    thr, rad = np.ones((n, 3)), np.zeros((n, 3))
    tol_env, env_scale = np.zeros((n, 3)), np.zeros((n, 3))
    e_d, rel = np.full(n, E_PRIMARY), np.full(n, 4.0)
    alive = np.ones(n, bool)
    fragile, underived = np.zeros(n, bool), np.zeros(n, bool)
    exact_origin = np.ones(n, bool)
    segments = np.zeros(n, np.int64)
    kind = np.zeros((n, max_depth), np.int8)
    back, emit = np.zeros((n, max_depth), bool), np.zeros((n, max_depth), bool)
    rr = np.zeros((n, max_depth), np.int8)
    stats = env_ref.map_stats(faces)
    S = np.asarray(faces).shape[1]

    def lookup_bound(du):
        with np.errstate(invalid="ignore"):
            return abs(f64(intensity)) * (2.0 * ((S - 1) * (du + EPS))[:, None] * stats[0][None, :] + 16 * EPS * stats[1][None, :])

    for bounce in range(max_depth):
        if not alive.any():
            break
        segments += alive
        hit, t, nrm, mi, is_sphere, sph_en, frag = _intersect(scene, o, d, alive, e_d, border)
        fragile |= frag
        miss = alive & ~hit
        if miss.any():
            dm = d[miss]
            bad = ~np.isfinite(dm).all(axis=1)  # (a mutant's degenerate basis)
            val, _, _ = env_ref.lookup(np.where(bad[:, None], (1.0, 0.0, 0.0), dm), faces, intensity, max_clamp, stats=stats)
            rad[miss] += thr[miss] * np.where(bad[:, None], np.nan, val)
            a = np.sort(np.abs(d[miss]), axis=1)
            seam = a[:, 1] >= a[:, 2] * (1.0 - SEAM_MARGIN - 2 * e_d[miss] * EPS)
            fragile[np.flatnonzero(miss)[seam]] = True
            du = env_ref.DU_DIRECT + 2 * e_d * EPS
            if du_underived is not None:
                du = np.where(underived, du_underived, du)
            tol_env[miss] = (thr * lookup_bound(du))[miss]
            env_scale[miss] = thr[miss]
        alive = hit
        if not alive.any():
            break
        underived |= alive & is_sphere & ~exact_origin
        e_n = np.where(underived, E_UNDERIVED, np.where(is_sphere, sph_en, E_PLANE))
        e_d = np.where(underived, E_UNDERIVED, e_d)
        m = mats[np.where(alive, mi, 0)]
        albedo, metallic, emission, ior = m[:, 0:3], m[:, 3], m[:, 5:8], m[:, 8]
        P = o + t[:, None] * d
        is_back = _dot(nrm, d) > 0
        back[:, bounce] = alive & is_back
        if mutant != "no_face_forward":
            nrm = np.where(is_back[:, None], -nrm, nrm)
        emits = alive & ((emission * emission).sum(axis=1) > 0)
        emit[:, bounce] = emits
        if mutant != "emission_after":
            rad[emits] += (thr * emission)[emits]

        is_metal = alive & (metallic > 0.5)
        is_glass = alive & ~is_metal & (metallic < f64(f32(0.1))) & (ior > f64(f32(1.3)))
        is_diff = alive & ~is_metal & ~is_glass
        cosi = -_dot(d, nrm)
        refl = _unit(d + 2.0 * cosi[:, None] * nrm)
        new_d, sign = d.copy(), np.ones(n)
        new_thr, new_e, k_now = thr.copy(), e_d.copy(), np.zeros(n, np.int8)
        killed = np.zeros(n, bool)

        # metal
        new_d[is_metal] = refl[is_metal]
        f = albedo if mutant == "metal_albedo_only" else albedo * metallic[:, None]
        new_thr[is_metal] = (thr * f)[is_metal]
        new_e[is_metal] = (e_d + 4 * e_n + 24)[is_metal]
        k_now[is_metal] = MIRROR
        rel[is_metal] += 4

        # glass
        if is_glass.any():
            eta = ior if mutant == "eta_is_ior" else 1.0 / ior
            tr = (ior - 1.0) / C_07
            if mutant != "tr_unclamped":
                tr = np.clip(tr, 0.0, C_095)
            r0 = ((1.0 - ior) / (1.0 + ior)) ** 2
            x = 1.0 - np.clip(np.abs(cosi), 0.0, 1.0)
            F = r0 + (1.0 - r0) * x ** (4 if mutant == "schlick_x4" else 5)
            state_g, xi = rand01(state)
            state = np.where(is_glass, state_g, state)
            fragile |= is_glass & (np.abs(xi - F) < F_MARGIN + 5 * (e_d + e_n) * EPS)
            fres = is_glass & (xi < F)
            kk = 1.0 - eta * eta * (1.0 - cosi * cosi)
            tir = is_glass & ~fres & (kk < 0)
            refr = is_glass & ~fres & ~tir
            rdir = _unit(eta[:, None] * d + (eta * cosi - np.sqrt(np.maximum(kk, 0.0)))[:, None] * nrm)
            new_d[fres | tir] = refl[fres | tir]
            new_d[refr] = rdir[refr]
            new_thr[fres] = (thr * (tr if mutant == "fresnel_reflect_times_tr" else 1.0 - tr)[:, None])[fres]
            new_thr[refr] = (thr * tr[:, None])[refr]
            if mutant != "refract_origin_plus":
                sign[refr] = -1.0
            new_e[fres | tir] = (e_d + 4 * e_n + 24)[fres | tir]
            new_e[refr] = (3 * e_d + 3 * e_n + 40)[refr]
            k_now[fres], k_now[tir], k_now[refr] = FRESNEL, TIR, REFRACT
            rel[fres] += 48
            rel[refr | tir] += 4

        # diffuse
        if is_diff.any():
            s = state
            if mutant == "xi_first":
                s, xi = rand01(s)
            s, r1 = rand01(s)
            s, r2 = rand01(s)
            if mutant != "xi_first":
                s, xi = rand01(s)
            state = np.where(is_diff, s, state)
            phi = 2.0 * C_PI * r1
            cphi, sphi = np.cos(phi), np.sin(phi)
            if mutant == "sincos_swapped":
                cphi, sphi = sphi, cphi
            ra, z = np.sqrt(r2), np.sqrt(np.maximum(0.0, 1.0 - r2))
            if mutant == "sqrt_swapped":
                ra, z = z, ra
            x, y = ra * cphi, ra * sphi
            z_branch = np.abs(nrm[:, 2]) < C_0999
            fragile |= is_diff & (np.abs(np.abs(nrm[:, 2]) - C_0999) < NZ_MARGIN + e_n * EPS)
            if mutant == "onb_never_switched":
                z_branch = np.ones(n, bool)
            tz = np.stack([nrm[:, 1], -nrm[:, 0], np.zeros(n)], axis=1)   # cross(n, (0, 0, 1))
            ty = np.stack([-nrm[:, 2], np.zeros(n), nrm[:, 0]], axis=1)   # cross(n, (0, 1, 0))
            tv = np.where(z_branch[:, None], tz, ty)
            sl = np.sqrt(_dot(tv, tv))
            tv = _unit(tv)
            bv = np.cross(nrm, tv) if mutant == "b_is_cross_n_t" else np.cross(tv, nrm)
            out = _unit(tv * x[:, None] + bv * y[:, None] + nrm * z[:, None])
            new_d[is_diff] = out[is_diff]
            with np.errstate(divide="ignore"):
                e_t = (e_n + 4) / sl + 4
            new_e[is_diff] = (2 * e_t + 2 * e_n + 72)[is_diff]
            k_now[is_diff] = np.where(z_branch, DIFFUSE_Z, DIFFUSE_Y)[is_diff]
            surv = albedo.max(axis=1)
            roulette = is_diff & (bounce > (1 if mutant == "roulette_from_2" else 2))
            killed = roulette & (xi >= surv)
            lives = roulette & ~killed
            div = 1.0 if mutant == "roulette_no_division" else np.maximum(surv, C_TINY)[:, None]
            new_thr[is_diff] = np.where(lives[:, None], thr * albedo / div, thr * albedo)[is_diff]
            rr[:, bounce] = np.where(killed, RR_KILL, np.where(lives, RR_SURVIVE, RR_NONE))
            rel[is_diff] += 4

        kind[:, bounce] = np.where(alive, k_now, NONE)
        thr = np.where((alive & ~killed)[:, None], new_thr, thr)
        if mutant == "emission_after":
            rad[emits] += (thr * emission)[emits]
        alive = alive & ~killed
        o = np.where(alive[:, None], P + (sign * C_OFF)[:, None] * nrm, o)
        d = np.where(alive[:, None], new_d, d)
        e_d = np.where(alive, new_e, e_d)
        exact_origin &= ~alive

    tol = tol_env + (rel * EPS)[:, None] * rad
    if du_underived is None:
        tol = np.where((underived & (env_scale > 0).any(axis=1))[:, None], np.inf, tol)
    return {"value": rad, "tol": tol, "segments": segments, "fragile": fragile, "underived": underived, "kind": kind,
            "back": back, "emit": emit, "rr": rr, "env_scale": env_scale, "rel": rel, "stats": stats,
            "S": S, "intensity": float(intensity)}


def ratio(got, res, mask=None):
    """(n,) worst |got - value| / tol over the channels; a tol of 0 gives 0 for an exact match, else inf; a
    non-finite `got` or model value gives inf."""
    got = np.asarray(got, f64).reshape(-1, 3)
    err = np.abs(got - res["value"])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0.0, 0.0, err / res["tol"])
    r = np.where(np.isnan(r), np.inf, r).max(axis=1)
    return r if mask is None else r[mask]


def needed_du(got, res):
    """The smallest du whose bound covers `got` on the underived rays of res (0 without any): the inverse of
    tol = env_scale * intensity * (2 (S - 1) (du + eps) D + 16 eps M) + rel eps value.  inf where no du can (a
    channel the map holds constant, or a path that met no environment)."""
    m = res["underived"] & ~res["fragile"]
    if not m.any():
        return 0.0
    got = np.asarray(got, f64).reshape(-1, 3)[m]
    D, M = res["stats"]
    rest = np.abs(got - res["value"][m]) - (res["rel"][m] * EPS)[:, None] * res["value"][m]
    scale = res["env_scale"][m] * res["intensity"]
    with np.errstate(invalid="ignore", divide="ignore"):
        du = ((rest / scale) - 16 * EPS * M[None, :]) / (2.0 * (res["S"] - 1) * D[None, :]) - EPS
    du = np.where(rest <= 0, 0.0, np.where(np.isnan(du), np.inf, du))
    return float(max(0.0, du.max()))


def granted_du(oracle_needed):
    """4 x the oracle's worst needed du, not below 16 eps."""
    return max(4.0 * oracle_needed, DU_FLOOR)
