"""Float64 closed form of the direct-light term of a depth-1 path (test infrastructure, plain numpy).

The scene is fixed: a floor quad (x in [-8, 8], z in [-8, 6], y = 0) and one sphere (centre (0.3, 1.0, 0.2),
radius 1), each with a material row of its own.  The inputs are the camera position, the float32 primary
directions promoted to float64, two 12-float material rows (albedo3 metallic roughness emission3 ior type pad
pad) and one 8-float light row (type v3 colour3 intensity; type 0 directional with v the direction the light
travels, type 1 point with v its position).  The output is, per pixel, the radiance one light adds to a path that
ends at its first hit: evaluateBRDF(N, V, L) * Li * max(N.L, 0) when the shadow ray is unoccluded, else 0.

Written from the formulas, every operation in float64:
  first hit    the nearer of ray-plane (inside the quad) and ray-sphere (smaller positive root)
  normal       +Y on the floor, (P - c) / r on the sphere, negated when it faces along the ray
  directional  L = normalize(-v), Li = colour * intensity, distance infinite
  point        L = (pos - P) / dist, Li = colour * intensity / (1 + 0.09 dist + 0.032 dist^2)
  shadow ray   from P + N * 1e-4 * max(1, |P|_inf) along L over [1e-4, dist - 1e-4]
  BRDF         r = clamp(roughness, 0.02, 1), alpha = r^2, D = alpha^2 / (pi ((N.H)^2 (alpha^2 - 1) + 1)^2),
               k = (clamp(sqrt(alpha), 0.02, 1) + 1)^2 / 8, G = G1(N.L) G1(N.V) with G1(x) = x / (x (1 - k) + k),
               F0 = mix(((ior - 1) / (ior + 1))^2, albedo, metallic), F = F0 + (1 - F0) (1 - H.V)^5,
               spec = D G F / (4 N.V N.L + 0.0001), diffuse = albedo (1 - metallic) / pi,
               f = ((1 - F) diffuse + spec) * N.L      (the BRDF carries a cosine of its own)
"""
import numpy as np

FLOOR_X = (-8.0, 8.0)
FLOOR_Z = (-8.0, 6.0)
SPHERE = (0.3, 1.0, 0.2, 1.0)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _hit_floor(o, d, tmin, tmax):
    """t of the ray's crossing of the floor quad within [tmin, tmax], inf where there is none."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[..., 1] / d[..., 1]
    x = o[..., 0] + t * d[..., 0]
    z = o[..., 2] + t * d[..., 2]
    ok = np.isfinite(t) & (t >= tmin) & (t <= tmax) & (x >= FLOOR_X[0]) & (x <= FLOOR_X[1]) \
        & (z >= FLOOR_Z[0]) & (z <= FLOOR_Z[1])
    return np.where(ok, t, np.inf)


def _hit_sphere(o, d, tmin, tmax):
    """Smallest t within [tmin, tmax] at which the ray meets the sphere, inf where there is none."""
    c = np.array(SPHERE[:3], np.float64)
    r = SPHERE[3]
    oc = o - c
    a = _dot(d, d)
    b = _dot(oc, d)
    q = _dot(oc, oc) - r * r
    disc = b * b - a * q
    s = np.sqrt(np.maximum(disc, 0.0))
    t0, t1 = (-b - s) / a, (-b + s) / a
    in0 = (disc >= 0.0) & (t0 >= tmin) & (t0 <= tmax)
    in1 = (disc >= 0.0) & (t1 >= tmin) & (t1 <= tmax)
    return np.where(in0, t0, np.where(in1, t1, np.inf))


def brdf(mat, N, V, L):
    """Material::evaluateBRDF's value (the trailing N.L included) for one material row, float64."""
    albedo = np.asarray(mat[0:3], np.float64)
    metallic, roughness, ior = float(mat[3]), float(mat[4]), float(mat[8])
    H = V + L
    H = H / np.sqrt(_dot(H, H))[..., None]
    NdotV = np.maximum(_dot(N, V), 0.0)
    NdotL = np.maximum(_dot(N, L), 0.0)
    HdotV = np.maximum(_dot(H, V), 0.0)
    NdotH = np.maximum(_dot(N, H), 0.0)
    r = min(max(roughness, 0.02), 1.0)
    alpha = r * r
    a2 = alpha * alpha
    dd = NdotH * NdotH * (a2 - 1.0) + 1.0
    D = a2 / (np.pi * dd * dd)
    rk = min(max(np.sqrt(max(alpha, 0.0)), 0.02), 1.0)
    k = (rk + 1.0) ** 2 / 8.0
    G = (NdotL / (NdotL * (1.0 - k) + k)) * (NdotV / (NdotV * (1.0 - k) + k))
    f0 = ((ior - 1.0) / (ior + 1.0)) ** 2
    F0 = f0 * (1.0 - metallic) + albedo * metallic
    F = F0 + (1.0 - F0) * (np.clip(1.0 - HdotV, 0.0, 1.0) ** 5)[..., None]
    spec = (D * G)[..., None] * F / (4.0 * NdotV * NdotL + 0.0001)[..., None]
    diffuse = albedo * (1.0 - metallic) / np.pi
    return ((1.0 - F) * diffuse + spec) * NdotL[..., None]


def direct_light(cam_pos, dirs, mat_floor, mat_sphere, light):
    """dirs (..., 3).  Returns a dict: "radiance" (..., 3) float64, and the masks "hit" (first hit on either
    primitive), "sphere" (first hit on the sphere), "facing" (the light is in front of the surface) and
    "shadowed" (facing, and the shadow ray is occluded)."""
    d = np.asarray(dirs, np.float64)
    o = np.broadcast_to(np.asarray(cam_pos, np.float64), d.shape)
    light = np.asarray(light, np.float64)
    tf = _hit_floor(o, d, 0.0, np.inf)
    ts = _hit_sphere(o, d, 0.0, np.inf)
    hit = np.isfinite(tf) | np.isfinite(ts)
    sphere = ts < tf
    t = np.where(hit, np.minimum(tf, ts), 0.0)
    P = o + t[..., None] * d
    N = np.where(sphere[..., None], (P - np.array(SPHERE[:3])) / SPHERE[3], np.array([0.0, 1.0, 0.0]))
    N = np.where((_dot(N, d) > 0.0)[..., None], -N, N)
    V = -d
    rad = light[4:7] * light[7]
    if int(light[0]) == 0:
        v = -light[1:4]
        L = np.broadcast_to(v / np.sqrt(v @ v), d.shape)
        dist = np.full(d.shape[:-1], np.inf)
        Li = np.broadcast_to(rad, d.shape)
    else:
        lv = light[1:4] - P
        dist = np.sqrt(_dot(lv, lv))
        L = lv / dist[..., None]
        Li = rad / (1.0 + 0.09 * dist + 0.032 * dist * dist)[..., None]
    cs = np.maximum(_dot(N, L), 0.0)
    facing = hit & (cs > 0.0)
    eps = 1e-4 * np.maximum(1.0, np.abs(P).max(axis=-1))
    so = P + N * eps[..., None]
    tfar = dist - 1e-4
    occ = np.isfinite(_hit_floor(so, L, 1e-4, tfar)) | np.isfinite(_hit_sphere(so, L, 1e-4, tfar))
    f = np.where(sphere[..., None], brdf(mat_sphere, N, V, L), brdf(mat_floor, N, V, L))
    out = np.where((facing & ~occ)[..., None], f * Li * cs[..., None], 0.0)
    return {"radiance": out, "hit": hit, "sphere": hit & sphere, "facing": facing, "shadowed": facing & occ}
