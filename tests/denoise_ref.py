"""numpy float32 restatement of the first-hit AOV rays (k_aov) and of the edge-avoiding a-trous filter
(k_dn_mean, k_atrous) of sptr_set_denoise, in the kernels' operation order (DESIGN.md "Denoiser").

The filter uses only + - x, correctly rounded division, max and compares, and the library is compiled
without contraction, so the device's results equal these bit for bit.  The last step, the resolve of the
filtered mean (ACES, gamma, 8 bit), is oracle.resolve(c, 1).
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
H5 = (f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625))  # B3 spline, 1/16 1/4 3/8 1/4 1/16
DEFAULTS = dict(sigma_color=0.5, sigma_depth=0.05, sigma_albedo=0.2, normal_log2_power=6)
MISS = 0xFFFFFFFF


def _dot(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def pixel_centre_dirs(cam: np.ndarray, W: int, H: int) -> np.ndarray:
    """(H, W, 3): camera_dir(div(x + 0.5, W), div(y + 0.5, H)) as Camera::getRayDirection evaluates it.
    cam: pos3 forward3 right3 up3 half_width half_height (sptr.Camera.as_array / oracle.camera)."""
    cam = np.asarray(cam, f32)
    fw, rt, up, hw, hh = cam[3:6], cam[6:9], cam[9:12], cam[12], cam[13]
    u = (np.arange(W, dtype=f32) + f32(0.5)) / f32(W)
    v = (np.arange(H, dtype=f32) + f32(0.5)) / f32(H)
    nx = ((u - f32(0.5)) * f32(2.0))[None, :, None]
    ny = (-(v - f32(0.5)) * f32(2.0))[:, None, None]
    d = (fw[None, None, :] + (nx * hw) * rt[None, None, :]) + (ny * hh) * up[None, None, :]
    return (d * (f32(1.0) / np.sqrt(_dot(d, d)))[..., None]).astype(f32)


def pixel_centre_rays(cam: np.ndarray, W: int, H: int, dirs: np.ndarray | None = None) -> np.ndarray:
    """(H*W, 8) o3 d3 tnear tfar: the wavefront primary ray's tnear 0 and tfar inf."""
    d = pixel_centre_dirs(cam, W, H) if dirs is None else dirs
    rays = np.zeros((H * W, 8), f32)
    rays[:, 0:3] = np.asarray(cam, f32)[0:3]
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 7] = np.inf
    return rays


def aov_from_hits(geom, prim, t, ng, dirs, materials, geom_material):
    """The AOV planes from closest-hit results (Renderer.intersect / oracle.Prepared.intersect) on the
    pixel-centre rays: nz (H, W, 4) = normal facing the camera | depth, albedo (H, W, 3), ids (H, W, 2).
    materials: (n, 12) float32 rows starting with the albedo."""
    Hh, Ww = dirs.shape[:2]
    geom = np.asarray(geom, np.uint32).reshape(Hh, Ww)
    hit = geom != MISS
    ng = np.asarray(ng, f32).reshape(Hh, Ww, 3)
    with np.errstate(all="ignore"):
        l2 = _dot(ng, ng)
        n = ng * (f32(1.0) / np.sqrt(l2))[..., None]
        n = np.where((l2 <= 0)[..., None], f32(0.0), n)
        n = np.where((_dot(n, dirs) > 0)[..., None], -n, n)
    nz = np.zeros((Hh, Ww, 4), f32)
    nz[..., 3] = -1.0
    nz[hit, 0:3] = n[hit]
    nz[hit, 3] = np.asarray(t, f32).reshape(Hh, Ww)[hit]
    albedo = np.zeros((Hh, Ww, 3), f32)
    mats = np.asarray(materials, f32)
    albedo[hit] = mats[np.asarray(geom_material)[geom[hit]], 0:3]
    ids = np.stack([geom, np.asarray(prim, np.uint32).reshape(Hh, Ww)], axis=-1)
    return nz, albedo, ids


def mean(accum: np.ndarray, n: int) -> np.ndarray:
    """c_0: the resolve's first step."""
    return (np.asarray(accum, f32) / f32(n)).astype(f32)


def atrous(c0: np.ndarray, nz: np.ndarray, albedo: np.ndarray, n: int, iterations: int, sigma_color: float = 0.0,
           sigma_depth: float = 0.0, sigma_albedo: float = 0.0, normal_log2_power: int = 0) -> np.ndarray:
    """c_iterations (H, W, 3) from c_0, the AOV planes and the accumulation's frame count n.  A zero
    parameter takes its default, as sptr_set_denoise."""
    sc = f32(sigma_color or DEFAULTS["sigma_color"])
    sz = f32(sigma_depth or DEFAULTS["sigma_depth"])
    sa = f32(sigma_albedo or DEFAULTS["sigma_albedo"])
    nl = int(normal_log2_power or DEFAULTS["normal_log2_power"])
    c = np.array(c0, f32)
    Hh, Ww = c.shape[:2]
    N = np.ascontiguousarray(nz[..., 0:3], f32)
    z = np.ascontiguousarray(nz[..., 3], f32)
    A = np.asarray(albedo, f32)
    hit = ~(z < 0)
    sa2 = sa * sa
    one, zero = f32(1.0), f32(0.0)
    for i in range(iterations):
        s = 1 << i
        S = sc * (one / f32(1 << i)) / f32(n)
        S2 = S * S
        ok = hit & np.isfinite(c).all(axis=-1)  # the others pass through, and weigh 0 as neighbours
        acc = np.zeros((Hh, Ww, 3), f32)
        wsum = np.zeros((Hh, Ww), f32)
        with np.errstate(all="ignore"):
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * s, dx * s
                    y0, y1, x0, x1 = max(0, -oy), min(Hh, Hh - oy), max(0, -ox), min(Ww, Ww - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    wn = np.maximum(zero, _dot(N[P], N[Q]))
                    for _ in range(nl):
                        wn = wn * wn
                    e = np.abs(z[P] - z[Q]) / (sz * np.maximum(z[P], z[Q]))
                    wz = one / (one + e * e)
                    da = A[P] - A[Q]
                    wa = one / (one + _dot(da, da) / sa2)
                    dc = c[P] - c[Q]
                    wc = one / (one + _dot(dc, dc) / S2)
                    w = H5[dy + 2] * H5[dx + 2] * wn * wz * wa * wc
                    valid = ok[Q]
                    w = np.where(valid, w, zero)
                    cq = np.where(valid[..., None], c[Q], zero)
                    acc[P] = acc[P] + w[..., None] * cq
                    wsum[P] = wsum[P] + w
            out = acc / wsum[..., None]
        c = np.where(ok[..., None], out, c).astype(f32)
    return c


def denoise(accum: np.ndarray, n: int, nz: np.ndarray, albedo: np.ndarray, iterations: int, **params) -> np.ndarray:
    return atrous(mean(accum, n), nz, albedo, n, iterations, **params)
