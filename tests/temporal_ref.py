"""numpy float32 restatement of the denoiser's temporal reprojection (k_dn_reproject) and of the a-trous
variant whose colour sigma is per pixel (k_atrous<true>), in the kernels' operation order (DESIGN.md §6f
"Temporal reprojection").  Only + - x, correctly rounded division and square root, floor, max and compares,
and the library is compiled without contraction, so the device's results equal these bit for bit.

A pass is described by a dict `carry` = {"hist": (H, W, 4) t_0 rgb | m', "nz": (H, W, 4), "ids": (H, W, 2),
"cam": 14 floats}: what an earlier pass wrote (reproject's first result, with the planes and the camera it
ran for).  carry None: no history to take."""
from __future__ import annotations

import numpy as np

import denoise_ref as D

f32 = np.float32
_dot = D._dot
CLIP = f32(0.5)  # gamma of the history's variance clip (kHistoryClip)


def _clip_bounds(c0, ok, g):
    """mu -+ CLIP sd of c_0 over the 3 x 3 neighbours that are valid (hit, finite) and of the centre's geomID,
    summed in (dy, dx) row-major order."""
    Hh, Ww = ok.shape
    zero = f32(0.0)
    s1 = np.zeros((Hh, Ww, 3), f32)
    s2 = np.zeros((Hh, Ww, 3), f32)
    cnt = np.zeros((Hh, Ww), f32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y0, y1, x0, x1 = max(0, -dy), min(Hh, Hh - dy), max(0, -dx), min(Ww, Ww - dx)
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            valid = ok[Q] & (g[Q] == g[P])
            cq = np.where(valid[..., None], c0[Q], zero)
            s1[P] = s1[P] + cq
            s2[P] = s2[P] + cq * cq
            cnt[P] = cnt[P] + valid.astype(f32)
    mu = s1 / cnt[..., None]
    var = s2 / cnt[..., None] - mu * mu
    var = np.where(zero < var, var, zero)  # max(0, var); 0 for a NaN
    sd = np.sqrt(var)
    return mu - CLIP * sd, mu + CLIP * sd


def reproject(c0: np.ndarray, n: int, nz: np.ndarray, ids: np.ndarray, cam: np.ndarray, carry: dict | None,
              max_history: int, sigma_depth: float = 0.0, normal_log2_power: int = 0):
    """(hist (H, W, 4) = t_0 | m', reprojected): the integrated colour and history length of every pixel, and
    the number of pixels that took history (m > 0).  c0 (H, W, 3): the accumulation's mean (D.mean)."""
    sz = f32(sigma_depth or D.DEFAULTS["sigma_depth"])
    nl = int(normal_log2_power or D.DEFAULTS["normal_log2_power"])
    c0 = np.asarray(c0, f32)
    Hh, Ww = c0.shape[:2]
    nf = f32(n)
    z = np.asarray(nz[..., 3], f32)
    ok = ~(z < 0) & np.isfinite(c0).all(axis=-1)  # the others pass through with m' = 0
    hist = np.zeros((Hh, Ww, 4), f32)
    hist[..., 0:3] = c0
    hist[..., 3] = np.where(ok, nf, f32(0.0))
    if carry is None:
        return hist, 0
    cam = np.asarray(cam, f32)
    pc = np.asarray(carry["cam"], f32)
    pos2, fw2, rt2, up2, hw2, hh2 = pc[0:3], pc[3:6], pc[6:9], pc[9:12], pc[12], pc[13]
    h2 = np.asarray(carry["hist"], f32)
    nz2 = np.asarray(carry["nz"], f32)
    g2 = np.asarray(carry["ids"], np.uint32)[..., 0]
    g1 = np.asarray(ids, np.uint32)[..., 0]
    N1 = np.asarray(nz[..., 0:3], f32)
    half, one, zero = f32(0.5), f32(1.0), f32(0.0)
    with np.errstate(all="ignore"):
        d = D.pixel_centre_dirs(cam, Ww, Hh)
        P = cam[None, None, 0:3] + z[..., None] * d
        v = P - pos2[None, None, :]
        zf = _dot(v, fw2[None, None, :])
        nx = _dot(v, rt2[None, None, :]) / (zf * hw2)
        ny = _dot(v, up2[None, None, :]) / (zf * hh2)
        fx = (nx * half + half) * f32(Ww) - half
        fy = (half - ny * half) * f32(Hh) - half
        inside = (fx > f32(-1.0)) & (fx < f32(Ww)) & (fy > f32(-1.0)) & (fy < f32(Hh))  # False for a NaN
        take = ok & (zf > zero) & inside
        fxs, fys = np.where(take, fx, zero), np.where(take, fy, zero)  # (no conversion of a rejected value)
        x0f, y0f = np.floor(fxs), np.floor(fys)
        a, b = fxs - x0f, fys - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        dist = np.sqrt(_dot(v, v))
        ws = np.zeros((Hh, Ww), f32)
        hs = np.zeros((Hh, Ww, 3), f32)
        ms = np.zeros((Hh, Ww), f32)
        for j in (0, 1):
            wy = b if j else one - b
            for i in (0, 1):
                w = (a if i else one - a) * wy
                qx, qy = x0 + i, y0 + j
                inb = take & (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                cx, cy = np.clip(qx, 0, Ww - 1), np.clip(qy, 0, Hh - 1)
                hq, nq = h2[cy, cx], nz2[cy, cx]
                wn = np.maximum(zero, _dot(N1, nq[..., 0:3]))
                for _ in range(nl):
                    wn = wn * wn
                e = np.abs(dist - nq[..., 3]) / (sz * np.maximum(dist, nq[..., 3]))
                wz = one / (one + e * e)
                valid = (inb & ~(nq[..., 3] < 0) & np.isfinite(hq[..., 0:3]).all(axis=-1) & (g2[cy, cx] == g1)
                         & (wn * wz >= half))
                w = np.where(valid, w, zero)
                hq = np.where(valid[..., None], hq, zero)
                ws = ws + w
                hs = hs + w[..., None] * hq[..., 0:3]
                ms = ms + w * hq[..., 3]
        got = take & (ws > zero)
        h = hs / ws[..., None]
        if not np.array_equal(cam, pc):  # the view changed: the history is clipped to the current neighbourhood
            lo, hi = _clip_bounds(c0, ok, g1)
            h = np.where(h < lo, lo, h)
            h = np.where(hi < h, hi, h)
        m = ms / ws
        m = np.where(m < f32(max_history), m, f32(max_history))
        got = got & (m > zero)
        neff = nf + m
        t0 = (nf * c0 + m[..., None] * h) / neff[..., None]
    hist[..., 0:3] = np.where(got[..., None], t0, c0)
    hist[..., 3] = np.where(got, neff, hist[..., 3])
    return hist.astype(f32), int(got.sum())


def atrous_per_pixel(hist: np.ndarray, nz: np.ndarray, albedo: np.ndarray, iterations: int, sigma_color: float = 0.0,
                     sigma_depth: float = 0.0, sigma_albedo: float = 0.0, normal_log2_power: int = 0) -> np.ndarray:
    """D.atrous with S = sigma_c 2^-i / n_eff(p), n_eff = hist[..., 3], for the centre pixel p."""
    sc = f32(sigma_color or D.DEFAULTS["sigma_color"])
    sz = f32(sigma_depth or D.DEFAULTS["sigma_depth"])
    sa = f32(sigma_albedo or D.DEFAULTS["sigma_albedo"])
    nl = int(normal_log2_power or D.DEFAULTS["normal_log2_power"])
    c = np.array(hist[..., 0:3], f32)
    neff = np.asarray(hist[..., 3], f32)
    Hh, Ww = c.shape[:2]
    N = np.ascontiguousarray(nz[..., 0:3], f32)
    z = np.ascontiguousarray(nz[..., 3], f32)
    A = np.asarray(albedo, f32)
    hit = ~(z < 0)
    sa2 = sa * sa
    one, zero = f32(1.0), f32(0.0)
    for it in range(iterations):
        s = 1 << it
        with np.errstate(all="ignore"):
            S = sc * (one / f32(1 << it)) / neff
            S2 = S * S
            ok = hit & np.isfinite(c).all(axis=-1)
            acc = np.zeros((Hh, Ww, 3), f32)
            wsum = np.zeros((Hh, Ww), f32)
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
                    wc = one / (one + _dot(dc, dc) / S2[P])
                    w = D.H5[dy + 2] * D.H5[dx + 2] * wn * wz * wa * wc
                    valid = ok[Q]
                    w = np.where(valid, w, zero)
                    cq = np.where(valid[..., None], c[Q], zero)
                    acc[P] = acc[P] + w[..., None] * cq
                    wsum[P] = wsum[P] + w
            out = acc / wsum[..., None]
        c = np.where(ok[..., None], out, c).astype(f32)
    return c


def denoise(accum: np.ndarray, n: int, nz: np.ndarray, albedo: np.ndarray, ids: np.ndarray, cam: np.ndarray,
            carry: dict | None, max_history: int, iterations: int, **params):
    """One pass with history on: (filtered (H, W, 3), hist (H, W, 4), reprojected).  hist, nz, ids and cam are
    what a later pass takes as its carry."""
    hist, cnt = reproject(D.mean(accum, n), n, nz, ids, cam, carry, max_history,
                          params.get("sigma_depth", 0.0), params.get("normal_log2_power", 0))
    return atrous_per_pixel(hist, nz, albedo, iterations, **params), hist, cnt
