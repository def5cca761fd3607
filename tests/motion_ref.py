"""numpy float32 restatement of the temporal reprojection through the previous geometry (k_dn_reproject<true>,
sptr_set_history_motion), in the kernel's operation order (DESIGN.md §6h "Motion vectors").  As
tests/temporal_ref.py: only + - x, correctly rounded division and square root, floor, max and compares, no
contraction, so the device's results equal these bit for bit.

The pass differs from temporal_ref.reproject in three places.  The point projected into the carry's camera is
the pixel's surface point carried to the previous geometry: a triangle hit's through its barycentrics (the
SPTR_AOV_UV plane) and the previous positions' record, a sphere hit's through its unit offset from the current
centre.  The taps' normal weight takes the previous geometry's normal at that point, turned towards the carry's
camera.  The history taken is always clipped.  The offset of the projection from the pixel is the motion vector.

Inputs: the planes the device hands out (nz, ids, uv), the carry dict of temporal_ref, and `topo` = (indices
(T, 3), tri_geom_first (G + 1,)), `prev` = (positions, spheres) the carry's pass saw, `cur` = the current ones
(of which only the spheres are read)."""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import query_common as Q
import temporal_ref as T

f32 = np.float32
_dot = D._dot
QNAN = np.uint32(0x7FC00000).view(f32)


def _safe_normalize(v):
    l2 = _dot(v, v)
    n = v * (f32(1.0) / np.sqrt(l2))[..., None]
    return np.where((l2 <= 0)[..., None], f32(0.0), n).astype(f32)


def previous_points(nz, ids, uv, cam, topo, prev, cur):
    """(P' (H, W, 3), n' (H, W, 3), known (H, W)): every hit pixel's surface point on the previous geometry and
    the normalised geometric normal there (not yet turned towards any camera); known: the pixel is a hit of
    the uploaded topology (false on a miss)."""
    indices, first = np.asarray(topo[0], np.int64).reshape(-1, 3), np.asarray(topo[1], np.int64)
    pos_prev = np.asarray(prev[0], f32).reshape(-1, 3)
    sph_prev = np.asarray(prev[1], f32).reshape(-1, 4)
    sph_cur = np.asarray(cur[1], f32).reshape(-1, 4)
    Hh, Ww = nz.shape[:2]
    G = len(first) - 1
    geom = np.asarray(ids, np.uint32)[..., 0].astype(np.int64)
    prim = np.asarray(ids, np.uint32)[..., 1].astype(np.int64)
    z = np.asarray(nz[..., 3], f32)
    hit = ~(z < 0) & (geom != D.MISS)
    is_tri = hit & (geom < G)
    is_sph = hit & (geom >= G) & (geom - G < len(sph_cur))
    Pp = np.zeros((Hh, Ww, 3), f32)
    n = np.zeros((Hh, Ww, 3), f32)
    with np.errstate(all="ignore"):
        if is_tri.any():
            tri = first[geom[is_tri]] + prim[is_tri]
            i = indices[tri]
            v0, v1, v2 = pos_prev[i[:, 0]], pos_prev[i[:, 1]], pos_prev[i[:, 2]]
            e1, e2 = v0 - v1, v2 - v0  # tri_record: plain float32 differences
            ng = Q._e_cross(e2, e1)
            u, v = np.asarray(uv, f32)[is_tri, 0], np.asarray(uv, f32)[is_tri, 1]
            Pp[is_tri] = (v0 - u[:, None] * e1) + v[:, None] * e2  # e1 = v0 - v1, hence the minus
            n[is_tri] = _safe_normalize(ng)
        if is_sph.any():
            cam = np.asarray(cam, f32)
            d = D.pixel_centre_dirs(cam, Ww, Hh)[is_sph]
            P = cam[None, 0:3] + z[is_sph][:, None] * d
            s = geom[is_sph] - G
            c, cp = sph_cur[s], sph_prev[s]
            g = (P - c[:, 0:3]) / c[:, 3:4]
            Pp[is_sph] = cp[:, 0:3] + cp[:, 3:4] * g
            n[is_sph] = _safe_normalize(g)
    return Pp, n, is_tri | is_sph


def reproject(c0, n, nz, ids, uv, cam, carry, max_history, topo, prev, cur, sigma_depth: float = 0.0,
              normal_log2_power: int = 0):
    """(hist (H, W, 4) = t_0 | m', reprojected, motion (H, W, 2)).  carry as temporal_ref's, not None: the pass
    takes this path only with a carry of an earlier geometry."""
    sz = f32(sigma_depth or D.DEFAULTS["sigma_depth"])
    nl = int(normal_log2_power or D.DEFAULTS["normal_log2_power"])
    c0 = np.asarray(c0, f32)
    Hh, Ww = c0.shape[:2]
    nf = f32(n)
    z = np.asarray(nz[..., 3], f32)
    ok = ~(z < 0) & np.isfinite(c0).all(axis=-1)
    hist = np.zeros((Hh, Ww, 4), f32)
    hist[..., 0:3] = c0
    hist[..., 3] = np.where(ok, nf, f32(0.0))
    pc = np.asarray(carry["cam"], f32)
    pos2, fw2, rt2, up2, hw2, hh2 = pc[0:3], pc[3:6], pc[6:9], pc[9:12], pc[12], pc[13]
    h2 = np.asarray(carry["hist"], f32)
    nz2 = np.asarray(carry["nz"], f32)
    g2 = np.asarray(carry["ids"], np.uint32)[..., 0]
    g1 = np.asarray(ids, np.uint32)[..., 0]
    half, one, zero = f32(0.5), f32(1.0), f32(0.0)
    Pp, N1, known = previous_points(nz, ids, uv, cam, topo, prev, cur)
    with np.errstate(all="ignore"):
        v = Pp - pos2[None, None, :]
        N1 = np.where((_dot(N1, v) > zero)[..., None], -N1, N1)
        zf = _dot(v, fw2[None, None, :])
        nx = _dot(v, rt2[None, None, :]) / (zf * hw2)
        ny = _dot(v, up2[None, None, :]) / (zf * hh2)
        fx = (nx * half + half) * f32(Ww) - half
        fy = (half - ny * half) * f32(Hh) - half
        reach = ok & known
        motion = np.full((Hh, Ww, 2), QNAN, f32)
        motion[..., 0] = np.where(reach, fx - np.arange(Ww, dtype=f32)[None, :], QNAN)
        motion[..., 1] = np.where(reach, fy - np.arange(Hh, dtype=f32)[:, None], QNAN)
        inside = (fx > f32(-1.0)) & (fx < f32(Ww)) & (fy > f32(-1.0)) & (fy < f32(Hh))
        take = reach & (zf > zero) & inside
        fxs, fys = np.where(take, fx, zero), np.where(take, fy, zero)
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
        lo, hi = T._clip_bounds(c0, ok, g1)  # always: the scene state changed
        h = np.where(h < lo, lo, h)
        h = np.where(hi < h, hi, h)
        m = ms / ws
        m = np.where(m < f32(max_history), m, f32(max_history))
        got = got & (m > zero)
        neff = nf + m
        t0 = (nf * c0 + m[..., None] * h) / neff[..., None]
    hist[..., 0:3] = np.where(got[..., None], t0, c0)
    hist[..., 3] = np.where(got, neff, hist[..., 3])
    return hist.astype(f32), int(got.sum()), motion


def denoise(accum, n, nz, albedo, ids, uv, cam, carry, max_history, iterations, topo, prev, cur, **params):
    """One pass on the motion path: (filtered (H, W, 3), hist (H, W, 4), reprojected, motion (H, W, 2))."""
    hist, cnt, motion = reproject(D.mean(accum, n), n, nz, ids, uv, cam, carry, max_history, topo, prev, cur,
                                  params.get("sigma_depth", 0.0), params.get("normal_log2_power", 0))
    return T.atrous_per_pixel(hist, nz, albedo, iterations, **params), hist, cnt, motion
