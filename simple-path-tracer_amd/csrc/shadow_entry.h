// shadow_entry.h — light-space cells of a directional light's shadow rays, for host and device.
//
// Every shadow ray of a directional light runs along the same direction w, so which primitives it can hit
// depends only on where its origin projects on the plane perpendicular to w.  The plane carries an orthonormal
// frame (eu, ev), chosen once on the host and stored with the table so that build and query use the same
// floats, and a grid of R x R square cells over the scene's projected bounds.  The table holds one walk entry
// word per cell (k_shadow_entries; the encoding of the bounce-0 cull's entries), computed from the tests below:
// "no ray that starts in this cell's prism and runs along +-w can hit this box / sphere / triangle".
//
// The tests only ever err towards "may hit", in the manner of cull_prims.h: every comparison carries a relative
// slack (kCullPrimSlack) and an absolute bound on the float rounding of its operands, a NaN makes every
// comparison false (not outside), and whether the primitive lies ahead of or behind an origin is ignored.  The
// prism of a cell is the cell widened by shadow_cell_margin, which covers the rounding of the query's two dot
// products and of its cell arithmetic.  The query projects the ray's own origin, which already carries
// light_term's n * eps offset, so that offset needs no margin of its own.
#pragma once
#include "cull_prims.h"

namespace sptr {

struct ShadowFrame {
  vec3 eu, ev;   // orthonormal, perpendicular to the light direction
  float u0, v0;  // the table's lower corner in (u, v)
  float cell;    // cell edge
  float inv_cell;
  float mag;     // L1 bound of the coordinates of any point of the scene (rounding is relative to it)
  float diag;    // bound of the distance between two points of the scene
  uint32_t R;    // cells per side
};

struct ShadowPrism {
  float a0, a1, b0, b1;  // [a0, a1] x [b0, b1] in (u, v), margin included
  float mag, diag;
  vec3 eu, ev;
};

// (eu, ev) for light direction w (unit): eu = normalize(axis x w) with the coordinate axis least aligned with w
inline void shadow_frame_axes(vec3 w, vec3& eu, vec3& ev) {
  const float ax = cull_abs(w.x), ay = cull_abs(w.y), az = cull_abs(w.z);
  const vec3 a = (ax <= ay && ax <= az) ? v3(1.0f, 0.0f, 0.0f) : (ay <= az ? v3(0.0f, 1.0f, 0.0f) : v3(0.0f, 0.0f, 1.0f));
  const vec3 c = cross(a, w);
  eu = c * (1.0f / cull_len(c));
  const vec3 d = cross(w, eu);
  ev = d * (1.0f / cull_len(d));
}

// The frame of an R x R table over the box [lo, hi] (the scene's bounds), padded by 1 % of its extent and by
// the cell margin.  false: no usable frame (empty or non-finite bounds, zero direction).
inline bool shadow_frame(vec3 w, vec3 lo, vec3 hi, uint32_t R, ShadowFrame& f) {
  const float wl = cull_len(w);
  if (!(wl > 0.5f && wl < 2.0f) || R == 0u) return false;
  if (!(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z)) return false;
  shadow_frame_axes(w * (1.0f / wl), f.eu, f.ev);
  float umin = 3.0e38f, umax = -3.0e38f, vmin = 3.0e38f, vmax = -3.0e38f;
  for (int k = 0; k < 8; ++k) {
    const vec3 p = v3((k & 1) ? hi.x : lo.x, (k & 2) ? hi.y : lo.y, (k & 4) ? hi.z : lo.z);
    const float u = dot(p, f.eu), v = dot(p, f.ev);
    umin = u < umin ? u : umin;
    umax = u > umax ? u : umax;
    vmin = v < vmin ? v : vmin;
    vmax = v > vmax ? v : vmax;
  }
  auto amax = [](float a, float b) { return cull_abs(a) > cull_abs(b) ? cull_abs(a) : cull_abs(b); };
  f.mag = amax(lo.x, hi.x) + amax(lo.y, hi.y) + amax(lo.z, hi.z);
  f.diag = cull_len(hi - lo);
  const float ext = (umax - umin) > (vmax - vmin) ? (umax - umin) : (vmax - vmin);
  const float pad = 0.01f * ext + 1e-4f * f.mag + 1e-6f;
  const float side = ext + 2.0f * pad;
  f.R = R;
  f.cell = side / float(R);
  f.inv_cell = float(R) / side;
  f.u0 = 0.5f * (umin + umax) - 0.5f * side;
  f.v0 = 0.5f * (vmin + vmax) - 0.5f * side;
  return f.mag < 1.0e30f && side > 0.0f && side < 1.0e30f;
}

// Cell of an origin; false: outside the table (or NaN), the caller walks from the scene's root.
SPTR_HD bool shadow_cell(const ShadowFrame& f, vec3 o, uint32_t& i, uint32_t& j) {
  const float fi = (dot(o, f.eu) - f.u0) * f.inv_cell, fj = (dot(o, f.ev) - f.v0) * f.inv_cell;
  const float r = float(f.R);
  if (!(fi >= 0.0f && fi < r && fj >= 0.0f && fj < r)) return false;
  i = (uint32_t)fi;
  j = (uint32_t)fj;
  return true;
}

// What the prism is widened by on every side: the query's u and v round by a few 2^-24 of the origin's
// coordinates (<= 4e-7 mag), its cell arithmetic by 2^-23 of the table's side (1.2e-7 R cells, R <= 256),
// the build's cell corners likewise; 1e-5 mag + 1e-4 cell is more than ten times their sum.
SPTR_HD float shadow_cell_margin(const ShadowFrame& f) { return 1e-5f * f.mag + kCullPrimSlack * f.cell; }

SPTR_HD ShadowPrism shadow_prism(const ShadowFrame& f, uint32_t i, uint32_t j) {
  const float m = shadow_cell_margin(f);
  ShadowPrism p;
  p.a0 = f.u0 + float(i) * f.cell - m;
  p.a1 = f.u0 + float(i + 1u) * f.cell + m;
  p.b0 = f.v0 + float(j) * f.cell - m;
  p.b1 = f.v0 + float(j + 1u) * f.cell + m;
  p.mag = f.mag;
  p.diag = f.diag;
  p.eu = f.eu;
  p.ev = f.ev;
  return p;
}

// no ray of the prism can hit the box [lo, hi]: its extent along eu and along ev against the cell's
SPTR_HD bool shadow_box_outside(const ShadowPrism& p, vec3 lo, vec3 hi) {
  const vec3 e[2] = {p.eu, p.ev};
  const float c0[2] = {p.a0, p.b0}, c1[2] = {p.a1, p.b1};
  for (int k = 0; k < 2; ++k) {
    const vec3 n = e[k];
    const vec3 pmin = v3(n.x >= 0.0f ? lo.x : hi.x, n.y >= 0.0f ? lo.y : hi.y, n.z >= 0.0f ? lo.z : hi.z);
    const vec3 pmax = v3(n.x >= 0.0f ? hi.x : lo.x, n.y >= 0.0f ? hi.y : lo.y, n.z >= 0.0f ? hi.z : lo.z);
    const float bmin = dot(pmin, n), bmax = dot(pmax, n);
    const float slack = kCullPrimSlack * (cull_mag(pmin, n) + cull_mag(pmax, n)) + kCullPrimRound * p.mag;
    if (bmin > c1[k] + slack) return true;
    if (bmax < c0[k] - slack) return true;
  }
  return false;
}

// no ray of the prism can hit the sphere (centre C, radius R): the centre's distance to the cell in the plane.
// The radius is inflated as in cull_sphere_outside, with the scene's diagonal for the origin's distance.
SPTR_HD bool shadow_sphere_outside(const ShadowPrism& p, vec3 C, float R) {
  const float cu = dot(C, p.eu), cv = dot(C, p.ev);
  const float round = kCullPrimRound * (p.mag + cull_mag(C, p.eu) + cull_mag(C, p.ev));
  const float Re = sq_root(R * R + 1e-6f * p.diag * p.diag) + round;
  float du = 0.0f, dv = 0.0f;
  if (cu < p.a0) du = p.a0 - cu;
  if (cu > p.a1) du = cu - p.a1;
  if (cv < p.b0) dv = p.b0 - cv;
  if (cv > p.b1) dv = cv - p.b1;
  const float lim = Re + kCullPrimSlack * (Re + du + dv) + round;
  return du * du + dv * dv > lim * lim;
}

// no ray of the prism can hit the triangle: a separating axis between its projection and the cell, one of
// eu, ev or the three edge normals.  Along an edge normal the projected triangle spans [0, s] with s the third
// vertex's offset, which covers a triangle seen edge-on (s ~ 0: a segment) and a zero-length edge (no axis).
SPTR_HD bool shadow_triangle_outside(const ShadowPrism& p, vec3 v0, vec3 v1, vec3 v2) {
  const vec3 q[3] = {v0, v1, v2};
  float u[3], v[3];
  for (int k = 0; k < 3; ++k) {
    u[k] = dot(q[k], p.eu);
    v[k] = dot(q[k], p.ev);
  }
  const float round = kCullPrimRound * p.mag;
  {
    const float umin = fmin_g(u[0], fmin_g(u[1], u[2])), umax = fmax_g(u[0], fmax_g(u[1], u[2]));
    const float vmin = fmin_g(v[0], fmin_g(v[1], v[2])), vmax = fmax_g(v[0], fmax_g(v[1], v[2]));
    const float su = kCullPrimSlack * (cull_abs(umin) + cull_abs(umax)) + round;
    const float sv = kCullPrimSlack * (cull_abs(vmin) + cull_abs(vmax)) + round;
    if (umin > p.a1 + su || umax < p.a0 - su || vmin > p.b1 + sv || vmax < p.b0 - sv) return true;
  }
  const float cu[4] = {p.a0, p.a1, p.a1, p.a0}, cv[4] = {p.b0, p.b0, p.b1, p.b1};
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    const float nu = -(v[i1] - v[i]), nv = u[i1] - u[i];  // the edge's normal in the plane
    const float nl = cull_abs(nu) + cull_abs(nv);
    const float st = nu * (u[i2] - u[i]) + nv * (v[i2] - v[i]);
    float mag = cull_abs(nu * (u[i2] - u[i])) + cull_abs(nv * (v[i2] - v[i]));
    float cmin = 3.0e38f, cmax = -3.0e38f;
    bool nan = false;
    for (int k = 0; k < 4; ++k) {
      const float a = nu * (cu[k] - u[i]), b = nv * (cv[k] - v[i]);
      const float s = a + b;
      nan = nan || !(s == s);
      cmin = s < cmin ? s : cmin;
      cmax = s > cmax ? s : cmax;
      mag = fmax_g(mag, cull_abs(a) + cull_abs(b));
    }
    if (nan || !(st == st)) continue;
    const float tmin = st < 0.0f ? st : 0.0f, tmax = st > 0.0f ? st : 0.0f;
    // (the operands u, v round by ~1e-7 mag each: 4 round nl bounds what that moves any of the sums by)
    const float slack = kCullPrimSlack * mag + 4.0f * round * nl;
    if (cmin > tmax + slack || cmax < tmin - slack) return true;
  }
  return false;
}

}  // namespace sptr
