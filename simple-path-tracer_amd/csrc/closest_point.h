// closest_point.h — the definition of sptr_query_points, for host and device: the closest point of one primitive
// to a point p (the candidate), the lower bound on every candidate of a box (node_bound), and the order of
// candidates.  k_pointquery (kernels_points.h) and the host twin sptr_host_query_points (host/host_api.cpp) call
// these functions, and tests/cpp/test_closest_point.cpp compiles the same text.  Only + - *, IEEE / and sqrt and
// compares are used, each written out; with -ffp-contract=off on both sides host and device give the same bits.
//
// Triangle.  From the stored record (v0, e1 = v0 - v1, e2 = v2 - v0; tri_record in lbvh_shared.h): ab = -e1,
// ac = e2, bc = ac - ab.  Four candidates, each a pair of weights (u, v) of v1 and v2:
//   edge ab : (t, 0),     t = clamp01(ap.ab / ab.ab)
//   edge ac : (0, t),     t = clamp01(ap.ac / ac.ac)
//   edge bc : (1 - t, t), t = clamp01(bp.bc / bc.bc), bp = ap - ab
//   face    : alpha = ab.ac / ab.ab, ep = ac - alpha ab, w = ap.ep / ep.ep, s = ap.ab / ab.ab - alpha w; (s, w),
//             taken only when s >= 0, w >= 0 and s + w <= 1 (a NaN or an infinity from a vanishing ab or ep fails)
// clamp01(num / den) is 0 unless num > 0 and den > 0, else min(num / den, 1): the weights are finite and convex by
// construction.  Each candidate's point is q = v0 + (ab u + ac v) and its d2 = (p - q).(p - q) of that q: the
// distance of a point of the triangle, never a plane distance.  The triangle's candidate is the one with the
// smallest d2, the first in the order above on ties.  (The textbook region classification cancels in its
// products' differences on thin triangles; a clamped projection does not, and the face solve is orthogonalised.)
//
// Sphere (a surface): m = p - c, len = sqrt(m.m), d2 = (len - r)^2, q = c + m (r / len), or c + (r, 0, 0) when
// len == 0; ng = (q - c) / r per component (0 when r is not positive); uv = 0.
//
// node_bound(p, lo, hi, M): a float32 lower bound on the d2 of every candidate of every primitive whose box lies
// in [lo, hi], for M >= max(|p|_inf, the largest absolute coordinate of the scene).  Per axis the gap
// max(lo - p, p - hi) is reduced by kCpPad M and clamped at 0, and the sum of squares is scaled by kCpShrink.
// DESIGN.md par. 6l derives both constants from the roundings above; the wide nodes' float32 plane decoding
// (cp_wide_plane) is covered by the same pad.
//
// Order: the candidate with the smaller key (d2, geomID, primID) wins, d2 compared as float and the ids as unsigned.
#pragma once
#include <stdint.h>

#include "sptr_math.h"

namespace sptr {

constexpr float kCpPad = 0x1p-20f;         // 16 eps, eps = 2^-24
constexpr float kCpShrink = 0x1.ffffep-1f;  // 1 - 16 eps
constexpr float kCpHuge = 3.402823466e+38f;

struct CpCand {
  float d2;
  vec3 q;
  float u, v;
};

SPTR_HD bool cp_finite(float x) { return (x < 0.0f ? -x : x) <= kCpHuge; }
// A point takes part in the walk only with finite coordinates and a radius that is neither negative nor NaN.
SPTR_HD bool cp_point_valid(vec3 p, float max_dist) {
  return cp_finite(p.x) && cp_finite(p.y) && cp_finite(p.z) && max_dist >= 0.0f;
}
SPTR_HD float cp_abs_max(vec3 p) {
  const float ax = p.x < 0.0f ? -p.x : p.x, ay = p.y < 0.0f ? -p.y : p.y, az = p.z < 0.0f ? -p.z : p.z;
  return fmax_g(fmax_g(ax, ay), az);
}

SPTR_HD float cp_clamp01(float num, float den) {
  if (!(num > 0.0f) || !(den > 0.0f)) return 0.0f;
  const float t = num / den;
  return t < 1.0f ? t : 1.0f;
}
SPTR_HD CpCand cp_at(vec3 p, vec3 v0, vec3 ab, vec3 ac, float u, float v) {
  CpCand c;
  c.q = v0 + (ab * u + ac * v);
  const vec3 d = p - c.q;
  c.d2 = dot(d, d);
  c.u = u;
  c.v = v;
  return c;
}

SPTR_HD CpCand cp_triangle(vec3 v0, vec3 e1, vec3 e2, vec3 p) {
  const vec3 ab = -e1, ac = e2, bc = ac - ab, ap = p - v0, bp = ap - ab;
  const float aa = dot(ab, ab), apab = dot(ap, ab);
  CpCand best = cp_at(p, v0, ab, ac, cp_clamp01(apab, aa), 0.0f);
  {
    const CpCand c = cp_at(p, v0, ab, ac, 0.0f, cp_clamp01(dot(ap, ac), dot(ac, ac)));
    if (c.d2 < best.d2) best = c;
  }
  {
    const float t = cp_clamp01(dot(bp, bc), dot(bc, bc));
    const CpCand c = cp_at(p, v0, ab, ac, 1.0f - t, t);
    if (c.d2 < best.d2) best = c;
  }
  {
    const float alpha = dot(ab, ac) / aa;
    const vec3 ep = ac - ab * alpha;
    const float w = dot(ap, ep) / dot(ep, ep);
    const float s = apab / aa - alpha * w;
    if (s >= 0.0f && w >= 0.0f && s + w <= 1.0f) {
      const CpCand c = cp_at(p, v0, ab, ac, s, w);
      if (c.d2 < best.d2) best = c;
    }
  }
  return best;
}
// Which candidate won (sptr_query_signed_distance, pseudonormal.h): 0 = the face candidate, whatever its weights;
// 1, 2, 3 = edge ab, ac, bc, an edge candidate with 0 < t < 1; 4, 5, 6 = vertex a, b, c, an edge candidate with
// t == 0 or t == 1 (ab: 0 -> a, 1 -> b; ac: 0 -> a, 1 -> c; bc: 0 -> b, 1 -> c); 7 = a sphere; kCpMiss = none.
constexpr uint32_t kCpFace = 0u, kCpEdge = 1u, kCpVertex = 4u, kCpSphere = 7u, kCpMiss = 0xFFFFFFFFu;
SPTR_HD uint32_t cp_edge_feature(uint32_t edge, uint32_t lo, uint32_t hi, float t) {
  return t == 0.0f ? kCpVertex + lo : (t == 1.0f ? kCpVertex + hi : kCpEdge + edge);
}
// cp_triangle's candidate, bit for bit (the same expressions in the same order), and its feature code
SPTR_HD CpCand cp_triangle_feature(vec3 v0, vec3 e1, vec3 e2, vec3 p, uint32_t& feature) {
  const vec3 ab = -e1, ac = e2, bc = ac - ab, ap = p - v0, bp = ap - ab;
  const float aa = dot(ab, ab), apab = dot(ap, ab);
  const float t0 = cp_clamp01(apab, aa);
  CpCand best = cp_at(p, v0, ab, ac, t0, 0.0f);
  feature = cp_edge_feature(0u, 0u, 1u, t0);
  {
    const float t = cp_clamp01(dot(ap, ac), dot(ac, ac));
    const CpCand c = cp_at(p, v0, ab, ac, 0.0f, t);
    if (c.d2 < best.d2) {
      best = c;
      feature = cp_edge_feature(1u, 0u, 2u, t);
    }
  }
  {
    const float t = cp_clamp01(dot(bp, bc), dot(bc, bc));
    const CpCand c = cp_at(p, v0, ab, ac, 1.0f - t, t);
    if (c.d2 < best.d2) {
      best = c;
      feature = cp_edge_feature(2u, 1u, 2u, t);
    }
  }
  {
    const float alpha = dot(ab, ac) / aa;
    const vec3 ep = ac - ab * alpha;
    const float w = dot(ap, ep) / dot(ep, ep);
    const float s = apab / aa - alpha * w;
    if (s >= 0.0f && w >= 0.0f && s + w <= 1.0f) {
      const CpCand c = cp_at(p, v0, ab, ac, s, w);
      if (c.d2 < best.d2) {
        best = c;
        feature = kCpFace;
      }
    }
  }
  return best;
}
// a triangle whose stored normal is exactly zero is one the build leaves out of the tree: no candidate
SPTR_HD bool cp_triangle_live(vec3 ng) { return !(ng.x == 0.0f && ng.y == 0.0f && ng.z == 0.0f); }

SPTR_HD float cp_sphere_d2(vec3 c, float r, vec3 p) {
  const vec3 m = p - c;
  const float h = sq_root(dot(m, m)) - r;
  return h * h;
}
SPTR_HD CpCand cp_sphere(vec3 c, float r, vec3 p, vec3& ng) {
  const vec3 m = p - c;
  const float len = sq_root(dot(m, m)), h = len - r;
  CpCand o;
  o.d2 = h * h;
  o.q = len == 0.0f ? v3(c.x + r, c.y, c.z) : c + m * (r / len);
  o.u = 0.0f;
  o.v = 0.0f;
  ng = r > 0.0f ? v3((o.q.x - c.x) / r, (o.q.y - c.y) / r, (o.q.z - c.z) / r) : v3(0.0f, 0.0f, 0.0f);
  return o;
}

SPTR_HD float cp_node_bound(vec3 p, vec3 lo, vec3 hi, float M) {
  const float pad = M * kCpPad;
  const float ax = fmax_g(fmax_g(lo.x - p.x, p.x - hi.x) - pad, 0.0f);
  const float ay = fmax_g(fmax_g(lo.y - p.y, p.y - hi.y) - pad, 0.0f);
  const float az = fmax_g(fmax_g(lo.z - p.z, p.z - hi.z) - pad, 0.0f);
  return (ax * ax + ay * ay + az * az) * kCpShrink;
}

// plane q (0..255) of a wide node's axis grid: org + q 2^e with the step's biased exponent byte, one rounding
SPTR_HD float cp_wide_plane(float org, uint32_t ebyte, uint32_t q) {
  const uint32_t bits = ebyte << 23;
  float step;
  __builtin_memcpy(&step, &bits, 4);
  return (float)q * step + org;  // the product is exact
}

// does candidate (d2, geom, prim) come before (bd2, bgeom, bprim)?
SPTR_HD bool cp_key_less(float d2, uint32_t geom, uint32_t prim, float bd2, uint32_t bgeom, uint32_t bprim) {
  if (d2 < bd2) return true;
  if (!(d2 == bd2)) return false;
  return geom < bgeom || (geom == bgeom && prim < bprim);
}

}  // namespace sptr
