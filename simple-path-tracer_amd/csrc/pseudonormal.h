// pseudonormal.h — the definition of sptr_query_signed_distance, for host and device: the angle-weighted
// pseudonormals of a triangle mesh (Baerentzen & Aanaes, "Signed distance computation using the angle weighted
// pseudonormal", 2005) and the sign they give a closest-point result.  The table build (kernels_signed.hip), the
// sign pass k_point_sign, the host twins (host/host_api.cpp) and tests/cpp/test_pseudonormal.cpp compile this
// text.  As in closest_point.h only + - *, IEEE / and sqrt and compares are used, each written out (the one fused
// operation is the explicit fma of the stored normal, as the build computes it); with -ffp-contract=off on both
// sides host and device give the same bits.  No libm or ocml function is called: they differ in the last bit.
//
// Triangles, corners, edges.  All indices are in uploaded order.  Corner 3t + k is vertex k of triangle t.  Edge 0
// of a triangle is v0v1, edge 1 is v0v2, edge 2 is v1v2: the order of cp_triangle's candidates.  A triangle is
// live if its stored Ng (pn_tri_ng, tri_ng3's expressions) is not exactly zero; others take no part anywhere.
//
// Unit normal n_t (pn_unit_normal): m = the largest absolute component of Ng, g = Ng / m per component,
// n = g / sqrt(g.g): no overflow or underflow for tiny or huge triangles.  If a component of n is not finite the
// triangle contributes nothing to any sum (it still counts as an incidence of its edges).
//
// Welding.  Two corners of live triangles are the same welded vertex iff they belong to the same geomID and their
// positions compare equal as floats in every component (pn_same_pos): -0 equals +0, a NaN equals nothing.
// pn_pos_bits gives the sort key of a component (-0 folded onto +0), so equal positions have equal keys.
//
// Vertex pseudonormal N_v: the float32 sum, started at 0, in ascending corner index, of angle_c * n_t over the
// corners of the welded vertex; angle_c = pn_angle(a, b) with a and b from the corner to the triangle's other two
// vertices in index order (pn_corner_angle).
//
// pn_angle(a, b) in [0, pi], 0 for a zero vector: Kahan's 2 atan(|ua - ub| / |ua + ub|) on the two vectors scaled
// by their largest components and normalised, the arctangent reduced to |z| <= tan(pi / 8) (swap to the
// reciprocal above 1, the (r - 1) / (r + 1) identity above tan(pi / 8)) and evaluated there by the odd Taylor
// polynomial to z^15 (truncation below 2^-25).  Its absolute error against float64 atan2 stays below 2^-20 rad
// (test_pseudonormal.cpp prints the worst case it finds).
//
// Edge pseudonormal N_e of an unordered pair of distinct welded vertices: the float32 sum, started at 0, in
// ascending (t, k), of n_t over the live triangles that have that pair as edge k.
//
// Sign (pn_signed): N = the winner's stored Ng (face), N_e or N_v by cp_triangle_feature's code, d = p - q with
// the query's output point q, s = (d.x N.x + d.y N.y) + d.z N.z; signed_dist = -dist if s < 0, else +dist, so 0
// and NaN count as positive; `flip` negates that choice.  Positive on the side the normals point to.
#pragma once
#include <stdint.h>

#include "closest_point.h"
#include "sptr_math.h"

namespace sptr {

// tri_ng3 (lbvh_shared.h): Embree's Ng = cross(e2, e1) in msub form
SPTR_HD vec3 pn_tri_ng(vec3 v0, vec3 v1, vec3 v2) {
  const vec3 e1 = v0 - v1, e2 = v2 - v0;
  return v3(__builtin_fmaf(e2.y, e1.z, -(e2.z * e1.y)), __builtin_fmaf(e2.z, e1.x, -(e2.x * e1.z)),
            __builtin_fmaf(e2.x, e1.y, -(e2.y * e1.x)));
}

SPTR_HD bool pn_finite3(vec3 v) { return cp_finite(v.x) && cp_finite(v.y) && cp_finite(v.z); }

// v scaled by its largest absolute component and normalised; the caller checks the result with pn_finite3
SPTR_HD vec3 pn_unit(vec3 v, float m) {
  const vec3 g = v3(v.x / m, v.y / m, v.z / m);
  const float l = sq_root(dot(g, g));
  return v3(g.x / l, g.y / l, g.z / l);
}
SPTR_HD vec3 pn_unit_normal(vec3 ng) { return pn_unit(ng, cp_abs_max(ng)); }

constexpr float kPnTanPi8 = 0x1.a8279ap-2f;   // tan(pi / 8) = sqrt(2) - 1
constexpr float kPnPio2Hi = 0x1.921fb6p+0f;   // pi / 2 = hi + lo
constexpr float kPnPio2Lo = -0x1.777a5cp-25f;
constexpr float kPnPio4Hi = 0x1.921fb6p-1f;   // pi / 4 = hi + lo
constexpr float kPnPio4Lo = -0x1.777a5cp-26f;

// atan(y / x) for y >= 0, x >= 0, not both 0: in [0, pi / 2]
SPTR_HD float pn_atan_quadrant(float y, float x) {
  const bool swap = y > x;
  const float r = swap ? x / y : y / x;  // [0, 1]
  const bool big = r > kPnTanPi8;
  const float z = big ? (r - 1.0f) / (r + 1.0f) : r;  // |z| <= tan(pi / 8)
  const float z2 = z * z;
  float c = 1.0f / 15.0f;
  c = c * z2;
  c = 1.0f / 13.0f - c;
  c = c * z2;
  c = 1.0f / 11.0f - c;
  c = c * z2;
  c = 1.0f / 9.0f - c;
  c = c * z2;
  c = 1.0f / 7.0f - c;
  c = c * z2;
  c = 1.0f / 5.0f - c;
  c = c * z2;
  c = 1.0f / 3.0f - c;
  c = c * z2;  // z^2 / 3 - z^4 / 5 + ...
  const float zc = z * c;
  float a = z - zc;
  if (big) {
    a = kPnPio4Hi + a;
    a = a + kPnPio4Lo;
  }
  if (swap) {
    a = kPnPio2Hi - a;
    a = a + kPnPio2Lo;
  }
  return a;
}

// the angle between a and b, in [0, pi]; 0 when either is zero
SPTR_HD float pn_angle(vec3 a, vec3 b) {
  const float ma = cp_abs_max(a), mb = cp_abs_max(b);
  if (!(ma > 0.0f) || !(mb > 0.0f)) return 0.0f;
  const vec3 ua = pn_unit(a, ma), ub = pn_unit(b, mb);
  const vec3 d = ua - ub, s = ua + ub;
  const float y = sq_root(dot(d, d)), x = sq_root(dot(s, s));
  if (y == 0.0f && x == 0.0f) return 0.0f;
  const float h = pn_atan_quadrant(y, x);
  return h + h;
}
// the triangle's angle at corner k
SPTR_HD float pn_corner_angle(vec3 v0, vec3 v1, vec3 v2, uint32_t k) {
  if (k == 0u) return pn_angle(v1 - v0, v2 - v0);
  if (k == 1u) return pn_angle(v0 - v1, v2 - v1);
  return pn_angle(v0 - v2, v1 - v2);
}

// corners of edge k of a triangle (0 = v0v1, 1 = v0v2, 2 = v1v2)
SPTR_HD uint32_t pn_edge_lo(uint32_t k) { return k == 2u ? 1u : 0u; }
SPTR_HD uint32_t pn_edge_hi(uint32_t k) { return k == 0u ? 1u : 2u; }

// does the triangle's boundary (v0 -> v1 -> v2 -> v0) run from the edge's smaller welded id to its larger one?
// (edge 1 is v0v2, which the boundary runs as v2 -> v0)
SPTR_HD bool pn_edge_forward(uint32_t k, uint32_t wlo, uint32_t whi) { return (wlo < whi) != (k == 1u); }

SPTR_HD bool pn_same_pos(vec3 a, vec3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// sort key of a coordinate: its bits, -0 as +0 (any order that puts equal floats together serves)
SPTR_HD uint32_t pn_pos_bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u == 0x80000000u ? 0u : u;
}
constexpr uint64_t kPnDeadKey = 0xFFFFFFFFFFFFFFFFull;  // corners and edges of triangles that are not live sort last
SPTR_HD uint64_t pn_edge_key(uint32_t wa, uint32_t wb) {
  if (wa == wb) return kPnDeadKey;  // not a pair of distinct vertices: no edge
  return wa < wb ? ((uint64_t)wa << 32) | wb : ((uint64_t)wb << 32) | wa;
}

// the sign of a triangle result: d = p - q
SPTR_HD float pn_signed(vec3 p, vec3 q, vec3 n, float dist, bool flip) {
  const vec3 d = p - q;
  const float s = (d.x * n.x + d.y * n.y) + d.z * n.z;
  const bool neg = (s < 0.0f) != flip;
  return neg ? -dist : dist;
}
// The whole result of a triangle winner from its three corners and its six table entries (nv3, ne3: 3 x 3 floats
// each, corner k and edge k of this triangle).
SPTR_HD float pn_triangle_result(vec3 v0, vec3 v1, vec3 v2, const float* nv3, const float* ne3, vec3 p, bool flip, vec3& n,
                                 uint32_t& feature) {
  const CpCand c = cp_triangle_feature(v0, v0 - v1, v2 - v0, p, feature);
  if (feature == kCpFace) {
    n = pn_tri_ng(v0, v1, v2);
  } else {
    const float* t = feature < kCpVertex ? ne3 + 3u * (feature - kCpEdge) : nv3 + 3u * (feature - kCpVertex);
    n = v3(t[0], t[1], t[2]);
  }
  return pn_signed(p, c.q, n, sq_root(c.d2), flip);
}
// ... and of a sphere winner: negative iff |p - c| < r, N = ng
SPTR_HD float pn_sphere_result(vec3 c, float r, vec3 p, vec3& n) {
  const CpCand o = cp_sphere(c, r, p, n);
  const vec3 m = p - c;
  const float len = sq_root(dot(m, m)), dist = sq_root(o.d2);
  return len < r ? -dist : dist;
}

}  // namespace sptr
