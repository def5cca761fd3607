// cull_prims.h — exact primitive tests of the bounce-0 pixel cull (k_cull), for host and device.
//
// A pixel quad's camera rays start at the apex o and run inside the pyramid spanned by four corner
// directions (already widened by the cull's pixel margin).  cull_sphere_outside / cull_triangle_outside
// answer "no such ray can hit this primitive".  They only ever err towards "may touch": every
// comparison carries a relative slack (kCullPrimSlack, the cull's kCullSlack) and an absolute bound on
// the float rounding of the operands, and a NaN makes every comparison false (not outside).
//
//   sphere   : distance of the centre to the pyramid's bounding cone (axis = centre direction,
//              half-angle covering the four corners) and to the four side planes, against the radius.
//              The four planes alone leave the corner regions of the sphere's bounding square.
//              The cone test is a test of directions about the apex, so it also covers a sphere that
//              reaches behind the apex; a sphere that holds the apex, or nearly, is never outside.
//   triangle : a separating plane through the apex: one of the four side planes (all three vertices
//              outside) or one of the three planes through the apex and an edge (all four corners on
//              the side away from the third vertex).  A triangle not strictly in front of the apex
//              (along the axis) is never outside; an edge plane that degenerates (edge in line with
//              the apex, zero-area triangle) is skipped.
//
// The radius is inflated by what the float discriminant of the renderer's sphere test can add:
// disc = b^2 - 4ac carries an error of up to ~3.5e-6 d^2 (d: distance of the centre), as if the
// radius were sqrt(R^2 + 1e-6 d^2) — nothing for the scene's unit spheres, about a pixel for a
// zero-radius sphere, which a ray "hits" whenever rounding brings disc to 0.
#pragma once
#include "sptr_math.h"

namespace sptr {

constexpr float kCullPrimSlack = 1e-4f;   // relative, on plane distances (== kCullSlack)
constexpr float kCullPrimRound = 1e-6f;   // absolute rounding bound, relative to the operands' lengths

struct CullPyramid {
  vec3 o;       // apex
  vec3 c[4];    // corner directions in order around the pyramid (any length)
  float cl[4];  // their lengths
  vec3 n[4];    // unit inward normals: side plane k holds c[k] and c[(k + 1) & 3]
  vec3 axis;    // unit centre direction
  float cos_h, sin_h;  // bounding cone about axis: covers the four corners
  float ol;     // |o|_1: the rounding of (vertex - o) is relative to the larger operand
};

SPTR_HD float cull_abs(float x) { return x < 0.0f ? -x : x; }
SPTR_HD float cull_len(vec3 v) { return sq_root(dot(v, v)); }
SPTR_HD float cull_mag(vec3 a, vec3 b) { return cull_abs(a.x * b.x) + cull_abs(a.y * b.y) + cull_abs(a.z * b.z); }

SPTR_HD CullPyramid cull_pyramid(vec3 o, vec3 c0, vec3 c1, vec3 c2, vec3 c3) {
  CullPyramid p;
  p.o = o;
  p.ol = cull_abs(o.x) + cull_abs(o.y) + cull_abs(o.z);
  p.c[0] = c0;
  p.c[1] = c1;
  p.c[2] = c2;
  p.c[3] = c3;
  const vec3 sum = (c0 + c1) + (c2 + c3);
  p.axis = sum * (1.0f / cull_len(sum));
  float cmin = 1.0f, smax = 0.0f;
  for (int k = 0; k < 4; ++k) {
    p.cl[k] = cull_len(p.c[k]);
    const float inv = 1.0f / p.cl[k];
    const float ck = dot(p.axis, p.c[k]) * inv;
    const float sk = cull_len(cross(p.axis, p.c[k])) * inv;
    cmin = ck < cmin ? ck : cmin;
    smax = sk > smax ? sk : smax;
  }
  // (cos from the smallest cosine, sin from the largest sine: each errs towards a wider cone)
  p.cos_h = cmin;
  p.sin_h = smax;
  for (int k = 0; k < 4; ++k) {
    vec3 n = cross(p.c[k], p.c[(k + 1) & 3]);
    if (dot(n, p.c[(k + 2) & 3]) < 0.0f) n = -n;  // inward
    p.n[k] = n * (1.0f / cull_len(n));
  }
  return p;
}

// no ray of the pyramid can hit the sphere (centre C, radius R)
SPTR_HD bool cull_sphere_outside(const CullPyramid& p, vec3 C, float R) {
  const vec3 v = C - p.o;
  const float d2 = dot(v, v);
  const float d = sq_root(d2);
  const float cl1 = cull_abs(C.x) + cull_abs(C.y) + cull_abs(C.z);
  const float round = kCullPrimRound * (d + p.ol + cl1);
  const float Re = sq_root(R * R + 1e-6f * d2) + round;
  if (!(d > 1.001f * Re + round)) return false;  // the apex is inside the sphere, or near it
  // bounding cone: with theta the angle between axis and v, s = d sin(theta), a = d cos(theta);
  // d sin(theta - h) is the centre's distance to the cone wherever theta - h <= pi/2, and below the
  // true distance (d, to the apex) beyond
  const float a = dot(p.axis, v);
  const float s = cull_len(cross(p.axis, v));
  const float dist = s * p.cos_h - a * p.sin_h;
  const float slack = kCullPrimSlack * (Re + cull_abs(s * p.cos_h) + cull_abs(a * p.sin_h)) + round;
  if (dist > Re + slack) return true;
  // theta - h well beyond pi/2: the apex is the cone's nearest point, at d > Re
  if (a * p.cos_h + s * p.sin_h < -1e-3f * d) return true;
  // side planes
  for (int k = 0; k < 4; ++k) {
    const float dk = dot(p.n[k], v);
    if (dk < -(Re + kCullPrimSlack * (Re + cull_mag(p.n[k], v)) + round)) return true;
  }
  return false;
}

// no ray of the pyramid can hit the triangle (v0, v1, v2)
SPTR_HD bool cull_triangle_outside(const CullPyramid& p, vec3 v0, vec3 v1, vec3 v2) {
  const vec3 q[3] = {v0 - p.o, v1 - p.o, v2 - p.o};
  float ql[3];
  for (int j = 0; j < 3; ++j) {
    ql[j] = cull_len(q[j]) + p.ol;  // length the rounding of q[j] is relative to
    if (!(dot(p.axis, q[j]) > kCullPrimRound * ql[j])) return false;  // not strictly in front
  }
  for (int k = 0; k < 4; ++k) {  // side planes: all three vertices outside one of them
    bool out = true;
    for (int j = 0; j < 3; ++j) {
      const float dj = dot(p.n[k], q[j]);
      out = out && dj < -(kCullPrimSlack * cull_mag(p.n[k], q[j]) + kCullPrimRound * ql[j]);
    }
    if (out) return true;
  }
  for (int i = 0; i < 3; ++i) {  // edge planes: all four corners on the side away from the third vertex
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    const vec3 m = cross(q[i], q[i1]);
    const float ab = ql[i] * ql[i1];  // |m| <= ab, and m's rounding <= kCullPrimRound * ab
    const float sw = dot(m, q[i2]);
    if (!(cull_abs(sw) > kCullPrimSlack * cull_mag(m, q[i2]) + kCullPrimRound * ab * ql[i2])) continue;  // degenerate
    const float sg = sw > 0.0f ? 1.0f : -1.0f;
    bool out = true;
    for (int k = 0; k < 4; ++k) {
      const float dk = sg * dot(m, p.c[k]);
      out = out && dk < -(kCullPrimSlack * cull_mag(m, p.c[k]) + kCullPrimRound * ab * p.cl[k]);
    }
    if (out) return true;
  }
  return false;
}

}  // namespace sptr
