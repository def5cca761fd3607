// The definition of sptr_query_points (csrc/closest_point.h) on the host: the text k_pointquery calls.
//
// Soundness of the bound, the inequality the walk relies on: for (primitive, point) pairs of several families,
// cp_node_bound(p, box, M) <= the candidate's d2, for the primitive's exact box (tri_box: the min / max of its
// vertices; sphere_box: c -+ r in float32) and for that box after the wide node's quantisation (quantize_wide's
// rule in csrc/lbvh_shared.h: per axis org = the parent's lower plane, step 2^e the smallest power of two with
// extent <= 255 * 2^e, qlo = floor, qhi = ceil, in double) and float32 decode (cp_wide_plane), inside parents of
// random sizes.  M is the smallest the kernel may use: max(|p|_inf, the box's largest absolute coordinate).
// Families: well-shaped triangles (edges ~0.5, points from on the surface to ~3 edge lengths away), slivers of
// relative width 10^-7 .. 10^-1, both offset by 10^3 and scaled by 10^-3, zero-length edges, points on vertices,
// on edges, on box faces and inside the box, spheres with points anywhere and at the centre.
// Also: the weights are finite and convex, d2 is that of the returned q, validity and key order.
// Prints the number of pairs and the smallest slack sqrt(d2) - sqrt(bound) in eps M (eps = 2^-24) over the pairs
// whose bound is positive, and the largest excess of the unpadded box distance over sqrt(d2).  The exit status is the number of failures.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "closest_point.h"

using namespace sptr;

static int fails = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      if (fails < 20) std::printf("FAIL line %d: %s\n", __LINE__, #c); \
      ++fails;                                                         \
    }                                                                  \
  } while (0)

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static double rnd() {  // [0, 1)
  rs ^= rs << 13;
  rs ^= rs >> 7;
  rs ^= rs << 17;
  return double(rs >> 11) * (1.0 / 9007199254740992.0);
}
static double uni(double a, double b) { return a + (b - a) * rnd(); }

struct D3 {
  double x, y, z;
};
static D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static D3 mul(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static D3 crs(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double len(D3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
static D3 rnd3(double r) { return {uni(-r, r), uni(-r, r), uni(-r, r)}; }
static vec3 f3(D3 a) { return v3(float(a.x), float(a.y), float(a.z)); }
static D3 d3(vec3 a) { return {a.x, a.y, a.z}; }

static const double kEps = std::ldexp(1.0, -24);
static double min_slack[2] = {1e300, 1e300}, max_raw_excess[2] = {0.0, 0.0};
static uint64_t pairs = 0, positive[2] = {0, 0};

static float box_abs_max(vec3 lo, vec3 hi) { return fmax_g(cp_abs_max(lo), cp_abs_max(hi)); }

// quantize_wide's rule for one child box inside a parent's extent on one axis, then the float32 decode
static void quantised_axis(float lo, float hi, float plo, float phi, float& qlo_f, float& qhi_f) {
  const double ext = double(phi) - double(plo);
  int e = -100;
  if (ext > 0.0) {
    int x;
    (void)std::frexp(ext / 255.0, &x);
    e = x;
    if (ext <= 255.0 * std::ldexp(1.0, e - 1)) --e;
    e = e < -100 ? -100 : (e > 60 ? 60 : e);
  }
  const double inv_step = std::ldexp(1.0, -e);
  double l = std::floor((double(lo) - double(plo)) * inv_step), h = std::ceil((double(hi) - double(plo)) * inv_step);
  l = l < 0.0 ? 0.0 : (l > 255.0 ? 255.0 : l);
  h = h < 0.0 ? 0.0 : (h > 255.0 ? 255.0 : h);
  qlo_f = cp_wide_plane(plo, uint32_t(e + 127), uint32_t(l));
  qhi_f = cp_wide_plane(plo, uint32_t(e + 127), uint32_t(h));
}

static void check_bound(vec3 p, vec3 lo, vec3 hi, float d2) {
  ++pairs;
  // a parent around the box: grown on each side by 0 .. 8 extents (0: the box is its parent's whole extent)
  vec3 plo = lo, phi = hi;
  const float gx = float(uni(0.0, 8.0) * (rnd() < 0.3 ? 0.0 : 1.0)) * (hi.x - lo.x + 1e-3f);
  const float gy = float(uni(0.0, 8.0) * (rnd() < 0.3 ? 0.0 : 1.0)) * (hi.y - lo.y + 1e-3f);
  const float gz = float(uni(0.0, 8.0) * (rnd() < 0.3 ? 0.0 : 1.0)) * (hi.z - lo.z + 1e-3f);
  plo = v3(lo.x - gx * float(rnd()), lo.y - gy * float(rnd()), lo.z - gz * float(rnd()));
  phi = v3(hi.x + gx * float(rnd()), hi.y + gy * float(rnd()), hi.z + gz * float(rnd()));
  vec3 qlo, qhi;
  quantised_axis(lo.x, hi.x, plo.x, phi.x, qlo.x, qhi.x);
  quantised_axis(lo.y, hi.y, plo.y, phi.y, qlo.y, qhi.y);
  quantised_axis(lo.z, hi.z, plo.z, phi.z, qlo.z, qhi.z);
  const vec3 los[2] = {lo, qlo}, his[2] = {hi, qhi};
  for (int k = 0; k < 2; ++k) {
    const float M = fmax_g(cp_abs_max(p), box_abs_max(los[k], his[k]));
    const float b = cp_node_bound(p, los[k], his[k], M);
    CHECK(b <= d2);
    if (!(b <= d2) && fails < 20)
      std::printf("  kind %d p %.9g %.9g %.9g box %.9g %.9g %.9g .. %.9g %.9g %.9g bound %.9g d2 %.9g\n", k, p.x, p.y, p.z,
                  los[k].x, los[k].y, los[k].z, his[k].x, his[k].y, his[k].z, b, d2);
    {  // what the pad is for: the unpadded box distance (double, from the float planes) may exceed the candidate's
      const double gx2 = std::max(std::max(double(los[k].x) - p.x, double(p.x) - his[k].x), 0.0);
      const double gy2 = std::max(std::max(double(los[k].y) - p.y, double(p.y) - his[k].y), 0.0);
      const double gz2 = std::max(std::max(double(los[k].z) - p.z, double(p.z) - his[k].z), 0.0);
      const double raw = std::sqrt(gx2 * gx2 + gy2 * gy2 + gz2 * gz2);
      max_raw_excess[k] = std::max(max_raw_excess[k], (raw - std::sqrt(double(d2))) / (kEps * double(M)));
    }
    if (b > 0.0f) {
      ++positive[k];
      const double s = (std::sqrt(double(d2)) - std::sqrt(double(b))) / (kEps * double(M));
      min_slack[k] = std::min(min_slack[k], s);
    }
  }
}

static void check_triangle(D3 a, D3 b, D3 c, D3 pd) {
  const vec3 v0 = f3(a), v1 = f3(b), v2 = f3(c), p = f3(pd);
  const vec3 e1 = v0 - v1, e2 = v2 - v0;  // tri_record
  const CpCand r = cp_triangle(v0, e1, e2, p);
  CHECK(cp_finite(r.u) && cp_finite(r.v) && r.u >= 0.0f && r.v >= 0.0f && r.u <= 1.0f && r.v <= 1.0f);
  CHECK(r.u + r.v <= 1.0f + 0x1p-23f);
  const vec3 d = p - r.q;
  CHECK(r.d2 == dot(d, d));
  const vec3 lo = v3(std::fmin(v0.x, std::fmin(v1.x, v2.x)), std::fmin(v0.y, std::fmin(v1.y, v2.y)), std::fmin(v0.z, std::fmin(v1.z, v2.z)));
  const vec3 hi = v3(std::fmax(v0.x, std::fmax(v1.x, v2.x)), std::fmax(v0.y, std::fmax(v1.y, v2.y)), std::fmax(v0.z, std::fmax(v1.z, v2.z)));
  check_bound(p, lo, hi, r.d2);
}

// the points of one triangle: free, on the surface, on vertices, on edges, on box faces, inside the box
static void triangle_points(D3 a, D3 b, D3 c, D3 shift, double scale, int per_kind) {
  auto T = [&](D3 x) { return mul(add(x, shift), scale); };
  const D3 A = T(a), B = T(b), C = T(c);
  const double el = std::max(len(sub(B, A)), std::max(len(sub(C, B)), len(sub(A, C)))) + 1e-30;
  const D3 v[3] = {d3(f3(A)), d3(f3(B)), d3(f3(C))};
  D3 lo = v[0], hi = v[0];
  for (int k = 1; k < 3; ++k) {
    lo = {std::min(lo.x, v[k].x), std::min(lo.y, v[k].y), std::min(lo.z, v[k].z)};
    hi = {std::max(hi.x, v[k].x), std::max(hi.y, v[k].y), std::max(hi.z, v[k].z)};
  }
  for (int i = 0; i < per_kind; ++i) {
    const double r1 = std::sqrt(rnd()), r2 = rnd();
    const D3 s = add(add(mul(A, 1.0 - r1), mul(B, r1 * (1.0 - r2))), mul(C, r1 * r2));
    D3 n = crs(sub(B, A), sub(C, A));
    const double nl = len(n);
    n = nl > 0.0 ? mul(n, 1.0 / nl) : D3{0.0, 0.0, 1.0};
    check_triangle(A, B, C, add(s, mul(rnd3(1.0), 3.0 * el)));                              // free
    check_triangle(A, B, C, add(s, mul(n, (rnd() < 0.5 ? -1.0 : 1.0) * el * std::pow(10.0, uni(-7.0, 0.5)))));  // off the surface
    check_triangle(A, B, C, s);                                                             // on it
    check_triangle(A, B, C, v[i % 3]);                                                      // a vertex
    check_triangle(A, B, C, add(mul(v[i % 3], 0.5), mul(v[(i + 1) % 3], 0.5)));             // an edge
    D3 q = {uni(lo.x - el, hi.x + el), uni(lo.y - el, hi.y + el), uni(lo.z - el, hi.z + el)};
    const int ax = i % 3;
    const double plane = (i & 1) ? (ax == 0 ? hi.x : ax == 1 ? hi.y : hi.z) : (ax == 0 ? lo.x : ax == 1 ? lo.y : lo.z);
    (ax == 0 ? q.x : ax == 1 ? q.y : q.z) = plane;
    check_triangle(A, B, C, q);                                                             // a box face's plane
    check_triangle(A, B, C, {uni(lo.x, hi.x), uni(lo.y, hi.y), uni(lo.z, hi.z)});           // inside the box
    check_triangle(A, B, C, add(s, mul(rnd3(1.0), el * std::pow(10.0, uni(-6.0, 0.0)))));   // near
  }
}

static void triangles(int count, int per_kind) {
  const D3 shifts[3] = {{0, 0, 0}, {1e3, 1e3, 1e3}, {0, 0, 0}};
  const double scales[3] = {1.0, 1.0, 1e-3};
  for (int t = 0; t < count; ++t) {
    const D3 ctr = rnd3(1.0);
    const D3 a = add(ctr, rnd3(0.25)), b = add(ctr, rnd3(0.25));
    D3 c = add(ctr, rnd3(0.25));
    const int shape = t % 4;
    if (shape == 1 || shape == 2) {  // a sliver: c at relative width w off the line a b
      const D3 ab = sub(b, a);
      D3 perp = crs(ab, rnd3(1.0));
      const double pl = len(perp);
      perp = pl > 0.0 ? mul(perp, 1.0 / pl) : D3{0.0, 0.0, 0.0};
      const double w = std::pow(10.0, uni(-7.0, -1.0));
      c = add(add(a, mul(ab, uni(-0.2, 1.2))), mul(perp, w * len(ab)));
    }
    const int fr = t % 3;
    if (shape == 3 && (t % 8) == 3) {  // zero-length edges
      const int which = (t / 8) % 4;
      // (a, a, c), (a, b, b), (a, b, a), (a, a, a)
      triangle_points(a, (which == 0 || which == 3) ? a : b, which == 0 ? c : which == 1 ? b : a, shifts[fr], scales[fr], per_kind);
      continue;
    }
    triangle_points(a, b, c, shifts[fr], scales[fr], per_kind);
  }
}

static void spheres(int count, int per) {
  for (int t = 0; t < count; ++t) {
    const double scale = (t % 3) == 2 ? 1e-3 : 1.0, shift = (t % 3) == 1 ? 1e3 : 0.0;
    const D3 cd = mul(add(rnd3(1.0), D3{shift, shift, shift}), scale);
    const float r = (t % 16) == 0 ? 0.0f : float(uni(0.01, 0.5) * scale);
    const vec3 c = f3(cd);
    const vec3 lo = v3(c.x - r, c.y - r, c.z - r), hi = v3(c.x + r, c.y + r, c.z + r);  // sphere_box
    for (int i = 0; i < per; ++i) {
      vec3 p;
      const int kind = i % 4;
      if (kind == 0) p = c;  // at the centre
      else if (kind == 1) p = f3(add(d3(c), mul(rnd3(1.0), 3.0 * scale)));
      else if (kind == 2) {  // near the surface
        D3 d = rnd3(1.0);
        d = mul(d, 1.0 / (len(d) + 1e-300));
        p = f3(add(d3(c), mul(d, double(r) * (1.0 + (rnd() < 0.5 ? -1.0 : 1.0) * std::pow(10.0, uni(-7.0, 0.0))))));
      } else p = v3(float(uni(lo.x, hi.x)), float(uni(lo.y, hi.y)), float(uni(lo.z, hi.z)));
      vec3 ng;
      const CpCand s = cp_sphere(c, r, p, ng);
      CHECK(s.d2 == cp_sphere_d2(c, r, p));
      CHECK(cp_finite(s.q.x) && cp_finite(s.q.y) && cp_finite(s.q.z) && cp_finite(ng.x) && cp_finite(ng.y) && cp_finite(ng.z));
      CHECK(s.u == 0.0f && s.v == 0.0f);
      if (kind == 0) CHECK(s.q.x == c.x + r && s.q.y == c.y && s.q.z == c.z && s.d2 == r * r);
      check_bound(p, lo, hi, s.d2);
    }
  }
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  CHECK(cp_point_valid(v3(1, 2, 3), 0.0f) && cp_point_valid(v3(1, 2, 3), inf) && cp_point_valid(v3(-3e38f, 0, 0), 1.0f));
  CHECK(!cp_point_valid(v3(1, 2, 3), -1.0f) && !cp_point_valid(v3(1, 2, 3), nan) && !cp_point_valid(v3(inf, 2, 3), 1.0f));
  CHECK(!cp_point_valid(v3(1, -inf, 3), 1.0f) && !cp_point_valid(v3(1, 2, nan), 1.0f));
  CHECK(cp_key_less(1.0f, 5, 5, 2.0f, 0, 0) && !cp_key_less(2.0f, 0, 0, 1.0f, 5, 5));
  CHECK(cp_key_less(1.0f, 1, 9, 1.0f, 2, 0) && cp_key_less(1.0f, 1, 3, 1.0f, 1, 4) && !cp_key_less(1.0f, 1, 4, 1.0f, 1, 4));
  CHECK(cp_key_less(inf, 0, 0, inf, 0xFFFFFFFFu, 0xFFFFFFFFu) && !cp_key_less(nan, 0, 0, 1.0f, 1, 1));
  CHECK(!cp_triangle_live(v3(0.0f, -0.0f, 0.0f)) && cp_triangle_live(v3(0.0f, 1e-45f, 0.0f)));
  CHECK(cp_clamp01(nan, 1.0f) == 0.0f && cp_clamp01(1.0f, 0.0f) == 0.0f && cp_clamp01(inf, 1.0f) == 1.0f && cp_clamp01(1.0f, 4.0f) == 0.25f);
  CHECK(cp_wide_plane(1.5f, 127u, 3u) == 4.5f && cp_wide_plane(-2.0f, 125u, 255u) == 61.75f);
  triangles(36000, 7);  // 36000 x 7 x 8 = 2 016 000 pairs
  spheres(8000, 8);
  std::printf("closest_point: %llu pairs, bound positive on %llu (exact box) and %llu (quantised box)\n",
              (unsigned long long)pairs, (unsigned long long)positive[0], (unsigned long long)positive[1]);
  std::printf("closest_point: smallest slack %.3f eps M (exact box), %.3f eps M (quantised box)\n", min_slack[0], min_slack[1]);
  std::printf("closest_point: the unpadded box distance exceeds the candidate's by at most %.3f eps M (exact box), %.3f eps M "
              "(quantised box); the pad is %.0f eps M\n", max_raw_excess[0], max_raw_excess[1], double(kCpPad) / kEps);
  std::printf("closest_point: %d failures\n", fails);
  return fails > 255 ? 255 : fails;
}
