// test_pseudonormal.cpp — stand-alone checks of csrc/pseudonormal.h and cp_triangle_feature (closest_point.h), the
// text the table build, the sign pass and the host twins compile.  Built with -ffp-contract=off and
// -fsanitize=address,undefined by tests/test_signed_cpu.py.
//   pn_angle against atan2 in double: right, tiny, obtuse, near-0 and near-pi angles, vectors scaled from 1e-18 to
//     1e18; the error stays at most 2^-20 rad, zero vectors give 0; the worst case is printed
//   pn_unit_normal: finite, | |n| - 1 | <= 4 eps for triangles from 1e-15 to 1e15 in size
//   cp_triangle_feature: cp_triangle's CpCand bit for bit on 10^6 random and sliver cases; each feature code is
//     reached from a point placed in that feature's region
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pseudonormal.h"

using namespace sptr;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return uint32_t(g_rng >> 32);
}
static float urand() { return float(rnd() >> 8) / 16777216.0f; }       // [0, 1)
static float srand1() { return urand() * 2.0f - 1.0f; }                // [-1, 1)
static vec3 vrand() { return v3(srand1(), srand1(), srand1()); }

static int g_fail = 0;
#define CHECK(c, ...)                  \
  do {                                 \
    if (!(c)) {                        \
      if (g_fail < 20) {               \
        std::printf("FAIL %s: ", #c);  \
        std::printf(__VA_ARGS__);      \
        std::printf("\n");             \
      }                                \
      ++g_fail;                        \
    }                                  \
  } while (0)

static double angle64(vec3 a, vec3 b) {
  const double ax = a.x, ay = a.y, az = a.z, bx = b.x, by = b.y, bz = b.z;
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  // scaled so that neither the cross nor the dot product leaves double's range for 1e-18 .. 1e18 inputs
  return std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), ax * bx + ay * by + az * bz);
}

static double g_worst = 0.0;
static vec3 g_wa, g_wb;
static void angle_case(vec3 a, vec3 b) {
  const float got = pn_angle(a, b);
  const double want = angle64(a, b), err = std::fabs(double(got) - want);
  if (err > g_worst) {
    g_worst = err;
    g_wa = a;
    g_wb = b;
  }
  CHECK(got >= 0.0f && got <= 3.14159274f, "angle %g out of [0, pi]", double(got));
  CHECK(err <= 0x1p-20, "angle error %.3g (2^%.2f) a=(%g %g %g) b=(%g %g %g)", err, std::log2(err), double(a.x), double(a.y),
        double(a.z), double(b.x), double(b.y), double(b.z));
}

// b at angle th from a, in a random plane, lengths la and lb
static void angle_family(double th, float la, float lb) {
  vec3 a = vrand(), t = vrand();
  const float al = std::sqrt(dot(a, a));
  if (!(al > 0.1f)) return;
  a = a / al;
  vec3 n = cross(a, t);
  const float nl = std::sqrt(dot(n, n));
  if (!(nl > 0.1f)) return;
  n = n / nl;
  const vec3 w = cross(n, a);
  const vec3 b = a * float(std::cos(th)) + w * float(std::sin(th));
  angle_case(a * la, b * lb);
}

static void test_angles() {
  const float scales[] = {1e-18f, 1e-9f, 1e-3f, 1.0f, 37.5f, 1e6f, 1e18f};
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < 200000; ++i) {
    const float la = scales[rnd() % 7u] * (0.5f + urand()), lb = scales[rnd() % 7u] * (0.5f + urand());
    const int fam = i % 8;
    double th;
    if (fam == 0) th = pi * 0.5 + (urand() - 0.5) * 1e-3;            // right
    else if (fam == 1) th = urand() * 1e-3;                           // tiny
    else if (fam == 2) th = std::pow(10.0, -7.0 * urand());           // near 0 by decades
    else if (fam == 3) th = pi - std::pow(10.0, -7.0 * urand());      // near pi by decades
    else if (fam == 4) th = pi * (0.5 + 0.5 * urand());               // obtuse
    else if (fam == 5) th = pi * 0.25 + (urand() - 0.5) * 1e-2;       // around the reduction's thresholds
    else if (fam == 6) th = pi * 0.75 + (urand() - 0.5) * 1e-2;
    else th = pi * urand();
    angle_family(th, la, lb);
  }
  for (int i = 0; i < 100000; ++i) angle_case(vrand(), vrand());
  angle_case(v3(1, 0, 0), v3(1, 0, 0));
  angle_case(v3(1, 0, 0), v3(-1, 0, 0));
  angle_case(v3(1, 0, 0), v3(0, 1, 0));
  angle_case(v3(1e18f, 0, 0), v3(0, 1e-18f, 0));
  CHECK(pn_angle(v3(0, 0, 0), v3(1, 2, 3)) == 0.0f, "zero a");
  CHECK(pn_angle(v3(1, 2, 3), v3(0, 0, 0)) == 0.0f, "zero b");
  CHECK(pn_angle(v3(0, 0, 0), v3(-0.0f, 0, 0)) == 0.0f, "zero both");
  std::printf("pn_angle: worst error %.4g rad = 2^%.2f at a=(%.9g %.9g %.9g) b=(%.9g %.9g %.9g)\n", g_worst,
              std::log2(g_worst > 0 ? g_worst : 1e-300), double(g_wa.x), double(g_wa.y), double(g_wa.z), double(g_wb.x),
              double(g_wb.y), double(g_wb.z));
}

static void test_unit_normals() {
  double worst = 0.0;
  for (int i = 0; i < 200000; ++i) {
    const float s = float(std::pow(10.0, -15.0 + 30.0 * urand()));
    const vec3 v0 = vrand() * s, v1 = vrand() * s, v2 = vrand() * s;
    const vec3 ng = pn_tri_ng(v0, v1, v2);
    if (!cp_triangle_live(ng)) continue;
    const vec3 n = pn_unit_normal(ng);
    CHECK(pn_finite3(n), "unit normal not finite at scale %g", double(s));
    const double l = std::sqrt(double(n.x) * n.x + double(n.y) * n.y + double(n.z) * n.z);
    const double e = std::fabs(l - 1.0);
    if (e > worst) worst = e;
    CHECK(e <= 4.0 * 0x1p-24, "|n| - 1 = %g at scale %g", e, double(s));
  }
  std::printf("pn_unit_normal: worst | |n| - 1 | = %.3g eps\n", worst / 0x1p-24);
}

static bool same_bits(const CpCand& a, const CpCand& b) { return std::memcmp(&a, &b, sizeof(CpCand)) == 0; }

static void test_feature_bits() {
  uint64_t seen[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 1000000; ++i) {
    vec3 v0 = vrand(), v1 = vrand(), v2 = vrand();
    const int fam = i % 4;
    if (fam == 1) v2 = v0 + (v1 - v0) * urand() + vrand() * 1e-6f;  // sliver
    if (fam == 2) v1 = v0 + vrand() * 1e-5f;                        // short edge
    if (fam == 3) {                                                 // large and far
      v0 = v0 * 1e4f;
      v1 = v1 * 1e4f;
      v2 = v2 * 1e4f;
    }
    vec3 p = vrand() * (fam == 3 ? 2e4f : 2.0f);
    if ((i & 7) == 0) p = v0 + (v1 - v0) * urand();  // on an edge
    if ((i & 15) == 1) p = v1;                       // on a vertex
    const vec3 e1 = v0 - v1, e2 = v2 - v0;
    uint32_t f = 99u;
    CpCand a, b;
    std::memset(&a, 0, sizeof a);
    std::memset(&b, 0, sizeof b);
    a = cp_triangle(v0, e1, e2, p);
    b = cp_triangle_feature(v0, e1, e2, p, f);
    CHECK(same_bits(a, b), "case %d: candidates differ (d2 %a vs %a)", i, double(a.d2), double(b.d2));
    CHECK(f <= 6u, "case %d: feature %u", i, f);
    if (f <= 6u) ++seen[f];
    // the code agrees with the weights it came with
    if (f >= kCpVertex && f <= 6u) {
      const float wa = 1.0f - b.u - b.v;
      const bool at_a = b.u == 0.0f && b.v == 0.0f, at_b = b.u == 1.0f && b.v == 0.0f, at_c = b.u == 0.0f && b.v == 1.0f;
      CHECK((f == 4u && at_a) || (f == 5u && at_b) || (f == 6u && at_c), "case %d: vertex code %u with u %g v %g (wa %g)", i, f,
            double(b.u), double(b.v), double(wa));
    }
    if (f == 1u) CHECK(b.v == 0.0f && b.u > 0.0f && b.u < 1.0f, "case %d: edge ab with u %g v %g", i, double(b.u), double(b.v));
    if (f == 2u) CHECK(b.u == 0.0f && b.v > 0.0f && b.v < 1.0f, "case %d: edge ac with u %g v %g", i, double(b.u), double(b.v));
    if (f == 3u) CHECK(b.v > 0.0f && b.v < 1.0f, "case %d: edge bc with v %g", i, double(b.v));
  }
  std::printf("cp_triangle_feature: codes seen face %llu ab %llu ac %llu bc %llu a %llu b %llu c %llu\n",
              (unsigned long long)seen[0], (unsigned long long)seen[1], (unsigned long long)seen[2], (unsigned long long)seen[3],
              (unsigned long long)seen[4], (unsigned long long)seen[5], (unsigned long long)seen[6]);
}

static uint32_t feature_of(vec3 v0, vec3 v1, vec3 v2, vec3 p) {
  uint32_t f = 99u;
  (void)cp_triangle_feature(v0, v0 - v1, v2 - v0, p, f);
  return f;
}

static void test_feature_regions() {
  // a = (0,0,0), b = (1,0,0), c = (0,1,0): the seven Voronoi regions of the triangle, above its plane
  const vec3 a = v3(0, 0, 0), b = v3(1, 0, 0), c = v3(0, 1, 0);
  CHECK(feature_of(a, b, c, v3(0.25f, 0.25f, 0.5f)) == 0u, "face");
  CHECK(feature_of(a, b, c, v3(0.5f, -0.5f, 0.5f)) == 1u, "edge ab");
  CHECK(feature_of(a, b, c, v3(-0.5f, 0.5f, 0.5f)) == 2u, "edge ac");
  CHECK(feature_of(a, b, c, v3(1.0f, 1.0f, 0.5f)) == 3u, "edge bc");
  CHECK(feature_of(a, b, c, v3(-0.5f, -0.5f, 0.5f)) == 4u, "vertex a");
  CHECK(feature_of(a, b, c, v3(2.0f, -0.5f, 0.5f)) == 5u, "vertex b");
  CHECK(feature_of(a, b, c, v3(-0.5f, 2.0f, 0.5f)) == 6u, "vertex c");
  vec3 n;
  uint32_t f;
  const float nv[9] = {0, 0, 1, 0, 0, 2, 0, 0, 3}, ne[9] = {0, 0, 4, 0, 0, 5, 0, 0, 6};
  // Ng = cross(e2, e1) = cross(c - a, a - b) = (0, 0, 1) for this winding
  float s = pn_triangle_result(a, b, c, nv, ne, v3(0.25f, 0.25f, 0.5f), false, n, f);
  CHECK(f == 0u && n.z == 1.0f && s == 0.5f, "face result %g n.z %g", double(s), double(n.z));
  s = pn_triangle_result(a, b, c, nv, ne, v3(0.25f, 0.25f, -0.5f), false, n, f);
  CHECK(s == -0.5f, "below the face %g", double(s));
  s = pn_triangle_result(a, b, c, nv, ne, v3(0.25f, 0.25f, -0.5f), true, n, f);
  CHECK(s == 0.5f, "flipped %g", double(s));
  s = pn_triangle_result(a, b, c, nv, ne, v3(1.0f, 1.0f, 0.5f), false, n, f);
  CHECK(f == 3u && n.z == 6.0f && s > 0.0f, "edge bc takes ne[2]");
  s = pn_triangle_result(a, b, c, nv, ne, v3(2.0f, -0.5f, -0.5f), false, n, f);
  CHECK(f == 5u && n.z == 2.0f && s < 0.0f, "vertex b takes nv[1]");
  s = pn_sphere_result(v3(0, 0, 0), 1.0f, v3(0.5f, 0, 0), n);
  CHECK(s == -0.5f && n.x == 1.0f, "inside a sphere %g", double(s));
  s = pn_sphere_result(v3(0, 0, 0), 1.0f, v3(2.0f, 0, 0), n);
  CHECK(s == 1.0f, "outside a sphere %g", double(s));
}

int main() {
  test_angles();
  test_unit_normals();
  test_feature_bits();
  test_feature_regions();
  std::printf("pseudonormal: %d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
