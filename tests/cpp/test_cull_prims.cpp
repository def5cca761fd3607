// Unit test of the bounce-0 cull's exact primitive tests (simple-path-tracer_amd/csrc/cull_prims.h),
// compiled with g++ by tests/test_cull_prims_cpu.py.
//
// Soundness: for every seeded case that a predicate reports "outside", a dense bundle of float64
// rays through the pyramid (a 17 x 17 grid over the quad, corners and edges included) is tested
// exactly against the primitive: no ray may hit.  The pyramid handed to the predicate is the bare one
// (no pixel margin), so the predicates' own slack has to carry their float rounding.
// Not vacuous: primitives clearly separated from the pyramid (more than two pixel widths) must be
// reported outside, and the seeded families must report a fair share outside.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "cull_prims.h"

using namespace sptr;

static int fails = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      if (fails++ < 10) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);   \
    }                                                                             \
  } while (0)

struct D3 {
  double x, y, z;
};
static D3 d3(vec3 v) { return D3{v.x, v.y, v.z}; }
static D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static D3 operator*(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
static double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static D3 dcross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// exact tests of the half-line o + t d, t > 0
static bool ray_sphere(D3 o, D3 d, D3 c, double r) {
  const D3 oc = o - c;
  const double a = ddot(d, d), b = ddot(oc, d), cc = ddot(oc, oc) - r * r;
  const double disc = b * b - a * cc;
  if (disc < 0.0) return false;
  return (-b + std::sqrt(disc)) / a > 0.0;  // the far root in front of the origin
}
static bool ray_triangle(D3 o, D3 d, D3 v0, D3 v1, D3 v2) {
  const D3 e1 = v1 - v0, e2 = v2 - v0, pv = dcross(d, e2);
  const double det = ddot(e1, pv);
  if (det == 0.0) return false;
  const D3 tv = o - v0, qv = dcross(tv, e1);
  const double u = ddot(tv, pv) / det, v = ddot(d, qv) / det, t = ddot(e2, qv) / det;
  return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t > 0.0;
}

struct Pyr {
  vec3 o, f, r, u;  // apex, axis, right, up (unit), and the half extents
  float hw, hh;
  vec3 c[4];
  CullPyramid p;
};
static constexpr int kGrid = 17;
template <class Hit>
static bool any_ray_hits(const Pyr& q, Hit&& hit) {
  const D3 c0 = d3(q.c[0]), c1 = d3(q.c[1]), c2 = d3(q.c[2]), c3 = d3(q.c[3]);
  for (int i = 0; i < kGrid; ++i)
    for (int j = 0; j < kGrid; ++j) {
      const double s = double(i) / (kGrid - 1), t = double(j) / (kGrid - 1);
      const D3 d = (c0 * (1 - s) + c1 * s) * (1 - t) + (c3 * (1 - s) + c2 * s) * t;
      if (hit(d3(q.o), d)) return true;
    }
  return false;
}

static std::mt19937_64 g(20250917);
static float uni(float a, float b) { return a + (b - a) * float(g() >> 40) / float(1 << 24); }
static vec3 unit_random() {
  for (;;) {
    const vec3 v = v3(uni(-1, 1), uni(-1, 1), uni(-1, 1));
    const float l2 = dot(v, v);
    if (l2 > 1e-3f && l2 <= 1.0f) return v * (1.0f / std::sqrt(l2));
  }
}
// mode 0: any apex and axis; 1: axis-parallel axis and basis; 2: apex at the origin
static Pyr make_pyramid(int mode, float half_lo, float half_hi) {
  Pyr q;
  q.o = mode == 2 ? v3(0, 0, 0) : v3(uni(-8, 8), uni(-8, 8), uni(-8, 8));
  if (mode == 1) {
    const int a = int(g() % 3);
    const float s = (g() & 1) ? 1.0f : -1.0f;
    q.f = v3(a == 0 ? s : 0.0f, a == 1 ? s : 0.0f, a == 2 ? s : 0.0f);
    q.r = v3(a == 1 ? 1.0f : 0.0f, a == 2 ? 1.0f : 0.0f, a == 0 ? 1.0f : 0.0f);
  } else {
    q.f = unit_random();
    vec3 t = unit_random();
    t = t - q.f * dot(t, q.f);
    if (dot(t, t) < 1e-4f) t = cross(q.f, v3(0.3f, -0.5f, 0.8f));
    q.r = t * (1.0f / std::sqrt(dot(t, t)));
  }
  q.u = cross(q.r, q.f);
  q.hw = uni(half_lo, half_hi);
  q.hh = uni(half_lo, half_hi);
  // an off-axis quad of the image plane, as a pixel quad is: centre offsets up to +-0.6
  const float cx = uni(-0.6f, 0.6f), cy = uni(-0.6f, 0.6f);
  auto dir = [&](float a, float b) { return q.f + (cx + a) * q.r + (cy + b) * q.u; };
  q.c[0] = dir(-q.hw, -q.hh);
  q.c[1] = dir(q.hw, -q.hh);
  q.c[2] = dir(q.hw, q.hh);
  q.c[3] = dir(-q.hw, q.hh);
  q.p = cull_pyramid(q.o, q.c[0], q.c[1], q.c[2], q.c[3]);
  return q;
}
// a point at distance dist whose direction lies `off` half-widths from the quad's centre, at a random bearing
static vec3 point_near(const Pyr& q, float dist, float off) {
  const float phi = uni(0.0f, 6.2831853f);
  const vec3 ctr = (q.c[0] + q.c[2]) * 0.5f;
  const vec3 d = ctr + (off * q.hw * std::cos(phi)) * q.r + (off * q.hh * std::sin(phi)) * q.u;
  return q.o + d * (dist / std::sqrt(dot(d, d)));
}

int main() {
  long n_sph = 0, out_sph = 0, n_tri = 0, out_tri = 0;
  auto check_sphere = [&](const Pyr& q, vec3 c, float r) {
    ++n_sph;
    if (!cull_sphere_outside(q.p, c, r)) return false;
    ++out_sph;
    CHECK(!any_ray_hits(q, [&](D3 o, D3 d) { return ray_sphere(o, d, d3(c), double(r)); }));
    return true;
  };
  auto check_triangle = [&](const Pyr& q, vec3 a, vec3 b, vec3 c) {
    ++n_tri;
    if (!cull_triangle_outside(q.p, a, b, c)) return false;
    ++out_tri;
    CHECK(!any_ray_hits(q, [&](D3 o, D3 d) { return ray_triangle(o, d, d3(a), d3(b), d3(c)); }));
    return true;
  };
  for (int it = 0; it < 60000; ++it) {
    const int mode = it % 3;
    const bool pixel = (it / 3) % 2 == 0;  // pixel-sized quads (~1e-3 rad) and wide ones
    const Pyr q = pixel ? make_pyramid(mode, 2e-4f, 4e-3f) : make_pyramid(mode, 0.02f, 0.4f);
    const float dist = uni(0.5f, 40.0f);
    // spheres: anywhere near; near-tangent (the silhouette within a few percent of a half-width of the
    // quad's edge or corner); zero radius; centre behind the apex with a radius that reaches forward
    {
      const float r = uni(0.01f, 3.0f);
      check_sphere(q, point_near(q, dist, uni(0.0f, 6.0f)), r);
      const float off = uni(0.9f, 1.6f);
      const vec3 c = point_near(q, dist, off);
      const vec3 ctr = (q.c[0] + q.c[2]) * 0.5f;
      // radii up to the centre's distance from the quad's centre ray: the silhouette sweeps across the quad
      const vec3 lv = cross(c - q.o, ctr);
      const float lat = std::sqrt(dot(lv, lv) / dot(ctr, ctr));
      check_sphere(q, c, lat * uni(0.0f, 1.05f));
      check_sphere(q, point_near(q, dist, uni(0.0f, 3.0f)), 0.0f);
      check_sphere(q, q.o - q.f * uni(0.1f, 5.0f) + unit_random() * uni(0.0f, 2.0f), uni(0.05f, 6.0f));
    }
    // the apex inside a sphere, or on it within rounding: never outside
    {
      const float r = uni(0.1f, 5.0f);
      const vec3 c = q.o + unit_random() * (r * uni(0.0f, 1.0f));
      CHECK(!cull_sphere_outside(q.p, c, r));
      ++n_sph;
    }
    // triangles: anywhere near; a vertex or an edge close to the quad's boundary; partly or wholly behind
    // the apex; degenerate (two equal vertices, collinear vertices, an edge in line with the apex);
    // axis-parallel edges
    {
      const float sz = dist * uni(0.2f, 3.0f) * (pixel ? 0.01f : 0.3f);
      const vec3 a = point_near(q, dist, uni(0.0f, 5.0f));
      check_triangle(q, a, a + unit_random() * sz, a + unit_random() * sz);
      const vec3 t = point_near(q, dist, uni(0.95f, 1.5f));  // near the boundary, the rest pointing away or across
      check_triangle(q, t, point_near(q, dist * uni(0.7f, 1.4f), uni(1.2f, 8.0f)), point_near(q, dist * uni(0.7f, 1.4f), uni(1.2f, 8.0f)));
      check_triangle(q, t, t + v3(sz, 0, 0), t + v3(0, (g() & 1) ? sz : 0.0f, (g() & 2) ? sz : 0.0f));
      vec3 side = unit_random();
      side = side - q.p.axis * dot(side, q.p.axis);
      const vec3 b = q.o - q.p.axis * uni(0.0f, 3.0f) + side * uni(0.0f, 3.0f);  // beside or behind the apex
      const bool o1 = check_triangle(q, a, b, a + unit_random() * sz);
      const bool o2 = check_triangle(q, b, b + unit_random() * sz, b + unit_random() * sz);
      CHECK(!o1 && !o2);  // not strictly in front: never outside
      check_triangle(q, a, a, a + unit_random() * sz);
      const vec3 e = unit_random() * sz;
      check_triangle(q, a, a + e, a + e * uni(-2.0f, 2.0f));
      check_triangle(q, a, q.o + (a - q.o) * uni(1.1f, 3.0f), a + unit_random() * sz);
      check_triangle(q, a, a, a);
    }
  }
  // clearly separated: more than two pixel widths (four half-widths) of clearance, at every bearing
  long sep = 0, sep_out = 0;
  for (int it = 0; it < 4000; ++it) {
    const Pyr q = make_pyramid(it % 3, 4e-4f, 2e-3f);
    const float hmax = std::fmax(q.hw, q.hh);
    const float dist = uni(2.0f, 20.0f);
    const float r = uni(0.0f, 1.5f);
    // the centre's direction off by the sphere's angular radius + the quad's half diagonal + 4 half-widths
    const float ang = std::asin(std::fmin(1.0f, r / dist)) + 1.5f * hmax + 4.0f * hmax + 1e-4f;
    const float phi = uni(0.0f, 6.2831853f);
    const vec3 ctr = (q.c[0] + q.c[2]) * 0.5f;
    const vec3 cd = ctr * (1.0f / std::sqrt(dot(ctr, ctr)));
    const vec3 e1 = cross(cd, q.u), e1n = e1 * (1.0f / std::sqrt(dot(e1, e1))), e2n = cross(cd, e1n);
    const vec3 d = cd * std::cos(ang) + (e1n * std::cos(phi) + e2n * std::sin(phi)) * std::sin(ang);
    ++sep;
    if (check_sphere(q, q.o + d * dist, r)) ++sep_out;
    // a small triangle about a point as far off: its angular size (< 1.2 sz / dist) added to the offset
    const float sz = uni(0.01f, 0.5f);
    const float angt = 1.3f * sz / dist + 1.5f * hmax + 4.0f * hmax + 1e-4f;
    const vec3 dt = cd * std::cos(angt) + (e1n * std::cos(phi) + e2n * std::sin(phi)) * std::sin(angt);
    const vec3 a = q.o + dt * dist;
    ++sep;
    if (check_triangle(q, a + unit_random() * sz, a + unit_random() * sz, a + unit_random() * sz)) ++sep_out;
  }
  std::printf("spheres: %ld cases, %ld outside; triangles: %ld cases, %ld outside; separated: %ld of %ld outside\n", n_sph,
              out_sph, n_tri, out_tri, sep_out, sep);
  CHECK(sep_out == sep);
  CHECK(out_sph * 10 > n_sph);  // the seeded families are not all "may touch"
  CHECK(out_tri * 10 > n_tri);
  if (fails) std::printf("%d checks failed\n", fails);
  return fails ? 1 : 0;
}
