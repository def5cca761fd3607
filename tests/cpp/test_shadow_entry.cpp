// Unit test of the shadow entry table's cell tests (simple-path-tracer_amd/csrc/shadow_entry.h), compiled with
// g++ by tests/test_shadow_entry_cpu.py.
//
// Soundness: an origin is placed, its cell taken with shadow_cell (the query's own arithmetic), and primitives
// are placed on and about its ray along the light direction.  Whatever a float64 ray from the origin along the
// light hits must not be reported outside the cell's prism: zero misses.  Light directions: axis-aligned,
// oblique, nearly horizontal.  Primitives: spheres (zero radius and near-tangent included), triangles (slivers,
// edge-on to the light, straddling cell borders), boxes.  Origins: anywhere, on cell borders, at the extent's edge.
// Not vacuous: primitives whose projection is clearly separated from the cell (more than two cells of
// clearance) must be reported outside, and the seeded families must report a fair share outside.
// A NaN in a primitive never answers "outside".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "shadow_entry.h"

using namespace sptr;

static int fails = 0;
#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      if (fails++ < 10) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                                           \
  } while (0)

struct D3 {
  double x, y, z;
};
static D3 d3(vec3 v) { return D3{v.x, v.y, v.z}; }
static D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static D3 dcross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// exact tests of the half-line o + t d, t > 0
static bool ray_sphere(D3 o, D3 d, D3 c, double r) {
  const D3 oc = o - c;
  const double a = ddot(d, d), b = ddot(oc, d), cc = ddot(oc, oc) - r * r;
  const double disc = b * b - a * cc;
  if (disc < 0.0) return false;
  return (-b + std::sqrt(disc)) / a > 0.0;
}
static bool ray_triangle(D3 o, D3 d, D3 v0, D3 v1, D3 v2) {
  const D3 e1 = v1 - v0, e2 = v2 - v0, pv = dcross(d, e2);
  const double det = ddot(e1, pv);
  if (det == 0.0) return false;
  const D3 tv = o - v0, qv = dcross(tv, e1);
  const double u = ddot(tv, pv) / det, v = ddot(d, qv) / det, t = ddot(e2, qv) / det;
  return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t > 0.0;
}
static bool ray_box(D3 o, D3 d, D3 lo, D3 hi) {
  double t0 = 0.0, t1 = std::numeric_limits<double>::infinity();
  const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
  for (int k = 0; k < 3; ++k) {
    if (dd[k] == 0.0) {
      if (oo[k] < l[k] || oo[k] > h[k]) return false;
      continue;
    }
    double a = (l[k] - oo[k]) / dd[k], b = (h[k] - oo[k]) / dd[k];
    if (a > b) std::swap(a, b);
    t0 = std::fmax(t0, a);
    t1 = std::fmin(t1, b);
  }
  return t0 <= t1;
}

static std::mt19937_64 g(20261021);
static float uni(float a, float b) { return a + (b - a) * float(g() >> 40) / float(1 << 24); }
static vec3 unit_random() {
  for (;;) {
    const vec3 v = v3(uni(-1, 1), uni(-1, 1), uni(-1, 1));
    const float l2 = dot(v, v);
    if (l2 > 1e-3f && l2 <= 1.0f) return v * (1.0f / std::sqrt(l2));
  }
}
static vec3 unit(vec3 v) { return v * (1.0f / std::sqrt(dot(v, v))); }

// family 0: axis-aligned; 1: oblique; 2: nearly horizontal (y within 1e-3 .. 3e-2 of the ground plane)
static vec3 light_dir(int family, int it) {
  if (family == 0) {
    const int a = it % 3;
    const float s = (it / 3) % 2 ? 1.0f : -1.0f;
    return v3(a == 0 ? s : 0.0f, a == 1 ? s : 0.0f, a == 2 ? s : 0.0f);
  }
  if (family == 1) return it == 0 ? unit(v3(0.5f, 1.0f, -0.3f)) : unit_random();
  const float phi = uni(0.0f, 6.2831853f);
  return unit(v3(std::cos(phi), uni(1e-3f, 3e-2f) * ((it & 1) ? 1.0f : -1.0f), std::sin(phi)));
}

int main() {
  long n_sph = 0, out_sph = 0, n_tri = 0, out_tri = 0, n_box = 0, out_box = 0, hits = 0, skipped = 0;
  long sep = 0, sep_out = 0;
  const uint32_t Rs[3] = {32u, 128u, 256u};
  for (int family = 0; family < 3; ++family)
    for (int it = 0; it < 24; ++it) {
      const vec3 w = light_dir(family, it);
      // scene bounds: about the origin, or well away from it (rounding relative to the coordinates)
      const vec3 ctr = (it % 4 == 3) ? v3(uni(-60, 60), uni(-60, 60), uni(-60, 60)) : v3(uni(-2, 2), uni(-2, 2), uni(-2, 2));
      const vec3 half = v3(uni(3, 12), uni(1, 12), uni(3, 12));
      const vec3 lo = ctr - half, hi = ctr + half;
      ShadowFrame fr;
      CHECK(shadow_frame(w, lo, hi, Rs[it % 3], fr));
      CHECK(std::fabs(dot(fr.eu, w)) < 1e-6f && std::fabs(dot(fr.ev, w)) < 1e-6f && std::fabs(dot(fr.eu, fr.ev)) < 1e-6f);
      const D3 dw = d3(w);
      for (int s = 0; s < 400; ++s) {
        // the origin: anywhere in the bounds; or on a cell border / at the extent's edge (u, v a whole number of cells)
        vec3 o = v3(uni(lo.x, hi.x), uni(lo.y, hi.y), uni(lo.z, hi.z));
        if (s % 4 == 1 || s % 4 == 2) {
          const uint32_t bi = (s % 8 == 1) ? 0u : (s % 8 == 2) ? fr.R : uint32_t(g() % (fr.R + 1u));
          const float u = fr.u0 + float(bi) * fr.cell, v = (s % 4 == 2) ? fr.v0 + float(g() % (fr.R + 1u)) * fr.cell : dot(o, fr.ev);
          o = fr.eu * u + fr.ev * v + w * dot(o, w);
        }
        uint32_t ci, cj;
        if (!shadow_cell(fr, o, ci, cj)) {
          ++skipped;  // outside the table: the renderer walks from the root
          continue;
        }
        CHECK(ci < fr.R && cj < fr.R);
        const ShadowPrism pr = shadow_prism(fr, ci, cj);
        const D3 od = d3(o);
        const float cell = fr.cell;
        auto on_ray = [&](float lateral) {  // a point ahead on the ray (or behind it), `lateral` off it
          vec3 side = unit_random();
          side = side - w * dot(side, w);
          side = dot(side, side) > 1e-6f ? unit(side) : fr.eu;
          return o + w * uni(-2.0f, 20.0f) + side * lateral;
        };
        auto check_sphere = [&](vec3 c, float r) {
          ++n_sph;
          const bool out = shadow_sphere_outside(pr, c, r);
          out_sph += out;
          if (ray_sphere(od, dw, d3(c), double(r))) {
            ++hits;
            CHECK(!out);
          }
          return out;
        };
        auto check_triangle = [&](vec3 a, vec3 b, vec3 c) {
          ++n_tri;
          const bool out = shadow_triangle_outside(pr, a, b, c);
          out_tri += out;
          if (ray_triangle(od, dw, d3(a), d3(b), d3(c))) {
            ++hits;
            CHECK(!out);
          }
          return out;
        };
        auto check_box = [&](vec3 a, vec3 b) {
          const vec3 bl = v3(std::fmin(a.x, b.x), std::fmin(a.y, b.y), std::fmin(a.z, b.z));
          const vec3 bh = v3(std::fmax(a.x, b.x), std::fmax(a.y, b.y), std::fmax(a.z, b.z));
          ++n_box;
          const bool out = shadow_box_outside(pr, bl, bh);
          out_box += out;
          if (ray_box(od, dw, d3(bl), d3(bh))) {
            ++hits;
            CHECK(!out);
          }
          return out;
        };
        // spheres: about the ray at up to a few radii; near-tangent; zero radius on and beside the ray
        const float r = uni(0.01f, 2.0f);
        check_sphere(on_ray(r * uni(0.0f, 3.0f)), r);
        check_sphere(on_ray(r * uni(0.98f, 1.02f)), r);
        check_sphere(on_ray(0.0f), 0.0f);
        check_sphere(on_ray(cell * uni(0.0f, 3.0f)), 0.0f);
        check_sphere(on_ray(cell * uni(0.0f, 2.0f)), cell * uni(0.0f, 1.0f));
        // triangles: about a point on the ray; a vertex or an edge on the ray; slivers; edge-on to the light
        // (w in the triangle's plane, exactly and nearly); cell-sized ones straddling the cell's borders
        const float sz = (s & 1) ? cell * uni(0.2f, 4.0f) : uni(0.1f, 4.0f);
        const vec3 p = on_ray(0.0f);
        check_triangle(p + unit_random() * sz, p + unit_random() * sz, p + unit_random() * sz);
        check_triangle(p, p + unit_random() * sz, p + unit_random() * sz);
        const vec3 e = unit_random() * sz;
        check_triangle(p - e, p + e, p + unit_random() * sz);
        check_triangle(p - e, p + e, p + e * uni(-1.0f, 1.0f) + unit_random() * (sz * 1e-4f));  // sliver through the ray
        const vec3 q = on_ray(sz * uni(0.0f, 0.5f));
        check_triangle(q, q + e, q + e * uni(0.2f, 0.8f) + unit_random() * (sz * 1e-3f));      // sliver beside it
        check_triangle(p - e, p + e, p + w * uni(-3.0f, 3.0f));                               // edge-on: contains a line along w
        check_triangle(q - e, q + e, q + w * uni(-3.0f, 3.0f) + unit_random() * (sz * 1e-5f));  // nearly edge-on
        check_triangle(p, p, p + e);
        check_triangle(p, p, p);
        // boxes about and beside the ray
        check_box(p - v3(uni(0, sz), uni(0, sz), uni(0, sz)), p + v3(uni(0, sz), uni(0, sz), uni(0, sz)));
        check_box(q, q + unit_random() * sz);
        // clearly separated: the primitive's projection keeps more than two cells of clearance from the cell
        {
          const float phi = uni(0.0f, 6.2831853f), rs = uni(0.0f, 1.5f), ext = uni(0.01f, 1.0f);
          const float cu = 0.5f * (pr.a0 + pr.a1), cv = 0.5f * (pr.b0 + pr.b1);
          const float clear = 0.75f * cell + 2.0f * cell;  // half the cell's diagonal + two cells
          const vec3 dirp = fr.eu * std::cos(phi) + fr.ev * std::sin(phi);
          const vec3 base = fr.eu * cu + fr.ev * cv + w * dot(o, w);
          const vec3 cs = base + dirp * (clear + rs * 1.01f + 1e-3f * fr.diag + 1e-3f) + w * uni(-5.0f, 5.0f);
          ++sep;
          sep_out += check_sphere(cs, rs);
          const vec3 ct = base + dirp * (clear + 1.01f * ext + 1e-3f) + w * uni(-5.0f, 5.0f);
          ++sep;
          sep_out += check_triangle(ct + unit_random() * ext, ct + unit_random() * ext, ct + unit_random() * ext);
          // (a box is tested by its extent along eu and along ev only: separated along one of the two)
          const vec3 axis = ((s & 2) ? fr.eu : fr.ev) * ((s & 4) ? 1.0f : -1.0f);
          const vec3 cb = base + axis * (clear + 1.01f * ext + 1e-3f) + ((s & 2) ? fr.ev : fr.eu) * (cell * uni(-3.0f, 3.0f)) +
                          w * uni(-5.0f, 5.0f);
          ++sep;
          sep_out += check_box(cb - v3(ext, ext, ext) * 0.57f, cb + v3(ext, ext, ext) * 0.57f);
        }
        // a NaN never answers "outside"
        if (s % 50 == 0) {
          const float nan = std::numeric_limits<float>::quiet_NaN();
          CHECK(!shadow_sphere_outside(pr, v3(nan, 0, 0), 1.0f));
          CHECK(!shadow_sphere_outside(pr, v3(100, 100, 100), nan));
          CHECK(!shadow_triangle_outside(pr, v3(nan, nan, nan), v3(100, 0, 0), v3(0, 100, 0)));
          CHECK(!shadow_triangle_outside(pr, v3(nan, nan, nan), v3(nan, nan, nan), v3(nan, nan, nan)));
          CHECK(!shadow_box_outside(pr, v3(nan, nan, nan), v3(nan, nan, nan)));
        }
      }
    }
  std::printf("spheres: %ld cases, %ld outside; triangles: %ld, %ld; boxes: %ld, %ld; float64 hits checked: %ld; "
              "origins outside the table: %ld; separated: %ld of %ld outside\n",
              n_sph, out_sph, n_tri, out_tri, n_box, out_box, hits, skipped, sep_out, sep);
  CHECK(sep_out == sep);
  CHECK(hits * 4 > n_sph);  // the placements do hit
  CHECK(out_sph * 10 > n_sph);
  CHECK(out_tri * 10 > n_tri);
  CHECK(out_box * 10 > n_box);
  if (fails) std::printf("%d checks failed\n", fails);
  return fails ? 1 : 0;
}
