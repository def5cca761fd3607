// Unit test of the per-vertex transform the host flattening and the refit's transform pass share
// (simple-path-tracer_amd/csrc/xform_point.h), compiled with g++ -ffp-contract=off by tests/test_transform_cpu.py.
//
// On random matrices and points (magnitudes over 2^-8 .. 2^8, both signs):
//   - every component equals (m0 + m1) + (m2 + m3) with each product and each sum rounded to float32, written
//     out here with volatile floats so that no other association or contraction can be substituted;
//   - the left-to-right sum ((m0 + m1) + m2) + m3 and the fused form differ from it on some inputs, so the
//     comparison does tell the orders apart;
//   - it lies within 3 * 2^-24 * (|m0| + |m1| + |m2| + |m3|) of the long-double evaluation (one rounding per
//     product, two per sum path);
//   - row 3 of the matrix is not read (NaN there changes nothing), the identity returns the point's bits, and a
//     translation of zero keeps the sign of nothing but zero.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "xform_point.h"

using sptr::vec3;

static int fails = 0;
#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      if (fails++ < 10) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                                           \
  } while (0)

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  std::mt19937 rng(12345);
  std::uniform_real_distribution<float> mant(1.0f, 2.0f);
  std::uniform_int_distribution<int> ex(-8, 8), sg(0, 1);
  auto rnd = [&]() { return std::ldexp(mant(rng), ex(rng)) * (sg(rng) ? -1.0f : 1.0f); };
  const int N = 200000;
  int differs_ltr = 0, differs_fma = 0;
  for (int it = 0; it < N; ++it) {
    float m[16];
    for (float& v : m) v = rnd();
    m[3] = m[7] = m[11] = m[15] = std::numeric_limits<float>::quiet_NaN();  // row 3: never read
    const vec3 p{rnd(), rnd(), rnd()};
    const vec3 got = sptr::xform_point(m, p);
    const float g[3] = {got.x, got.y, got.z};
    for (int k = 0; k < 3; ++k) {
      volatile float m0 = m[k] * p.x, m1 = m[4 + k] * p.y, m2 = m[8 + k] * p.z, m3 = m[12 + k] * 1.0f;
      volatile float a = m0 + m1, b = m2 + m3;
      volatile float want = a + b;
      CHECK(bits(g[k]) == bits(want));
      volatile float l1 = a + m2;
      volatile float ltr = l1 + m3;
      if (bits(ltr) != bits(want)) ++differs_ltr;
      const float fused = std::fma(m[k], p.x, std::fma(m[4 + k], p.y, std::fma(m[8 + k], p.z, m[12 + k])));
      if (bits(fused) != bits(want)) ++differs_fma;
      const long double exact = (long double)m[k] * p.x + (long double)m[4 + k] * p.y + (long double)m[8 + k] * p.z + (long double)m[12 + k];
      const long double mag = std::fabs((long double)m[k] * p.x) + std::fabs((long double)m[4 + k] * p.y) +
                              std::fabs((long double)m[8 + k] * p.z) + std::fabs((long double)m[12 + k]);
      // (1 + 2^-20: the sums round values that already carry the products' errors)
      CHECK(std::fabs((long double)g[k] - exact) <= 3.0L * std::ldexp(1.0L, -24) * (1.0L + std::ldexp(1.0L, -20)) * mag);
    }
  }
  CHECK(differs_ltr > N / 100);
  CHECK(differs_fma > N / 100);
  float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int it = 0; it < 1000; ++it) {
    const vec3 p{rnd(), rnd(), rnd()};
    const vec3 q = sptr::xform_point(id, p);
    CHECK(bits(q.x) == bits(p.x) && bits(q.y) == bits(p.y) && bits(q.z) == bits(p.z));
  }
  // exact doubling (the tree-cost test scales a scene by diag(2, 2, 2))
  float two[16] = {2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 1};
  for (int it = 0; it < 1000; ++it) {
    const vec3 p{rnd(), rnd(), rnd()};
    const vec3 q = sptr::xform_point(two, p);
    CHECK(q.x == 2.0f * p.x && q.y == 2.0f * p.y && q.z == 2.0f * p.z);
  }
  std::printf("%d points, %d failures; the left-to-right sum differs on %d components, the fused form on %d\n", N, fails,
              differs_ltr, differs_fma);
  return fails ? 1 : 0;
}
