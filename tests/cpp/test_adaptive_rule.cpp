// The rule of sptr_render_adaptive (csrc/adaptive_rule.h) on the host: the text the kernels call.
// RULE lines: for a table of inputs — special values and pseudo-random sums — the inputs as hex words and what
// the header computes from them: "RULE Sr Sg Sb Er Eg Eb n thr min max step -> err active take key".
// tests/test_adaptive_cpu.py compares every line with tests/adaptive_ref.py.
// PLAN lines: the chunk plan over a list (ray_batch.h's plan with "ray" = list entry and samples = the take,
// adaptive_path for a chunk's paths, the consumer advancing n chunk by chunk): for lists of n entries with unequal
// counts, takes of 1 .. 9 and the capacities 1, n - 1, n, n + 1 and n * take, every (entry, sample index) of the
// pass appears exactly once and no chunk exceeds the capacity.  The exit status is the number of failures.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "adaptive_rule.h"

static int fails = 0;
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static uint32_t lcg(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return s;
}
static float unit(uint32_t& s) { return float(lcg(s) >> 8) / float(1u << 24); }

static void rule_line(sptr::vec3 S, sptr::vec3 E, uint32_t n, const sptr::AdaptiveRule& r) {
  const float e = sptr::adaptive_err(S, E, n);
  const bool a = sptr::adaptive_active(r, S, E, n);
  const uint32_t take = n < r.max_samples ? sptr::adaptive_take(r, n) : 0u;
  const uint32_t key = n < r.max_samples ? sptr::adaptive_key(r, n) : 0u;
  std::printf("RULE %08x %08x %08x %08x %08x %08x %u %08x %u %u %u -> %08x %d %u %u\n", bits(S.x), bits(S.y), bits(S.z), bits(E.x),
              bits(E.y), bits(E.z), n, bits(r.threshold), r.min_samples, r.max_samples, r.step, bits(e), a ? 1 : 0, take, key);
}

static void plan(uint32_t n, uint32_t take, uint64_t cap) {
  if (cap == 0) return;
  std::vector<uint32_t> n0(n), cur(n);
  for (uint32_t e = 0; e < n; ++e) n0[e] = cur[e] = (e * 7u) % 5u;  // unequal counts before the pass
  std::vector<uint32_t> seen((size_t)n * take, 0u);
  const uint64_t chunks = sptr::ray_chunk_count(n, take, cap);
  bool ok = true;
  for (uint64_t c = 0; c < chunks && ok; ++c) {
    const sptr::RayChunk ck = sptr::ray_chunk_at(n, take, cap, c);
    const uint64_t np = (uint64_t)ck.nrays * ck.ns;
    if (np > cap || np == 0) ok = false;
    for (uint32_t j = 0; j < np && ok; ++j) {
      uint32_t e, s;
      sptr::adaptive_path(ck, j, e, s);
      if (e < ck.ray0 || e >= ck.ray0 + ck.nrays || e >= n || s >= ck.ns) {
        ok = false;
        break;
      }
      const uint32_t index = cur[e] + 1u + s;  // 1-based sample index, as k_adapt_inject derives it
      if (index <= n0[e] || index > n0[e] + take) ok = false;
      else ++seen[(size_t)e * take + (index - n0[e] - 1u)];
    }
    for (uint32_t i = 0; i < ck.nrays; ++i) cur[ck.ray0 + i] += ck.ns;  // k_adapt_gather
  }
  for (uint32_t v : seen) ok = ok && v == 1u;
  for (uint32_t e = 0; e < n; ++e) ok = ok && cur[e] == n0[e] + take;
  std::printf("PLAN n %u take %u cap %llu chunks %llu %s\n", n, take, (unsigned long long)cap, (unsigned long long)chunks,
              ok ? "ok" : "FAIL");
  if (!ok) ++fails;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const sptr::AdaptiveRule rules[] = {{0.02f, 8u, 32u, 4u}, {0.0f, 4u, 8u, 2u}, {1e30f, 2u, 7u, 3u}, {0.5f, 2u, 65536u, 1000u}};
  for (const sptr::AdaptiveRule& r : rules) {
    const uint32_t ns[] = {0u, 1u, 2u, 3u, r.min_samples - 1u, r.min_samples, r.min_samples + 1u, r.max_samples - 1u, r.max_samples,
                           r.max_samples + 1u};
    for (uint32_t n : ns) {
      rule_line(sptr::v3(0.0f, 0.0f, 0.0f), sptr::v3(0.0f, 0.0f, 0.0f), n, r);           // black: den at its floor
      rule_line(sptr::v3(1.0f, 2.0f, 3.0f), sptr::v3(0.5f, 1.0f, 1.5f), n, r);
      rule_line(sptr::v3(nan, 2.0f, 3.0f), sptr::v3(0.5f, 1.0f, 1.5f), n, r);            // a NaN sample
      rule_line(sptr::v3(inf, 2.0f, 3.0f), sptr::v3(inf, 1.0f, 1.5f), n, r);
      rule_line(sptr::v3(-1.0f, -2.0f, 0.5f), sptr::v3(-0.5f, 0.0f, 0.25f), n, r);       // a negative sum
      rule_line(sptr::v3(1e-6f, 1e-6f, 1e-6f), sptr::v3(4e-7f, 6e-7f, 5e-7f), n, r);
      rule_line(sptr::v3(-0.0f, 0.0f, -0.0f), sptr::v3(0.0f, -0.0f, 0.0f), n, r);
    }
    uint32_t s = 12345u + r.min_samples;
    for (int k = 0; k < 400; ++k) {
      const uint32_t n = 2u + lcg(s) % (r.max_samples < 64u ? r.max_samples : 64u);
      const float scale = k % 3 == 0 ? 0.01f : (k % 3 == 1 ? 1.0f : 50.0f);
      sptr::vec3 S = sptr::v3(unit(s) * scale * float(n), unit(s) * scale * float(n), unit(s) * scale * float(n));
      const float h = float(n / 2u) / float(n), d = k % 2 ? 0.02f : 0.3f;  // E near S / 2
      sptr::vec3 E = sptr::v3(S.x * h * (1.0f + d * (unit(s) - 0.5f)), S.y * h * (1.0f + d * (unit(s) - 0.5f)),
                              S.z * h * (1.0f + d * (unit(s) - 0.5f)));
      rule_line(S, E, n, r);
    }
  }
  for (uint32_t n : {1u, 2u, 7u, 64u, 257u})
    for (uint32_t take : {1u, 2u, 4u, 9u})
      for (uint64_t cap : {(uint64_t)1, (uint64_t)n - 1u, (uint64_t)n, (uint64_t)n + 1u, (uint64_t)n * take, (uint64_t)take - 1u,
                           (uint64_t)take, (uint64_t)take + 1u})
        plan(n, take, cap);
  for (uint32_t i = 1; i <= 9; ++i)
    if (sptr::adaptive_even(i) != (i % 2u == 0u)) ++fails;
  std::printf("%s (%d failures)\n", fails ? "FAILED" : "ok", fails);
  return fails ? 1 : 0;
}
