// The chunk plan and the seed rule of sptr_render_rays (csrc/ray_batch.h) on the host.
// Plan: for n in {1, 2, 7, 64, 257} rays, samples in {1, 2, 5, 16} and the capacities 1, n - 1, n, n + 1,
// n * samples (and samples - 1, samples, samples + 1, which sit at the plan's own threshold), every path
// (ray, sample) appears in exactly one chunk; no chunk exceeds the capacity; chunks hold whole rays (every
// sample of each) unless one ray's samples exceed the capacity, and then each chunk is one ray with a
// contiguous sample range, the ranges of a ray in order and the rays in order; chunks come in ray order.
// Seeds: the rule against a restatement of primary_at's out.rng.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ray_batch.h"

static int fails = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      ++fails;                        \
      std::printf("FAIL %s: ", #c);   \
      std::printf(__VA_ARGS__);       \
      std::printf("\n");              \
    }                                 \
  } while (0)

static void check_plan(uint32_t n, uint32_t samples, uint64_t cap) {
  if (cap == 0) return;
  const uint64_t chunks = sptr::ray_chunk_count(n, samples, cap);
  std::vector<uint32_t> seen((size_t)n * samples, 0u);
  const bool split = (uint64_t)samples > cap;
  uint32_t next_ray = 0, next_s = 0;
  for (uint64_t c = 0; c < chunks; ++c) {
    const sptr::RayChunk k = sptr::ray_chunk_at(n, samples, cap, c);
    CHECK(k.nrays >= 1 && k.ns >= 1, "n %u samples %u cap %llu chunk %llu empty", n, samples, (unsigned long long)cap, (unsigned long long)c);
    CHECK((uint64_t)k.nrays * k.ns <= cap, "n %u samples %u cap %llu chunk %llu holds %llu", n, samples, (unsigned long long)cap,
          (unsigned long long)c, (unsigned long long)k.nrays * k.ns);
    CHECK((uint64_t)k.ray0 + k.nrays <= n && (uint64_t)k.s0 + k.ns <= samples, "n %u samples %u cap %llu chunk %llu out of range", n,
          samples, (unsigned long long)cap, (unsigned long long)c);
    if ((uint64_t)k.ray0 + k.nrays > n || (uint64_t)k.s0 + k.ns > samples) return;
    if (split) {  // one ray, the next contiguous sample range of it
      CHECK(k.nrays == 1u && k.ray0 == next_ray && k.s0 == next_s, "split plan n %u samples %u cap %llu chunk %llu: ray %u s0 %u",
            n, samples, (unsigned long long)cap, (unsigned long long)c, k.ray0, k.s0);
      next_s = k.s0 + k.ns;
      if (next_s == samples) {
        next_s = 0;
        ++next_ray;
      }
    } else {  // whole rays, in order
      CHECK(k.s0 == 0u && k.ns == samples && k.ray0 == next_ray, "whole-ray plan n %u samples %u cap %llu chunk %llu: ray0 %u s0 %u ns %u",
            n, samples, (unsigned long long)cap, (unsigned long long)c, k.ray0, k.s0, k.ns);
      next_ray = k.ray0 + k.nrays;
    }
    for (uint32_t s = 0; s < k.ns; ++s)
      for (uint32_t i = 0; i < k.nrays; ++i) ++seen[(size_t)(k.s0 + s) * n + k.ray0 + i];
  }
  CHECK(next_ray == n && next_s == 0u, "n %u samples %u cap %llu: the plan ends at ray %u sample %u", n, samples,
        (unsigned long long)cap, next_ray, next_s);
  for (size_t p = 0; p < seen.size(); ++p)
    if (seen[p] != 1u) {
      CHECK(false, "n %u samples %u cap %llu: path %zu appears %u times", n, samples, (unsigned long long)cap, p, seen[p]);
      break;
    }
}

// primary_at's out.rng (kernels_wavefront.hip) for pixel seed ps and accumulation index acc
static uint32_t primary_rng(uint32_t ps, uint32_t acc) { return sptr::wang_hash((ps ^ acc) ^ 1u); }

int main() {
  for (uint32_t n : {1u, 2u, 7u, 64u, 257u})
    for (uint32_t samples : {1u, 2u, 5u, 16u})
      for (uint64_t cap : {(uint64_t)1, (uint64_t)n - 1, (uint64_t)n, (uint64_t)n + 1, (uint64_t)n * samples, (uint64_t)samples - 1,
                           (uint64_t)samples, (uint64_t)samples + 1, (uint64_t)n * samples + 3})
        check_plan(n, samples, cap);
  CHECK(sptr::ray_chunk_count(0u, 3u, 8u) == 0u, "an empty batch has no chunk");
  // the largest batch against a small capacity: the count does not overflow
  CHECK(sptr::ray_chunk_count(1u << 28, 2u, 1u) == (1ull << 29), "2^28 rays x 2 samples, capacity 1");
  const sptr::RayChunk last = sptr::ray_chunk_at(1u << 28, 2u, 1u, (1ull << 29) - 1);
  CHECK(last.ray0 == (1u << 28) - 1u && last.nrays == 1u && last.s0 == 1u && last.ns == 1u, "its last chunk");

  // seeds given, one sample: the seed itself
  CHECK(sptr::ray_rng(true, 1u, 0xDEADBEEFu, 5u, 9u, 0u) == 0xDEADBEEFu, "seed passed through");
  for (uint32_t i : {0u, 1u, 149u, 12299u, 0xFFFFFFFFu})
    for (uint32_t fi : {1u, 2u, 77u, 0xFFFFFFF0u})
      for (uint32_t s : {0u, 1u, 4u}) {
        CHECK(sptr::ray_rng(false, 1u, 123u, i, fi, s) == primary_rng(i, fi + s), "no seeds: pixel %u of frame %u + %u", i, fi, s);
        CHECK(sptr::ray_rng(false, 5u, 123u, i, fi, s) == primary_rng(i, fi + s), "no seeds, 5 samples");
        CHECK(sptr::ray_rng(true, 5u, i, 3u, fi, s) == primary_rng(i, fi + s), "seeds, 5 samples: b = seeds[i]");
      }
  std::printf(fails ? "%d checks failed\n" : "ray_batch: ok\n", fails);
  return fails ? 1 : 0;
}
