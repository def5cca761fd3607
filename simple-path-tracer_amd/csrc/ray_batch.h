// ray_batch.h — chunk plan and seed rule of sptr_render_rays, for host and device.
//
// A batch of n rays with `samples` paths per ray runs in chunks that fit the wave capacity `cap` (paths).
// A chunk holds whole rays, every sample of each: rays [ray0, ray0 + nrays), samples [0, samples).  Only when
// one ray's samples alone exceed the capacity is the sample range split as well: every chunk then holds one
// ray and a contiguous sample range [s0, s0 + ns) of it, the ranges of a ray in order, so that k_rays_gather
// can carry the ray's running sum from one chunk to the next and every add keeps its place.
// Path j of a chunk is sample s0 + j / nrays of ray ray0 + j % nrays: path id = stream slot = j.
#pragma once
#include <stdint.h>

#include "sptr_math.h"

namespace sptr {

struct RayChunk {
  uint32_t ray0, nrays;  // rays [ray0, ray0 + nrays)
  uint32_t s0, ns;       // samples [s0, s0 + ns) of each
};

// whether the plan splits sample ranges (one ray per chunk)
SPTR_HD bool ray_plan_splits(uint32_t samples, uint64_t cap) { return (uint64_t)samples > cap; }
// rays per chunk of a plan that keeps rays whole (cap >= samples >= 1)
SPTR_HD uint32_t ray_plan_rays(uint32_t n, uint32_t samples, uint64_t cap) {
  const uint64_t r = cap / samples;
  return r < (uint64_t)n ? (uint32_t)r : n;
}
// sample ranges per ray of a splitting plan
SPTR_HD uint32_t ray_plan_ranges(uint32_t samples, uint64_t cap) { return (uint32_t)(((uint64_t)samples + cap - 1u) / cap); }

// chunks of the plan: n, samples, cap >= 1 (n == 0: none)
SPTR_HD uint64_t ray_chunk_count(uint32_t n, uint32_t samples, uint64_t cap) {
  if (n == 0u) return 0u;
  if (ray_plan_splits(samples, cap)) return (uint64_t)n * ray_plan_ranges(samples, cap);
  const uint32_t r = ray_plan_rays(n, samples, cap);
  return ((uint64_t)n + r - 1u) / r;
}
// chunk c < ray_chunk_count(n, samples, cap)
SPTR_HD RayChunk ray_chunk_at(uint32_t n, uint32_t samples, uint64_t cap, uint64_t c) {
  RayChunk k;
  if (ray_plan_splits(samples, cap)) {
    const uint32_t ranges = ray_plan_ranges(samples, cap);
    const uint32_t q = (uint32_t)(c % ranges);
    k.ray0 = (uint32_t)(c / ranges);
    k.nrays = 1u;
    k.s0 = (uint32_t)(q * cap);  // (q * cap < samples)
    k.ns = samples - k.s0 < cap ? samples - k.s0 : (uint32_t)cap;
    return k;
  }
  const uint32_t r = ray_plan_rays(n, samples, cap);
  k.ray0 = (uint32_t)(c * r);
  k.nrays = n - k.ray0 < r ? n - k.ray0 : r;
  k.s0 = 0u;
  k.ns = samples;
  return k;
}

// Rng state of sample s of ray i.  seed: seeds[i] (has_seeds) or anything.  With seeds and one sample per ray
// the state is the seed itself; otherwise it is primary_at's out.rng for pixel seed b = seeds[i] or i and
// accumulation index frame_index + s, so ray i of a batch without seeds draws what pixel i of that frame draws.
SPTR_HD uint32_t ray_rng(bool has_seeds, uint32_t samples, uint32_t seed, uint32_t i, uint32_t frame_index, uint32_t s) {
  if (has_seeds && samples == 1u) return seed;
  const uint32_t b = has_seeds ? seed : i;
  return wang_hash((b ^ (frame_index + s)) ^ 1u);
}

}  // namespace sptr
