// adaptive_rule.h — the rule of sptr_render_adaptive, for host and device: the half-buffer error of a pixel,
// the active predicate, the samples a pass takes, and where a path of a chunk belongs.  The kernels of
// kernels_adaptive.h call these functions, and tests/cpp/test_adaptive_rule.cpp compiles the same text.
//
// Every float operation is one correctly rounded float32 operation (-ffp-contract=off; HIP's default division and
// square root), as include/sptr_hip.h states the rule.
#pragma once
#include <stdint.h>

#include "ray_batch.h"
#include "sptr_math.h"

namespace sptr {

struct AdaptiveRule {
  float threshold;
  uint32_t min_samples, max_samples, step;
};

SPTR_HD float adaptive_abs(float v) { return __builtin_fabsf(v); }

// err of a pixel with sums S (all samples) and E (even-indexed samples) after n samples.  n < 2: E = 0 and
// hf = 0 give 0 / 0, a NaN, which compares false below.
SPTR_HD float adaptive_err(vec3 S, vec3 E, uint32_t n) {
  const float nf = float(n), hf = float(n / 2u);
  const vec3 I = S / nf, A = E / hf;
  const float num = (adaptive_abs(I.x - A.x) + adaptive_abs(I.y - A.y)) + adaptive_abs(I.z - A.z);
  const float den = sq_root(fmax_g((I.x + I.y) + I.z, 1e-4f));
  return num / den;
}

// active iff n < max && !(n >= min && err < threshold); err is read only when n >= min
SPTR_HD bool adaptive_active(const AdaptiveRule& r, vec3 S, vec3 E, uint32_t n) {
  if (n >= r.max_samples) return false;
  if (n < r.min_samples) return true;
  return !(adaptive_err(S, E, n) < r.threshold);
}

// samples an active pixel takes in a pass (n < max_samples)
SPTR_HD uint32_t adaptive_take(const AdaptiveRule& r, uint32_t n) {
  if (n == 0u) return r.min_samples;
  const uint32_t left = r.max_samples - n;
  return r.step < left ? r.step : left;
}

// A pass runs its active pixels in groups of equal take, one list per group, the groups in ascending key: the
// take of a pixel with n > 0, and kAdaptiveKeyFresh, above every take, for n == 0.  In that order no pixel is
// sampled twice in a pass: a group with take < step ends at max_samples and is inactive afterwards, the group
// with take == step comes last among the pixels with n > 0, and the pixels it leaves active have n > 0 and a take
// <= step, which no later group of the pass (only n == 0 follows) can match.
constexpr uint32_t kAdaptiveKeyFresh = 0x7FFFFFFFu;
SPTR_HD uint32_t adaptive_key(const AdaptiveRule& r, uint32_t n) { return n == 0u ? kAdaptiveKeyFresh : adaptive_take(r, n); }

// Path j of chunk ck (ray_batch.h's plan with "ray" = list entry and samples = the group's take): the entry, and
// the sample's place s after the pixel's current count — its 1-based index is n + 1 + s.  The consumer advances
// n chunk by chunk, so a split sample range continues from the state and the chunk's s0 is not added again.
SPTR_HD void adaptive_path(const RayChunk& ck, uint32_t j, uint32_t& entry, uint32_t& s) {
  s = j / ck.nrays;
  entry = ck.ray0 + (j - s * ck.nrays);
}
// whether sample index i (1-based) also goes to E
SPTR_HD bool adaptive_even(uint32_t i) { return (i & 1u) == 0u; }

}  // namespace sptr
