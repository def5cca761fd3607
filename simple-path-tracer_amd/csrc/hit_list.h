// hit_list.h — the per-ray list of sptr_query_multi_hit, for host and device: the K nearest candidate hits of a
// ray in ascending order of the key (t, geomID, primID).  k_rayquery_multi (kernels_query.h) calls these functions
// from its leaf routine, and tests/cpp/test_hit_list.cpp compiles the same text.
//
// An entry is (t, ref).  ref is the primitive reference the walks carry ([kSphereBit] | slot, slot < 2^30) with
// bit 31 (kHitSecond) set for a sphere's second hit.  Bit 31 is kLeafBit in a *link*; a primitive reference never
// carries it, so the flag costs no index bit and the primitive limit stays what the leaf links allow (2^26).
//
// Store: where the entries live, passed as an accessor so that the list's code does not know (LDS columns on
// the device, an array with guard values in the stand-alone program):
//   float t(uint32_t i) const; uint32_t ref(uint32_t i) const; void set(uint32_t i, float t, uint32_t ref);
// Key: ref -> (uint64_t(geomID) << 32) | primID, exactly as the query reports the ids.  It is called only when
// two entries tie exactly in t (float comparison: +0.0 == -0.0), so the id loads cost nothing otherwise.
#pragma once
#include <stdint.h>

#include "sptr_math.h"

namespace sptr {

constexpr uint32_t kHitSecond = 0x80000000u;

// Inserts candidate (t, ref) into the sorted list of n <= k entries, k <= the store's capacity, keeping the k
// smallest keys.  A candidate whose key equals an entry's is dropped: it is the same primitive reached through
// another reference.  The result does not depend on the order of the insertions: it is the first k of the set
// of distinct keys.  Touches entries 0 .. min(n, k - 1) only.
template <class Store, class Key>
SPTR_HD void hit_list_insert(Store& s, uint32_t& n, uint32_t k, float t, uint32_t ref, Key&& key) {
  uint32_t pos = n;
  uint64_t kc = 0;
  bool have = false;
  while (pos > 0u) {
    const float te = s.t(pos - 1u);
    if (te == t) {
      const uint32_t re = s.ref(pos - 1u);
      if (re == ref) return;
      if (!have) {
        kc = key(ref);
        have = true;
      }
      const uint64_t ke = key(re);
      if (ke == kc) return;
      if (ke < kc) break;
    } else if (!(te > t)) {
      break;
    }
    --pos;
  }
  if (pos >= k) return;
  for (uint32_t i = n < k ? n : k - 1u; i > pos; --i) s.set(i, s.t(i - 1u), s.ref(i - 1u));
  s.set(pos, t, ref);
  if (n < k) ++n;
}

// The distance beyond which a box cannot hold a candidate that enters the list: the ray's tfar while the list
// is not full, the k-th t once it is (a candidate at exactly that t may still enter, by its ids: the box tests
// are inclusive).
template <class Store>
SPTR_HD float hit_list_bound(const Store& s, uint32_t n, uint32_t k, float tfar) {
  if (n < k) return tfar;
  const float tk = s.t(k - 1u);
  return tk < tfar ? tk : tfar;
}

// A sphere's candidates: what the closest-hit test `hit(tnear, tfar, t)` reports on (tnear, tfar), and, if it
// reports t_a, what the same test reports on (t_a, tfar).  emit(t, flag): flag 0 for the first, kHitSecond for
// the second.
template <class Hit, class Emit>
SPTR_HD void hit_list_sphere(Hit&& hit, float tnear, float tfar, Emit&& emit) {
  float ta = 0.0f, tb = 0.0f;
  if (!hit(tnear, tfar, ta)) return;
  emit(ta, 0u);
  if (hit(ta, tfar, tb)) emit(tb, kHitSecond);
}

}  // namespace sptr
