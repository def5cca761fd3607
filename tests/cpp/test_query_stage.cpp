// The layout of the staging buffer of host-pointer queries (csrc/query_stage.h), for the field tables of the four
// query kinds as csrc/sptr_api.cpp states them:
//   rays       geom 4, prim 4, t 4, ng 12, uv 8 bytes per ray; occluded 1 byte per ray (the any-hit table)
//   multi-hit  count 4 n, then geom 4, prim 4, t 4, ng 12, uv 8 per hit slot (n K slots)
//   points     geom 4, prim 4, dist2 4, dist 4, point 12, uv 8, ng 12
//   signed     the points table and signed_dist 4, normal 12, feature 4
// and n in {1, 3, 63, 64, 257, 2^28}, K in {1, 2, 7, SPTR_MULTI_HIT_MAX} with n K <= 2^28.  Per table and count:
// every offset is a multiple of 16; the fields lie in the given order and do not overlap; the total is at least
// the sum of the sizes and at most that plus 16 per field; nothing wraps 64 bits (the sums are redone in 128
// bits; the largest case is the signed table, 68 bytes x 2^28).  The exit status is the number of failures.
#include <cstdint>
#include <cstdio>

#include "query_stage.h"
#include "sptr_hip.h"

static int fails = 0, cases = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      if (fails < 20) std::printf("FAIL line %d: %s\n", __LINE__, #c); \
      ++fails;                                                         \
    }                                                                  \
  } while (0)

static_assert(sizeof(size_t) == 8, "the bounds below are about 64-bit sizes");

// per[i] bytes for each of rows[i] rows
static void check_table(const char* what, const unsigned* per, const uint64_t* rows, int k) {
  size_t bytes[16], offset[16];
  unsigned __int128 sum = 0;
  for (int i = 0; i < k; ++i) {
    bytes[i] = (size_t)(per[i] * rows[i]);
    sum += (unsigned __int128)per[i] * rows[i];
    offset[i] = ~(size_t)0;
  }
  const size_t total = sptr::stage_layout(bytes, k, offset);
  ++cases;
  unsigned __int128 end = 0;  // of the fields so far
  for (int i = 0; i < k; ++i) {
    CHECK(offset[i] % 16 == 0);
    CHECK((unsigned __int128)offset[i] >= end);  // the given order, no overlap
    end = (unsigned __int128)offset[i] + bytes[i];
  }
  CHECK((unsigned __int128)total >= end);
  CHECK((unsigned __int128)total >= sum);
  CHECK((unsigned __int128)total <= sum + 16u * (unsigned)k);
  if (fails) std::printf("  in %s, %d fields, %llu rows\n", what, k, (unsigned long long)rows[k - 1]);
}

int main() {
  const uint64_t counts[] = {1, 3, 63, 64, 257, 1ull << 28};
  const unsigned hits[] = {1, 2, 7, SPTR_MULTI_HIT_MAX};
  const unsigned rays[] = {4, 4, 4, 12, 8}, occluded[] = {1}, multi[] = {4, 4, 4, 4, 12, 8};
  const unsigned points[] = {4, 4, 4, 4, 12, 8, 12}, sign[] = {4, 4, 4, 4, 12, 8, 12, 4, 12, 4};
  for (const uint64_t n : counts) {
    const uint64_t all[10] = {n, n, n, n, n, n, n, n, n, n};
    check_table("rays", rays, all, 5);
    check_table("rays, any-hit", occluded, all, 1);
    check_table("points", points, all, 7);
    check_table("signed", sign, all, 10);
    for (int k = 1; k <= 10; ++k) check_table("signed, the first fields", sign, all, k);  // (a shorter table)
    for (const unsigned K : hits) {
      if (n * K > (1ull << 28)) continue;
      const uint64_t m = n * K, slots[6] = {n, m, m, m, m, m};
      check_table("multi-hit", multi, slots, 6);
    }
  }
  // fields the caller does not take have 0 bytes: they take no room and disturb nobody's alignment
  {
    size_t bytes[4] = {0, 13, 0, 5}, offset[4];
    const size_t total = sptr::stage_layout(bytes, 4, offset);
    CHECK(offset[0] == 0 && offset[1] == 0 && offset[2] == 16 && offset[3] == 16 && total == 32);
  }
  std::printf("query_stage: %d tables, %d failures\n", cases, fails);
  return fails;
}
