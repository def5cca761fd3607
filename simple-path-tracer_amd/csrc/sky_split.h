// sky_split.h — partition of a lane-group bounce 0 (k_trace_wp) with a cull mask, for host and device.
//
// k_cull leaves two lists in one buffer of P + 2 words: the unculled valid pixels from plist[0] up (count at
// plist[P]) and the culled valid pixels from plist[P - 1] down (culled rank j at plist[P - 1 - j], count at
// plist[P + 1]).  Together they hold at most P pixels, so the two cannot meet.
//
// A culled pixel's samples all miss: its sum needs no lane group, no LDS and no barrier.  With T bulk threads,
//   m      = n_culled / T            culled pixels per bulk thread, exactly
//   bulk   = culled ranks [0, m T)   thread t sums ranks t, t + T, ..., t + (m - 1) T   (k_sky, list mode)
//   items  = the unculled pixels, then the culled ranks [m T, n_culled)                 (k_trace_wp, list mode)
// The items are walked in chunks of kSkySplitChunk consecutive items dealt round-robin over the blocks: a chunk
// is a run of one tile's pixels (two at a seam), since k_cull lists each tile's pixels as one run.
// n_culled < T gives m = 0: no bulk, and every valid pixel is an item.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SPTR_SS __host__ __device__ __forceinline__
#else
#define SPTR_SS inline
#endif

namespace sptr {

constexpr uint32_t kSkySplitChunk = 32;  // items per block round (k_trace_wp: kBlock / kFoldLanes pixels)

struct SkySplit {
  uint32_t n_unculled, n_culled;
  uint32_t threads;  // T
  uint32_t m;        // culled pixels per bulk thread
  uint32_t bulk;     // m T: the culled ranks below it are the bulk threads'
  uint32_t items;    // n_unculled + (n_culled - bulk)
};

SPTR_SS SkySplit sky_split(uint32_t n_unculled, uint32_t n_culled, uint32_t threads) {
  SkySplit s;
  s.n_unculled = n_unculled;
  s.n_culled = n_culled;
  s.threads = threads;
  s.m = threads ? n_culled / threads : 0u;
  s.bulk = s.m * threads;
  s.items = n_unculled + (n_culled - s.bulk);
  return s;
}

// word of the list buffer (P pixels) that holds culled rank j
SPTR_SS uint32_t sky_split_culled_word(uint32_t P, uint32_t rank) { return P - 1u - rank; }
// j-th pixel (j < m) of bulk thread t (t < T): its culled rank
SPTR_SS uint32_t sky_split_bulk_rank(const SkySplit& s, uint32_t t, uint32_t j) { return t + j * s.threads; }
// item i (i < items) -> word of the list buffer that holds its pixel
SPTR_SS uint32_t sky_split_item_word(const SkySplit& s, uint32_t P, uint32_t i) {
  return i < s.n_unculled ? i : sky_split_culled_word(P, s.bulk + (i - s.n_unculled));
}
// whether item i is a culled pixel (it takes no walk)
SPTR_SS bool sky_split_item_culled(const SkySplit& s, uint32_t i) { return i >= s.n_unculled; }

// Items of (logical) block b of a grid of `blocks`: chunks b, b + blocks, ... of kSkySplitChunk items.
SPTR_SS uint32_t sky_split_block_items(uint32_t items, uint32_t blocks, uint32_t b) {
  const uint32_t step = blocks * kSkySplitChunk;
  uint32_t n = 0u;
  for (uint32_t base = b * kSkySplitChunk; base < items; base += step)
    n += items - base < kSkySplitChunk ? items - base : kSkySplitChunk;
  return n;
}
// Pixels per block at most, over P pixels or over any item list of at most P items: the stride (times the
// batch's samples) of a block's hit-record segment, which the host sizes from P alone.
SPTR_SS uint32_t sky_split_block_cap(uint32_t P, uint32_t blocks) {
  const uint32_t step = blocks * kSkySplitChunk;
  return (P + step - 1u) / step * kSkySplitChunk;
}

}  // namespace sptr
