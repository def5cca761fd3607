// Unit test of the SAH order of LDS-staged scenes (simple-path-tracer_amd/csrc/sah_order.h), compiled with g++ by
// tests/test_sah_order_cpu.py (and once with -fsanitize=address,undefined).
//
// For every case and leaf_max in 1, 2, 4, 8, 16:
//   - the keys are unique and prefix-free (a key's path, of the length the builder gave it, is no prefix of
//     another's: checked through the rebuilt tree, in which every reference ends as a single leaf);
//   - the hierarchy rebuilt from the sorted keys by their highest differing bit (what k_karras does) is the
//     builder's tree, node for node, with the same depth, leaf count and modelled cost;
//   - every reference is in exactly one leaf range; leaf ranges are contiguous in key order, numbered in that
//     order, hold at most leaf_max references, spheres before triangles, each kind by index;
//   - building twice gives the same keys and leaf indices; 63-bit keys are the 64-bit keys' paths;
//   - sah_order_choose never keeps a SAH tree whose modelled cost is not below the Morton tree's, nor one deeper
//     than max(Morton depth, free stack).
// Cases: 1, 2 and 9 references; 12 references with identical centres; a chain of 71 nested segments, 70 deep (falls back: a
// path longer than the key); the 21 boxes of the default scene with its emitter (no fallback, every leaf one
// kind, modelled cost below the Morton tree's); 200 random scenes of 8 .. 430 boxes.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "sah_order.h"

using namespace sptr;

static int fails = 0;
#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      if (fails++ < 10) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                                           \
  } while (0)

struct Scene {
  std::vector<SahBox> box;
  std::vector<uint8_t> is_tri;
};

// k_morton's key of a reference (21 bits per axis of the box centre within the centres' bounds)
static std::vector<uint64_t> morton_keys(const Scene& s) {
  const size_t n = s.box.size();
  float lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    lo[k] = 3.4e38f;
    hi[k] = -3.4e38f;
    for (size_t i = 0; i < n; ++i) {
      const float c = 0.5f * (s.box[i].lo[k] + s.box[i].hi[k]);
      lo[k] = std::min(lo[k], c);
      hi[k] = std::max(hi[k], c);
    }
  }
  std::vector<uint64_t> key(n, 0);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      const float c = 0.5f * (s.box[i].lo[k] + s.box[i].hi[k]), ext = hi[k] - lo[k];
      const float t = ext > 0.0f ? (c - lo[k]) / ext : 0.5f;
      const uint32_t q = (uint32_t)std::min(std::max(t * 2097152.0f, 0.0f), 2097151.0f);
      for (int b = 0; b < 21; ++b) key[i] |= (uint64_t)((q >> b) & 1u) << (3 * b + 2 - k);
    }
  return key;
}

static bool close(double a, double b) { return std::fabs(a - b) <= 1e-9 * std::max(std::fabs(a), std::fabs(b)); }

// the checks of one build; returns false when the keys overflowed (nothing more to check)
static bool check_order(const Scene& s, uint32_t leaf_max, SahCosts k, uint32_t max_bits, bool expect_one_kind) {
  const uint32_t n = (uint32_t)s.box.size();
  const SahOrder o = sah_order_build(s.box.data(), s.is_tri.data(), n, leaf_max, k, max_bits);
  const SahOrder o2 = sah_order_build(s.box.data(), s.is_tri.data(), n, leaf_max, k, max_bits);
  CHECK(o.key == o2.key && o.leaf == o2.leaf && o.order == o2.order && o.overflow == o2.overflow);
  CHECK(o.key.size() == n && o.leaf.size() == n && o.order.size() == n);
  if (o.overflow) {
    CHECK(o.path_depth >= max_bits);
    return false;
  }
  CHECK(o.path_depth <= max_bits);
  // order: a permutation, ascending unique keys
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t j = 0; j < n; ++j) {
    CHECK(o.order[j] < n && !seen[o.order[j]]);
    seen[o.order[j]] = 1;
    if (j) CHECK(o.key[o.order[j - 1]] < o.key[o.order[j]]);
    if (max_bits < 64) CHECK((o.key[o.order[j]] & ((1ull << (64 - max_bits)) - 1ull)) == 0ull);
  }
  // the tree k_karras builds over the sorted keys
  std::vector<uint64_t> sk(n);
  std::vector<SahBox> sb(n);
  std::vector<uint8_t> st(n);
  std::vector<uint32_t> sl(n);
  for (uint32_t j = 0; j < n; ++j) {
    sk[j] = o.key[o.order[j]];
    sb[j] = s.box[o.order[j]];
    st[j] = s.is_tri[o.order[j]];
    sl[j] = o.leaf[o.order[j]];
  }
  const SahTreeStats r = sah_tree_from_keys(sk.data(), sb.data(), st.data(), n, sl.data(), leaf_max, k);
  CHECK(r.nodes == o.tree.nodes);
  CHECK(r.depth == o.tree.depth && r.leaves == o.tree.leaves);
  CHECK(close(r.cost, o.tree.cost));
  // prefix-free: with one leaf index per reference the rebuilt tree goes down to single references, and a key
  // that were a prefix of another (zero-padded) could not be split from it where the builder split them
  std::vector<uint32_t> single(n);
  for (uint32_t j = 0; j < n; ++j) single[j] = j;
  const SahTreeStats full = sah_tree_from_keys(sk.data(), sb.data(), st.data(), n, n > 1 ? single.data() : sl.data(), 1u, k);
  CHECK(full.leaves == n && full.depth == o.tree.depth);
  CHECK(o.tree.depth <= o.path_depth || n == 1);
  CHECK(o.path_depth == o.tree.depth);  // the longest path is the height
  // leaves
  uint32_t leaves = 0, covered = 0;
  for (const SahTreeNode& nd : o.tree.nodes) {
    if (nd.left) {
      CHECK(nd.left < nd.count);
      continue;
    }
    CHECK(nd.count >= 1 && nd.count <= std::max(1u, leaf_max));
    CHECK(nd.first == covered);  // preorder visits the leaves in key order, each reference once
    covered += nd.count;
    bool one_kind = true;
    for (uint32_t j = nd.first; j < nd.first + nd.count; ++j) {
      CHECK(sl[j] == leaves);
      if (j > nd.first) {
        CHECK(st[j - 1] <= st[j]);
        if (st[j - 1] == st[j]) CHECK(o.order[j - 1] < o.order[j]);
        one_kind = one_kind && st[j - 1] == st[j];
      }
    }
    if (expect_one_kind) CHECK(one_kind);
    ++leaves;
  }
  CHECK(covered == n && leaves == o.tree.leaves);
  for (uint32_t j = 1; j < n; ++j) CHECK(sl[j] == sl[j - 1] || sl[j] == sl[j - 1] + 1);
  return true;
}

static void check_choice(const Scene& s, uint32_t leaf_max, SahCosts k, uint32_t stack_free, int expect_fallback) {
  const uint32_t n = (uint32_t)s.box.size();
  const std::vector<uint64_t> mk = morton_keys(s);
  const SahChoice c = sah_order_choose(s.box.data(), s.is_tri.data(), mk.data(), n, leaf_max, k, 63u, stack_free);
  if (expect_fallback >= 0) CHECK((int)c.fallback == expect_fallback);
  if (expect_fallback == -2) CHECK(c.fallback != kSahNone);  // any guard
  if (c.fallback == kSahNone) {
    CHECK(c.sah.tree.cost < c.morton.cost);
    CHECK(c.sah.tree.depth <= std::max(c.morton.depth, stack_free));
    CHECK(!c.sah.overflow && c.sah.path_depth <= 63u);
  }
  CHECK(c.morton.leaves >= 1);
}

static Scene random_scene(uint32_t n, uint32_t seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<float> pos(-4.0f, 4.0f), ext(0.0f, 0.6f);
  Scene s;
  for (uint32_t i = 0; i < n; ++i) {
    SahBox b;
    for (int k = 0; k < 3; ++k) {
      const float c = pos(g), e = ext(g);
      b.lo[k] = c - e;
      b.hi[k] = c + e;
    }
    if (i % 7 == 3) b.hi[1] = b.lo[1];  // flat boxes, as axis-aligned triangles have
    s.box.push_back(b);
    s.is_tri.push_back(g() % 3 != 0);
  }
  return s;
}

// the default scene with its emitter: 12 cube triangles, 9 spheres
static Scene default_emitter() {
  static const struct {
    SahBox b;
    int tri;
  } kPrims[21] = {
      {{{-0.75f, 0.25f, 1.25f}, {0.75f, 0.25f, 2.75f}}, 1},  {{{-0.75f, 0.25f, 1.25f}, {0.75f, 0.25f, 2.75f}}, 1},
      {{{-0.75f, 1.75f, 1.25f}, {0.75f, 1.75f, 2.75f}}, 1},  {{{-0.75f, 1.75f, 1.25f}, {0.75f, 1.75f, 2.75f}}, 1},
      {{{-0.75f, 0.25f, 1.25f}, {0.75f, 1.75f, 1.25f}}, 1},  {{{-0.75f, 0.25f, 1.25f}, {0.75f, 1.75f, 1.25f}}, 1},
      {{{-0.75f, 0.25f, 2.75f}, {0.75f, 1.75f, 2.75f}}, 1},  {{{-0.75f, 0.25f, 2.75f}, {0.75f, 1.75f, 2.75f}}, 1},
      {{{-0.75f, 0.25f, 1.25f}, {-0.75f, 1.75f, 2.75f}}, 1}, {{{-0.75f, 0.25f, 1.25f}, {-0.75f, 1.75f, 2.75f}}, 1},
      {{{0.75f, 0.25f, 1.25f}, {0.75f, 1.75f, 2.75f}}, 1},   {{{0.75f, 0.25f, 1.25f}, {0.75f, 1.75f, 2.75f}}, 1},
      {{{-4.0f, 0.0f, -1.0f}, {-2.0f, 2.0f, 1.0f}}, 0},      {{{-2.0f, 0.0f, -1.0f}, {0.0f, 2.0f, 1.0f}}, 0},
      {{{0.0f, 0.0f, -1.0f}, {2.0f, 2.0f, 1.0f}}, 0},        {{{2.0f, 0.0f, -1.0f}, {4.0f, 2.0f, 1.0f}}, 0},
      {{{-3.0f, 0.0f, -3.0f}, {-1.0f, 2.0f, -1.0f}}, 0},     {{{-1.0f, 0.0f, -3.0f}, {1.0f, 2.0f, -1.0f}}, 0},
      {{{1.0f, 0.0f, -3.0f}, {3.0f, 2.0f, -1.0f}}, 0},       {{{-1.0f, 0.0f, -5.0f}, {1.0f, 2.0f, -3.0f}}, 0},
      {{{-0.5f, 2.0f, 0.5f}, {0.5f, 3.0f, 1.5f}}, 0},
  };
  Scene s;
  for (const auto& p : kPrims) {
    s.box.push_back(p.b);
    s.is_tri.push_back((uint8_t)p.tri);
  }
  return s;
}

int main() {
  const SahCosts k0;  // 2 : 1 : 1.3
  const uint32_t leaf_sizes[] = {1u, 2u, 4u, 8u, 16u};
  // n = 1, 2, 9
  for (uint32_t n : {1u, 2u, 9u}) {
    const Scene s = random_scene(n, 10u + n);
    for (uint32_t lm : leaf_sizes) {
      CHECK(check_order(s, lm, k0, 64u, false));
      CHECK(check_order(s, lm, k0, 63u, false));
      check_choice(s, lm, k0, 12u, -1);
    }
  }
  {  // one reference: key 0, leaf 0, depth 0
    const Scene s = random_scene(1, 5u);
    const SahOrder o = sah_order_build(s.box.data(), s.is_tri.data(), 1u, 8u, k0);
    CHECK(o.key[0] == 0ull && o.leaf[0] == 0u && o.tree.depth == 0u && o.tree.leaves == 1u);
  }
  {  // 12 references with identical centres: no sweep position separates them; the median by index
    Scene s;
    for (uint32_t i = 0; i < 12; ++i) {
      const float e = 0.125f * (float)(1 + i % 5);
      s.box.push_back(SahBox{{1.0f - e, 2.0f - 2.0f * e, -1.0f - e}, {1.0f + e, 2.0f + 2.0f * e, -1.0f + e}});
      s.is_tri.push_back(i % 2);
    }
    for (uint32_t lm : leaf_sizes) {
      CHECK(check_order(s, lm, k0, 63u, false));
      check_choice(s, lm, k0, 12u, -1);
    }
    const SahOrder o = sah_order_build(s.box.data(), s.is_tri.data(), 12u, 1u, k0);
    CHECK(o.tree.depth == 4u);  // medians: 12 -> 6 -> 3 -> 2 -> 1
    CHECK(o.order[0] == 0u && o.order[11] == 11u);
  }
  {  // a nested chain 70 deep: 71 segments [0, 2^-i] on the x axis.  Every box of every subset has area 0, so
     // every split costs the same and the first position wins: the reference with the lowest centre is split
     // off, 70 times.  (With areas that shrink by a constant factor the sweep splits off three at a time, and a
     // chain of single references would need a factor of about n per level: beyond float's range at n = 70.)
    Scene s;
    for (uint32_t i = 0; i < 71; ++i) {
      s.box.push_back(SahBox{{0.0f, 0.0f, 0.0f}, {std::ldexp(1.0f, -(int)i), 0.0f, 0.0f}});
      s.is_tri.push_back(i % 2);
    }
    const SahOrder o = sah_order_build(s.box.data(), s.is_tri.data(), 71u, 1u, k0, 63u);
    CHECK(o.overflow && o.path_depth == 70u && o.tree.depth == 70u);
    CHECK(!check_order(s, 1u, k0, 63u, false));
    // (a leaf range of 16 ends the chain 15 levels early, 4 of them its own: 59 levels, which the depth guard refuses)
    for (uint32_t lm : leaf_sizes) check_choice(s, lm, k0, 12u, lm <= 8u ? (int)kSahPathDepth : -2);
    // the first 40 of them: short enough for the key, deeper than the Morton tree and than the stack
    Scene t;
    t.box.assign(s.box.begin(), s.box.begin() + 40);
    t.is_tri.assign(s.is_tri.begin(), s.is_tri.begin() + 40);
    CHECK(check_order(t, 1u, k0, 63u, false));
    const std::vector<uint64_t> mk = morton_keys(t);
    const SahChoice c = sah_order_choose(t.box.data(), t.is_tri.data(), mk.data(), 40u, 1u, k0, 63u, 12u);
    CHECK(c.sah.tree.depth == 39u && c.morton.depth < 39u && c.fallback == kSahTreeDepth);
    // ... and with room on the stack, no cheaper than the Morton tree (both cost 0)
    const SahChoice c2 = sah_order_choose(t.box.data(), t.is_tri.data(), mk.data(), 40u, 1u, k0, 63u, 64u);
    CHECK(c2.fallback == kSahCost);
  }
  {  // the default scene with its emitter
    const Scene s = default_emitter();
    const float cns[] = {1.0f, 1.5f, 2.0f, 3.0f, 4.0f};
    const float css[] = {1.0f, 1.3f};
    for (float cn : cns)
      for (float cs : css) {
        const SahCosts k{cn, 1.0f, cs};
        CHECK(check_order(s, 8u, k, 63u, true));
        check_choice(s, 8u, k, 12u, (int)kSahNone);
        const std::vector<uint64_t> mk = morton_keys(s);
        const SahChoice c = sah_order_choose(s.box.data(), s.is_tri.data(), mk.data(), 21u, 8u, k, 63u, 12u);
        std::printf("default_emitter Cn %.1f Cs %.1f: SAH cost %.3f depth %u leaves %u; Morton cost %.3f depth %u leaves %u\n",
                    cn, cs, c.sah.tree.cost, c.sah.tree.depth, c.sah.tree.leaves, c.morton.cost, c.morton.depth,
                    c.morton.leaves);
      }
    for (uint32_t lm : leaf_sizes) CHECK(check_order(s, lm, k0, 63u, lm > 1u));
  }
  // random scenes of 8 .. 430 boxes
  for (uint32_t i = 0; i < 200; ++i) {
    const uint32_t n = i < 8 ? (i % 2 ? 430u : 8u) : 8u + (i * 2654435761u) % 423u;
    const Scene s = random_scene(n, 1000u + i);
    const uint32_t lm = leaf_sizes[i % 5];
    const SahCosts k{1.0f + 0.5f * (float)(i % 7), 1.0f, i % 2 ? 1.3f : 1.0f};
    CHECK(check_order(s, lm, k, 63u, false));
    check_choice(s, lm, k, 12u, -1);
  }
  std::printf("%s (%d failures)\n", fails ? "FAILED" : "ok", fails);
  return fails ? 1 : 0;
}
