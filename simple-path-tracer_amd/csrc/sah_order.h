// sah_order.h — SAH order for the BVH2 of an LDS-staged scene, as plain host C++ (no HIP; unit-tested by
// tests/cpp/test_sah_order.cpp).
//
// The device build (kernels_lbvh.hip) sorts 64-bit keys and k_karras turns the sorted keys into a binary
// radix tree: a range of keys is split where their highest differing bit changes.  The Morton keys of a
// scene of a few dozen primitives give a poor tree (leaves that mix spheres and triangles, boxes that
// overlap).  This builder makes a top-down sweep-SAH tree over the same reference boxes and hands it to
// the same device code as keys: a reference's key is its root-to-leaf path (left 0, right 1, most
// significant bit first, zero-padded).  Paths are prefix-free, so two keys first differ at the depth of
// their lowest common ancestor and the radix tree over the sorted keys is this tree, node for node.
// Node numbering, parents, refit order and the N - 1 node allocation stay what they were.
//
// The tree goes down to single references (refit and the node allocation need the whole binary tree); which
// subtrees the walk treats as leaf ranges is told apart by a leaf index per reference: a child range is a
// leaf range iff its first and last reference carry the same index.
//
// Cost model (the walk of kernels_wavefront.hip, bvh2_walk: a node step tests both child boxes, a leaf
// child is tested as soon as its box is hit): with A the half surface area of a box,
//   leaf range under box A:   A * (Ct * triangles + Cs * spheres)
//   inner node under box A:   A * Cn + cost(left) + cost(right)
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sptr {

struct SahCosts {
  float cn = 2.0f, ct = 1.0f, cs = 1.3f;  // node step, triangle test, sphere test
};

// why the last upload's tree is in Morton order (sptr_tree_info)
enum SahFallback : uint32_t {
  kSahNone = 0,        // SAH order in use
  kSahOff = 1,         // Morton order asked for (sptr_set_tree_order)
  kSahNotStaged = 2,   // not an LDS-staged scene with leaf ranges and unsplit references
  kSahPathDepth = 3,   // a path longer than the key
  kSahTreeDepth = 4,   // deeper than the Morton tree and than the walk's LDS stack
  kSahCost = 5,        // modelled cost not below the Morton tree's
};

struct SahBox {
  float lo[3], hi[3];
};

// what a tree over the sorted references looks like: preorder list of inner nodes and leaf ranges
struct SahTreeNode {
  uint32_t first, count, left;  // sorted positions [first, first + count); left = size of the left child, 0 for a leaf range
  bool operator==(const SahTreeNode& o) const { return first == o.first && count == o.count && left == o.left; }
};

struct SahTreeStats {
  double cost = 0.0;        // modelled cost (above)
  uint32_t depth = 0;       // height of the binary tree down to single references (one reference: 0)
  uint32_t leaves = 0;      // leaf ranges
  std::vector<SahTreeNode> nodes;  // the walk's tree, preorder (left first)
};

struct SahOrder {
  std::vector<uint64_t> key;   // per reference: the path key (in the top max_bits bits of the word)
  std::vector<uint32_t> leaf;  // per reference: index of its leaf range, numbered in key order
  std::vector<uint32_t> order; // references in key order
  SahTreeStats tree;           // the builder's own tree
  uint32_t path_depth = 0;     // longest path (bits)
  bool overflow = false;       // a path did not fit into max_bits: the keys are not usable
};

namespace sah_detail {

inline SahBox box_empty() { return SahBox{{3.4e38f, 3.4e38f, 3.4e38f}, {-3.4e38f, -3.4e38f, -3.4e38f}}; }
inline void box_grow(SahBox& a, const SahBox& b) {
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = std::min(a.lo[k], b.lo[k]);
    a.hi[k] = std::max(a.hi[k], b.hi[k]);
  }
}
inline double half_area(const SahBox& b) {
  const double dx = (double)b.hi[0] - (double)b.lo[0], dy = (double)b.hi[1] - (double)b.lo[1],
               dz = (double)b.hi[2] - (double)b.lo[2];
  if (dx < 0.0 || dy < 0.0 || dz < 0.0) return 0.0;
  return dx * dy + dy * dz + dz * dx;
}
inline double centre(const SahBox& b, int a) { return 0.5 * ((double)b.lo[a] + (double)b.hi[a]); }

struct Builder {
  const SahBox* box;
  const uint8_t* is_tri;
  uint32_t leaf_max;
  SahCosts k;
  uint32_t max_bits;
  SahOrder* out;
  uint32_t next_leaf = 0;

  double weight(const uint32_t* ids, uint32_t n) const {
    double w = 0.0;
    for (uint32_t i = 0; i < n; ++i) w += is_tri[ids[i]] ? k.ct : k.cs;
    return w;
  }
  void emit_key(uint32_t ref, uint64_t path, uint32_t depth) {
    out->key[ref] = path;
    out->path_depth = std::max(out->path_depth, depth);
    out->order.push_back(ref);
  }
  static uint64_t child_path(uint64_t path, uint32_t depth, uint32_t max_bits, bool right, bool& overflow) {
    if (depth >= max_bits) {
      overflow = true;
      return path;
    }
    return right ? (path | (1ull << (63u - depth))) : path;
  }
  // inside a leaf range: the references stay in the given order, split at the median down to single ones;
  // returns the height
  uint32_t sub_leaf(const uint32_t* ids, uint32_t n, uint64_t path, uint32_t depth, uint32_t leaf) {
    if (n == 1) {
      out->leaf[ids[0]] = leaf;
      emit_key(ids[0], path, depth);
      return 0;
    }
    const uint32_t nl = (n + 1) / 2;
    const uint32_t hl = sub_leaf(ids, nl, child_path(path, depth, max_bits, false, out->overflow), depth + 1, leaf);
    const uint32_t hr = sub_leaf(ids + nl, n - nl, child_path(path, depth, max_bits, true, out->overflow), depth + 1, leaf);
    return std::max(hl, hr) + 1;
  }
  // best sweep split of ids (n >= 2): ids is left reordered with the left child's references first;
  // returns the left count and the children's summed cost estimate
  uint32_t best_split(std::vector<uint32_t>& ids, double& child_cost) const {
    const uint32_t n = (uint32_t)ids.size();
    bool same = true;
    for (int a = 0; a < 3 && same; ++a)
      for (uint32_t i = 1; i < n && same; ++i) same = centre(box[ids[i]], a) == centre(box[ids[0]], a);
    std::vector<uint32_t> best_ids;
    double best = 0.0;
    uint32_t best_nl = 0;
    int best_axis = 0;
    auto by_axis = [&](std::vector<uint32_t>& s, int a) {
      std::sort(s.begin(), s.end(), [&](uint32_t x, uint32_t y) {
        const double cx = centre(box[x], a), cy = centre(box[y], a);
        return cx != cy ? cx < cy : x < y;
      });
    };
    if (!same) {
      std::vector<uint32_t> s(ids);
      std::vector<double> right_cost(n);
      for (int a = 0; a < 3; ++a) {
        by_axis(s, a);
        SahBox b = box_empty();
        double w = 0.0;
        for (uint32_t i = n - 1; i >= 1; --i) {
          box_grow(b, box[s[i]]);
          w += is_tri[s[i]] ? k.ct : k.cs;
          right_cost[i] = half_area(b) * w;
        }
        b = box_empty();
        w = 0.0;
        for (uint32_t nl = 1; nl < n; ++nl) {
          box_grow(b, box[s[nl - 1]]);
          w += is_tri[s[nl - 1]] ? k.ct : k.cs;
          const double c = half_area(b) * w + right_cost[nl];
          if (best_nl == 0 || c < best) {  // ties: the first axis, then the first position
            best = c;
            best_nl = nl;
            best_axis = a;
          }
        }
      }
      best_ids = ids;
      by_axis(best_ids, best_axis);
    }
    if (best_nl == 0) {  // all centres equal: the median by index
      best_ids = ids;
      std::sort(best_ids.begin(), best_ids.end());
      best_nl = (n + 1) / 2;
      SahBox bl = box_empty(), br = box_empty();
      for (uint32_t i = 0; i < n; ++i) box_grow(i < best_nl ? bl : br, box[best_ids[i]]);
      best = half_area(bl) * weight(best_ids.data(), best_nl) + half_area(br) * weight(best_ids.data() + best_nl, n - best_nl);
    }
    ids = best_ids;
    child_cost = best;
    return best_nl;
  }
  // returns the height; cost: the subtree's modelled cost
  uint32_t build(std::vector<uint32_t> ids, uint64_t path, uint32_t depth, double& cost) {
    const uint32_t n = (uint32_t)ids.size();
    const uint32_t first = (uint32_t)out->order.size();
    SahBox b = box_empty();
    for (uint32_t r : ids) box_grow(b, box[r]);
    const double A = half_area(b);
    const double leaf_cost = A * weight(ids.data(), n);
    double child_cost = 0.0;
    uint32_t nl = 0;
    if (n >= 2) nl = best_split(ids, child_cost);
    if (n == 1 || (n <= leaf_max && leaf_cost <= (double)k.cn * A + child_cost)) {
      // a leaf range: spheres first, then triangles, each by index
      std::sort(ids.begin(), ids.end(), [&](uint32_t x, uint32_t y) {
        return is_tri[x] != is_tri[y] ? is_tri[x] < is_tri[y] : x < y;
      });
      out->tree.nodes.push_back(SahTreeNode{first, n, 0u});
      ++out->tree.leaves;
      cost = leaf_cost;
      return sub_leaf(ids.data(), n, path, depth, next_leaf++);
    }
    const size_t me = out->tree.nodes.size();
    out->tree.nodes.push_back(SahTreeNode{first, n, nl});
    double cl = 0.0, cr = 0.0;
    const uint32_t hl = build(std::vector<uint32_t>(ids.begin(), ids.begin() + nl),
                              child_path(path, depth, max_bits, false, out->overflow), depth + 1, cl);
    const uint32_t hr = build(std::vector<uint32_t>(ids.begin() + nl, ids.end()),
                              child_path(path, depth, max_bits, true, out->overflow), depth + 1, cr);
    (void)me;
    cost = (double)k.cn * A + cl + cr;
    return std::max(hl, hr) + 1;
  }
};

inline int clz64(uint64_t x) { return x ? __builtin_clzll(x) : 64; }

}  // namespace sah_detail

// The SAH order of n references (n >= 1).  box / is_tri: per reference.  leaf_max: most references in a leaf
// range (1 .. 16).  max_bits: key bits available for the path (<= 64); the keys use the top max_bits bits.
inline SahOrder sah_order_build(const SahBox* box, const uint8_t* is_tri, uint32_t n, uint32_t leaf_max, SahCosts k,
                                uint32_t max_bits = 64) {
  SahOrder o;
  o.key.assign(n, 0ull);
  o.leaf.assign(n, 0u);
  o.order.reserve(n);
  if (n == 0) return o;
  sah_detail::Builder b{box, is_tri, std::max(1u, leaf_max), k, std::min(max_bits, 64u), &o};
  std::vector<uint32_t> ids(n);
  for (uint32_t i = 0; i < n; ++i) ids[i] = i;
  o.tree.depth = b.build(std::move(ids), 0ull, 0u, o.tree.cost);
  return o;
}

// The tree k_karras builds over sorted keys (key[i], i = sorted position; equal keys split by position, as
// k_karras's delta does), as the walk sees it, with the model's cost.  box / is_tri: per sorted position.
// leaf_idx != null: a range is a leaf range iff its ends carry the same index; else iff it holds at most
// leaf_max references.
inline SahTreeStats sah_tree_from_keys(const uint64_t* key, const SahBox* box, const uint8_t* is_tri, uint32_t n,
                                       const uint32_t* leaf_idx, uint32_t leaf_max, SahCosts k) {
  SahTreeStats t;
  if (n == 0) return t;
  struct Rec {
    const uint64_t* key;
    const SahBox* box;
    const uint8_t* is_tri;
    const uint32_t* leaf_idx;
    uint32_t leaf_max;
    SahCosts k;
    SahTreeStats* t;
    // first position of the right child of [lo, hi]
    uint32_t split(uint32_t lo, uint32_t hi) const {
      if (key[lo] != key[hi]) {
        const uint64_t bit = 1ull << (63 - sah_detail::clz64(key[lo] ^ key[hi]));
        uint32_t a = lo, b = hi;  // key[a] has the bit clear, key[b] has it set
        while (b - a > 1) {
          const uint32_t m = a + (b - a) / 2;
          if (key[m] & bit) b = m;
          else a = m;
        }
        return b;
      }
      const uint32_t bit = 1u << (31 - __builtin_clz(lo ^ hi));
      return (hi & ~(bit - 1u));
    }
    // height of the binary tree below [lo, hi]
    uint32_t height(uint32_t lo, uint32_t hi) const {
      if (lo == hi) return 0;
      const uint32_t s = split(lo, hi);
      return std::max(height(lo, s - 1), height(s, hi)) + 1;
    }
    uint32_t walk(uint32_t lo, uint32_t hi, double& cost) const {
      const uint32_t n = hi - lo + 1;
      SahBox b = sah_detail::box_empty();
      double w = 0.0;
      for (uint32_t i = lo; i <= hi; ++i) {
        sah_detail::box_grow(b, box[i]);
        w += is_tri[i] ? k.ct : k.cs;
      }
      const double A = sah_detail::half_area(b);
      const bool leaf = leaf_idx ? leaf_idx[lo] == leaf_idx[hi] : n <= leaf_max;
      if (leaf) {
        t->nodes.push_back(SahTreeNode{lo, n, 0u});
        ++t->leaves;
        cost = A * w;
        return height(lo, hi);
      }
      const uint32_t s = split(lo, hi);
      t->nodes.push_back(SahTreeNode{lo, n, s - lo});
      double cl = 0.0, cr = 0.0;
      const uint32_t hl = walk(lo, s - 1, cl), hr = walk(s, hi, cr);
      cost = (double)k.cn * A + cl + cr;
      return std::max(hl, hr) + 1;
    }
  };
  Rec r{key, box, is_tri, leaf_idx, std::max(1u, leaf_max), k, &t};
  t.depth = r.walk(0, n - 1, t.cost);
  return t;
}

// What build_lbvh decides with: the SAH order of the references against their Morton order.
struct SahChoice {
  SahOrder sah;
  SahTreeStats morton;
  uint32_t fallback = kSahNone;
};
// morton_key: per reference.  stack_free: tree depth the walk holds without spilling its stack.
inline SahChoice sah_order_choose(const SahBox* box, const uint8_t* is_tri, const uint64_t* morton_key, uint32_t n,
                                  uint32_t leaf_max, SahCosts k, uint32_t max_bits, uint32_t stack_free) {
  SahChoice c;
  std::vector<uint32_t> ord(n);
  for (uint32_t i = 0; i < n; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return morton_key[x] < morton_key[y]; });
  std::vector<uint64_t> mk(n);
  std::vector<SahBox> mb(n);
  std::vector<uint8_t> mt(n);
  for (uint32_t i = 0; i < n; ++i) {
    mk[i] = morton_key[ord[i]];
    mb[i] = box[ord[i]];
    mt[i] = is_tri[ord[i]];
  }
  c.morton = sah_tree_from_keys(mk.data(), mb.data(), mt.data(), n, nullptr, leaf_max, k);
  c.sah = sah_order_build(box, is_tri, n, leaf_max, k, max_bits);
  if (c.sah.overflow) c.fallback = kSahPathDepth;
  else if (c.sah.tree.depth > std::max(c.morton.depth, stack_free)) c.fallback = kSahTreeDepth;
  else if (!(c.sah.tree.cost < c.morton.cost)) c.fallback = kSahCost;
  return c;
}

}  // namespace sptr
