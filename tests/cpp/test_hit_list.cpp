// The list of sptr_query_multi_hit (csrc/hit_list.h) on the host: the text k_rayquery_multi calls.
// Candidate streams — random t, runs of exact ties, duplicates of one key under several references, +0.0 and
// -0.0, more and fewer candidates than the list holds — are fed in many permutations into lists of every
// capacity 1 .. 16 and every k <= capacity, and each list is compared with a sort of the stream: the first k
// distinct keys in ascending (t, geomID, primID).  The storage sits between guard values, and entries at and
// beyond k are guards too: no write outside the k entries.  A sphere's two evaluations (hit_list_sphere) are
// checked on a table of roots.  The exit status is the number of failures.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hit_list.h"

static int fails = 0;
static uint32_t lcg(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return s;
}
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (fails < 20) std::printf("FAIL line %d: %s\n", __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

constexpr uint32_t kGuardT = 0x7FC0DEADu, kGuardRef = 0xA5A5A5A5u;
constexpr int kPad = 8, kMaxCap = 16;

// the list's storage: cap entries inside guard runs, every access checked against the capacity
struct Store {
  std::vector<uint32_t> w;
  int cap;
  explicit Store(int c) : w(2 * (c + 2 * kPad)), cap(c) {
    for (size_t i = 0; i < w.size(); i += 2) {
      w[i] = kGuardT;
      w[i + 1] = kGuardRef;
    }
  }
  float t(uint32_t i) const {
    CHECK((int)i < cap);
    float f;
    std::memcpy(&f, &w[2 * (kPad + i)], 4);
    return f;
  }
  uint32_t ref(uint32_t i) const {
    CHECK((int)i < cap);
    return w[2 * (kPad + i) + 1];
  }
  void set(uint32_t i, float t, uint32_t r) {
    CHECK((int)i < cap);
    w[2 * (kPad + i)] = bits(t);
    w[2 * (kPad + i) + 1] = r;
  }
  bool guard(int e) const { return w[2 * e] == kGuardT && w[2 * e + 1] == kGuardRef; }  // e: absolute entry
};

struct Cand {
  float t;
  uint32_t ref;
};
// references 0 .. 255 name 64 primitives: refs r and r + 64 k are one primitive (split references), and the ids
// are no monotone function of the reference
static uint64_t key_of(uint32_t ref) {
  const uint32_t p = ref & 63u;
  return ((uint64_t)((p * 37u) & 7u) << 32) | ((p * 11u) & 63u) | ((uint64_t)(ref >> 31) << 8);
}
struct Key {
  mutable long calls = 0;
  uint64_t operator()(uint32_t ref) const {
    ++calls;
    return key_of(ref);
  }
};

static bool less(const Cand& a, const Cand& b) { return a.t < b.t || (a.t == b.t && key_of(a.ref) < key_of(b.ref)); }

static void run(const std::vector<Cand>& stream, int cap, uint32_t k, bool ties) {
  std::vector<Cand> want = stream;
  std::stable_sort(want.begin(), want.end(), less);
  want.erase(std::unique(want.begin(), want.end(), [](const Cand& a, const Cand& b) { return a.t == b.t && key_of(a.ref) == key_of(b.ref); }),
             want.end());
  const uint32_t expect = std::min<uint32_t>(k, (uint32_t)want.size());
  Store s(cap);
  Key key;
  uint32_t n = 0;
  for (const Cand& c : stream) {
    sptr::hit_list_insert(s, n, k, c.t, c.ref, key);
    CHECK(n <= k);
    const float b = sptr::hit_list_bound(s, n, k, 1e30f);
    CHECK(n < k ? b == 1e30f : b == s.t(k - 1u));
  }
  if (!ties) CHECK(key.calls == 0);  // the ids are resolved only on an exact tie
  CHECK(n == expect);
  for (uint32_t i = 0; i < n; ++i) {
    CHECK(s.t(i) == want[i].t);  // (as float: +0.0 and -0.0 are one distance)
    CHECK(key_of(s.ref(i)) == key_of(want[i].ref));
  }
  for (int e = 0; e < cap + 2 * kPad; ++e)
    if (e < kPad || e >= kPad + (int)n) CHECK(s.guard(e));
}

static void permutations(std::vector<Cand> stream, uint32_t& seed, bool ties) {
  for (int cap = 1; cap <= kMaxCap; ++cap)
    for (uint32_t k = 1; k <= (uint32_t)cap; ++k)
      for (int p = 0; p < 6; ++p) {
        if (p == 1) std::sort(stream.begin(), stream.end(), less);
        else if (p == 2) std::reverse(stream.begin(), stream.end());
        else if (p > 2)
          for (size_t i = stream.size(); i > 1; --i) std::swap(stream[i - 1], stream[lcg(seed) % i]);
        run(stream, cap, k, ties);
      }
}

int main() {
  uint32_t seed = 12345u;
  for (int len : {0, 1, 2, 3, 5, 15, 16, 17, 40, 100}) {
    // random, distinct t: no key is ever resolved
    std::vector<Cand> a;
    for (int i = 0; i < len; ++i) a.push_back({float(i * 7 % 101) + float(i) / 256.0f, lcg(seed) & 255u});
    permutations(a, seed, false);
    // runs of exact ties, with duplicates of one key under several references and both flags
    std::vector<Cand> b;
    for (int i = 0; i < len; ++i)
      b.push_back({float((lcg(seed) >> 8) % 4u) * 0.5f, (lcg(seed) & 255u) | ((lcg(seed) & 0x100u) ? sptr::kHitSecond : 0u)});
    permutations(b, seed, true);
    // every candidate at one distance, written as +0.0 or -0.0
    std::vector<Cand> z;
    for (int i = 0; i < len; ++i) z.push_back({(lcg(seed) & 0x200u) ? 0.0f : -0.0f, lcg(seed) & 255u});
    permutations(z, seed, true);
    // one key, many times
    std::vector<Cand> d(len, Cand{2.5f, 7u});
    for (int i = 0; i < len; ++i) d[i].ref = 7u + 64u * (uint32_t)(i % 4);
    permutations(d, seed, true);
  }
  // a sphere's candidates: the closest-hit rule (the first root inside the open interval, t > 0) evaluated twice
  struct Roots {
    float t1, t2, tnear, tfar;
    int hits;
    float a, b;
  };
  const Roots table[] = {{1.0f, 3.0f, 0.0f, 10.0f, 2, 1.0f, 3.0f},  {-1.0f, 3.0f, 0.0f, 10.0f, 1, 3.0f, 0.0f},
                         {2.0f, 2.0f, 0.0f, 10.0f, 1, 2.0f, 0.0f},  {1.0f, 3.0f, 0.0f, 3.0f, 1, 1.0f, 0.0f},
                         {1.0f, 3.0f, 1.0f, 10.0f, 1, 3.0f, 0.0f},  {1.0f, 3.0f, 3.0f, 10.0f, 0, 0.0f, 0.0f},
                         {-3.0f, -1.0f, -5.0f, 10.0f, 0, 0.0f, 0.0f}, {-1.0f, 3.0f, -2.0f, 10.0f, 0, 0.0f, 0.0f}};  // (the last: t1 < 0 is chosen, then refused)
  for (const Roots& r : table) {
    std::vector<Cand> got;
    auto hit = [&](float tn, float tf, float& t) {
      float tt = -1.0f;
      if (r.t1 > tn && r.t1 < tf) tt = r.t1;
      else if (r.t2 > tn && r.t2 < tf) tt = r.t2;
      if (!(tt > 0.0f && tt < tf)) return false;
      t = tt;
      return true;
    };
    sptr::hit_list_sphere(hit, r.tnear, r.tfar, [&](float t, uint32_t flag) { got.push_back({t, flag}); });
    CHECK((int)got.size() == r.hits);
    if (r.hits >= 1 && got.size() >= 1) CHECK(got[0].t == r.a && got[0].ref == 0u);
    if (r.hits == 2 && got.size() == 2) CHECK(got[1].t == r.b && got[1].ref == sptr::kHitSecond);
  }
  std::printf("hit_list: %d failures\n", fails);
  return fails > 255 ? 255 : fails;
}
