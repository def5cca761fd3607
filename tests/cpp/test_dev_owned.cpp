// dev_owned.h's owners against a fake HIP runtime: host malloc / free behind hipMalloc / hipFree and
// counted tokens behind the handles, with a set of what is live.  A double or unknown free aborts, and
// the program exits 0 only if nothing is live at the end.  Links no HIP runtime:
//   g++ -std=c++20 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I<csrc>
#include "dev_owned.h"

#include <cstdio>
#include <cstdlib>
#include <set>

namespace {
std::set<void*> g_blocks;   // live device blocks
std::set<void*> g_handles;  // live events, streams, graphs
bool g_fail_next_malloc = false;
size_t g_max_blocks = 0;  // most blocks live at once since it was last zeroed
int g_failed = 0;

void drop(std::set<void*>& live, void* p, const char* what) {
  if (live.erase(p) != 1) {
    std::fprintf(stderr, "%s: double or unknown free of %p\n", what, p);
    std::abort();
  }
  std::free(p);
}
template <class H>
hipError_t make_handle(H* out) {
  void* p = std::malloc(1);
  g_handles.insert(p);
  *out = static_cast<H>(p);
  return hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
  if (g_fail_next_malloc) {
    g_fail_next_malloc = false;
    return hipErrorOutOfMemory;
  }
  *p = std::malloc(n);
  g_blocks.insert(*p);
  if (g_blocks.size() > g_max_blocks) g_max_blocks = g_blocks.size();
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  drop(g_blocks, p, "hipFree");
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return make_handle(e); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make_handle(e); }
hipError_t hipEventDestroy(hipEvent_t e) {
  drop(g_handles, e, "hipEventDestroy");
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  drop(g_handles, s, "hipStreamDestroy");
  return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t g) {
  drop(g_handles, g, "hipGraphDestroy");
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t g) {
  drop(g_handles, g, "hipGraphExecDestroy");
  return hipSuccess;
}
}

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      ++g_failed;                                                   \
    }                                                               \
  } while (0)

using namespace sptr;

static void test_ensure() {
  {
    DevBuf b;
    CHECK(b.ensure(0) == hipSuccess && b.p && b.bytes == 16);
  }
  CHECK(g_blocks.empty());
  DevBuf b;
  CHECK(b.ensure(100) == hipSuccess && b.bytes == 100);
  void* p = b.p;
  CHECK(b.ensure(100) == hipSuccess && b.p == p && b.bytes == 100);  // twice: kept
  CHECK(b.ensure(40) == hipSuccess && b.p == p && b.bytes == 100);   // smaller: kept, with its size
  CHECK(b.ensure(0) == hipSuccess && b.p == p && b.bytes == 100);
  g_max_blocks = 0;
  CHECK(b.ensure(101) == hipSuccess && b.p && b.bytes == 101);  // larger: the old block goes first
  CHECK(g_max_blocks == 1 && g_blocks.size() == 1 && g_blocks.count(b.p) == 1);
  g_fail_next_malloc = true;
  CHECK(b.ensure(1000) == hipErrorOutOfMemory && b.p == nullptr && b.bytes == 0 && g_blocks.empty());
  CHECK(b.ensure(1000) == hipSuccess && b.p && b.bytes == 1000);  // still usable
  g_fail_next_malloc = true;
  DevBuf e;
  CHECK(e.ensure(8) == hipErrorOutOfMemory && e.p == nullptr && e.bytes == 0);  // an empty one that fails
  b.release();
  CHECK(b.p == nullptr && b.bytes == 0 && g_blocks.empty());
  b.release();  // twice
  CHECK(g_blocks.empty());
}

static void test_buf_moves() {
  DevBuf a, b;
  CHECK(a.ensure(32) == hipSuccess && b.ensure(64) == hipSuccess && g_blocks.size() == 2);
  void *pa = a.p, *pb = b.p;
  DevBuf c(std::move(a));  // move-construct: the source is empty
  CHECK(c.p == pa && c.bytes == 32 && a.p == nullptr && a.bytes == 0 && g_blocks.size() == 2);
  b = std::move(c);  // onto a non-empty target: its old block is freed, once
  CHECK(b.p == pa && b.bytes == 32 && c.p == nullptr && c.bytes == 0);
  CHECK(g_blocks.size() == 1 && g_blocks.count(pa) == 1 && g_blocks.count(pb) == 0);
  DevBuf& self = b;
  b = std::move(self);  // self-move: harmless
  CHECK(b.p == pa && b.bytes == 32 && g_blocks.size() == 1);
  a = std::move(c);  // empty onto empty
  CHECK(a.p == nullptr && g_blocks.size() == 1);
}

static void test_handles() {
  {
    DevEvent e;
    CHECK(!e && hipEventCreate(e.put()) == hipSuccess && e && g_handles.size() == 1);
  }
  CHECK(g_handles.empty());  // the destructor
  DevEvent a, b;
  CHECK(hipEventCreate(a.put()) == hipSuccess && hipEventCreateWithFlags(b.put(), 0) == hipSuccess);
  const hipEvent_t ha = a, hb = b;  // the implicit conversion
  CHECK(ha && hb && ha != hb && g_handles.size() == 2);
  DevEvent c(std::move(a));
  CHECK(c == ha && !a && g_handles.size() == 2);
  b = std::move(c);  // onto a non-empty target: its old event is destroyed, once
  CHECK(b == ha && !c && g_handles.size() == 1 && g_handles.count(hb) == 0);
  DevEvent& self = b;
  b = std::move(self);
  CHECK(b == ha && g_handles.size() == 1);
  b.reset();
  CHECK(!b && g_handles.empty());
  b.reset();  // twice
  CHECK(hipEventCreate(b.put()) == hipSuccess && b && g_handles.size() == 1);  // put() after a reset
  // the other three kinds share the template: one of each through its own destroy call
  DevStream s;
  DevGraph g;
  DevGraphExec x;
  make_handle(s.put());
  make_handle(g.put());
  make_handle(x.put());
  CHECK(g_handles.size() == 4);
}

// shaped like the library's context: arrays of buffers, a grown event pool, a nested struct, typed scratch
struct Nested {
  DevBuf in, out;
  DevEvent ev[3];
};
struct Aggregate {
  DevStream stream;
  DevGraph graph;
  DevGraphExec exec;
  DevBuf bufs[2][3];
  std::vector<DevEvent> pool;
  Nested n;
};

static void test_aggregate() {
  {
    Aggregate a;
    make_handle(a.stream.put());
    make_handle(a.graph.put());
    make_handle(a.exec.put());
    for (auto& row : a.bufs)
      for (DevBuf& b : row) CHECK(b.ensure(24) == hipSuccess);
    for (int i = 0; i < 100; ++i) {  // grown one by one: the vector reallocates and moves its events
      DevEvent e;
      CHECK(hipEventCreate(e.put()) == hipSuccess);
      a.pool.push_back(std::move(e));
    }
    CHECK(a.n.in.ensure(8) == hipSuccess);  // (out stays empty)
    for (DevEvent& e : a.n.ev) CHECK(hipEventCreate(e.put()) == hipSuccess);
    CHECK(g_blocks.size() == 7 && g_handles.size() == 106);
    Aggregate b(std::move(a));  // the whole aggregate moves; a is left empty
    CHECK(!a.stream && a.bufs[1][2].p == nullptr && a.pool.empty());
    CHECK(g_blocks.size() == 7 && g_handles.size() == 106);
    DevTemps t;
    float* f = nullptr;
    char* z = nullptr;
    CHECK(t.alloc(&f, 10) == hipSuccess && f && t.bufs.back().bytes == 40);
    CHECK(t.alloc(&z, 0) == hipSuccess && z && t.bufs.back().bytes == 16);
    g_fail_next_malloc = true;
    CHECK(t.alloc(&f, 10) == hipErrorOutOfMemory && f == nullptr && t.bufs.size() == 2);
    CHECK(g_blocks.size() == 9);
  }
  CHECK(g_blocks.empty() && g_handles.empty());
}

int main() {
  test_ensure();
  CHECK(g_blocks.empty() && g_handles.empty());
  test_buf_moves();
  CHECK(g_blocks.empty() && g_handles.empty());
  test_handles();
  CHECK(g_blocks.empty() && g_handles.empty());
  test_aggregate();
  std::printf("dev_owned: %d failed checks, %zu live blocks, %zu live handles\n", g_failed, g_blocks.size(), g_handles.size());
  return g_failed == 0 && g_blocks.empty() && g_handles.empty() ? 0 : 1;
}
