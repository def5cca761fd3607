// dev_owned.h — owners of the device resources the library holds: memory blocks, events, streams,
// graphs.  Each frees what it holds when it goes out of scope and can be moved but not copied, so a
// struct of them (Context, sptr_ctx) needs no cleanup list and cannot alias device memory by accident.
// Host-only: the HIP runtime API and the standard library, nothing else.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cassert>
#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

namespace sptr {

// A device memory block.  p and bytes are read directly (static_cast<T*>(b.p)); only ensure(),
// release(), a move and the destructor change them.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;

  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      bytes = std::exchange(o.bytes, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }

  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // Grow or keep: a block of at least n bytes (0 counts as 16).  A block that is large enough stays;
  // otherwise the old one is freed first (its contents are not carried over) and bytes becomes the
  // size allocated.  On failure the buffer is empty.
  hipError_t ensure(size_t n) {
    if (n == 0) n = 16;
    if (bytes >= n) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    else p = nullptr;
    return e;
  }
};
static_assert(!std::is_copy_constructible_v<DevBuf> && !std::is_copy_assignable_v<DevBuf>, "a copy would alias device memory");

// An event, stream, graph or executable graph.  Creation stays with the caller (flags and priorities
// differ per site): pass put() to the runtime's create / capture / instantiate call.
template <class H, hipError_t (*Destroy)(H)>
struct DevHandle {
  H h = nullptr;

  DevHandle() = default;
  DevHandle(DevHandle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  DevHandle& operator=(DevHandle&& o) noexcept {
    if (this != &o) {
      reset();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~DevHandle() { reset(); }

  operator H() const { return h; }
  H* put() {  // where the runtime stores a new handle: only into an empty owner
    assert(!h);
    return &h;
  }
  void reset() {
    if (h) (void)Destroy(h);
    h = nullptr;
  }
};
using DevEvent = DevHandle<hipEvent_t, hipEventDestroy>;
using DevStream = DevHandle<hipStream_t, hipStreamDestroy>;
using DevGraph = DevHandle<hipGraph_t, hipGraphDestroy>;
using DevGraphExec = DevHandle<hipGraphExec_t, hipGraphExecDestroy>;
static_assert(!std::is_copy_constructible_v<DevEvent>, "a copy would destroy the handle twice");

// The typed scratch arrays of one call (build_lbvh): alloc() hands out n elements of T, and all of
// them are freed when this goes out of scope.
struct DevTemps {
  std::vector<DevBuf> bufs;
  template <class T>
  hipError_t alloc(T** p, size_t n) {
    DevBuf b;
    const hipError_t e = b.ensure(n * sizeof(T));
    *p = static_cast<T*>(b.p);
    if (e == hipSuccess) bufs.push_back(std::move(b));
    return e;
  }
};

}  // namespace sptr
