// query_stage.h — where the outputs of a host-pointer query go in the context's staging buffer (sptr_api.cpp:
// stage_query).  Plain C++, no HIP: tests/cpp/test_query_stage.cpp runs it under sanitizers.
#pragma once
#include <cstddef>

namespace sptr {

// offset[i] for a field of bytes[i], i < k, in the given order; returns the bytes the buffer needs.  Every offset
// is a multiple of 16 (hipMalloc's blocks are aligned far beyond that), so each field may be written by 16-byte
// stores whatever the sizes before it; no two fields overlap.  The largest table, 68 bytes for each of 2^28
// points and ten fields, needs 2^34 + 2^30 + at most 160 bytes: far inside size_t.
inline size_t stage_layout(const size_t* bytes, int k, size_t* offset) {
  size_t at = 0;
  for (int i = 0; i < k; ++i) {
    offset[i] = at;
    at += (bytes[i] + 15u) & ~(size_t)15u;
  }
  return at;
}

}  // namespace sptr
