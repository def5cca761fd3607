// xform_point.h — a point through a glm-layout mat4, for the host layer's flattening
// (scene::transform_point, host/scene_desc.cpp) and for the refit's transform pass (k_refit_slots<true>,
// kernels_refit.hip): one function, so that a vertex the device moves has the bits of the vertex the host
// would have uploaded.  glm's mat4 * vec4(p, 1): per output component k the four products, summed as
// (m0 + m1) + (m2 + m3); float32, no contraction (-ffp-contract=off on both sides).
#pragma once
#include "sptr_math.h"

namespace sptr {

// m: 16 floats, column-major (m[4 * col + row], as float[4][4] m[col][row] lies in memory).  Row 3 is not read.
SPTR_HD vec3 xform_point(const float* m, vec3 p) {
  float o[3];
  for (int k = 0; k < 3; ++k) {
    const float m0 = m[k] * p.x, m1 = m[4 + k] * p.y, m2 = m[8 + k] * p.z, m3 = m[12 + k] * 1.0f;
    o[k] = (m0 + m1) + (m2 + m3);
  }
  return vec3{o[0], o[1], o[2]};
}

}  // namespace sptr
