// lbvh_shared.h — device functions the LBVH build (kernels_lbvh.hip) and the in-place refit
// (kernels_refit.hip) both call, so that the same coordinates give the same bits in either:
// the triangle record and primitive boxes of a slot, and the wide node's child list and quantisation.
#pragma once
#include <hip/hip_runtime.h>

#include "sptr_internal.h"

namespace sptr {

// Embree's precomputed geometric normal Ng = cross(e2, e1) (msub form)
__device__ __forceinline__ vec3 tri_ng3(const vec3& v0, const vec3& v1, const vec3& v2) {
  const vec3 e1 = v0 - v1, e2 = v2 - v0;
  return v3(__builtin_fmaf(e2.y, e1.z, -(e2.z * e1.y)), __builtin_fmaf(e2.z, e1.x, -(e2.x * e1.z)),
            __builtin_fmaf(e2.x, e1.y, -(e2.y * e1.x)));
}
// the three float4 of a triangle slot: v0.xyz e1.x | e1.yz e2.xy | e2.z Ng.xyz (as Embree's TriangleM)
__device__ __forceinline__ void tri_record(const vec3& v0, const vec3& v1, const vec3& v2, float4* rec) {
  const vec3 e1 = v0 - v1, e2 = v2 - v0;
  const vec3 ng = tri_ng3(v0, v1, v2);
  rec[0] = make_float4(v0.x, v0.y, v0.z, e1.x);
  rec[1] = make_float4(e1.y, e1.z, e2.x, e2.y);
  rec[2] = make_float4(e2.z, ng.x, ng.y, ng.z);
}
__device__ __forceinline__ void tri_box(const vec3& p0, const vec3& p1, const vec3& p2, vec3& lo, vec3& hi) {
  lo = v3(fminf(p0.x, fminf(p1.x, p2.x)), fminf(p0.y, fminf(p1.y, p2.y)), fminf(p0.z, fminf(p1.z, p2.z)));
  hi = v3(fmaxf(p0.x, fmaxf(p1.x, p2.x)), fmaxf(p0.y, fmaxf(p1.y, p2.y)), fmaxf(p0.z, fmaxf(p1.z, p2.z)));
}
__device__ __forceinline__ void sphere_box(const float4& s, vec3& lo, vec3& hi) {
  lo = v3(s.x - s.w, s.y - s.w, s.z - s.w);
  hi = v3(s.x + s.w, s.y + s.w, s.z + s.w);
}

struct WideBoxes {
  float lo[3][kWide], hi[3][kWide];
  uint32_t link[kWide];
};

// Quantise the n child boxes of one wide node (WideNode): per axis, org = the smallest lower
// plane, step 2^e the smallest power of two (e in [-100, 60]) with extent <= 255 * 2^e, qlo =
// floor((lo - org) / 2^e) and qhi = ceil((hi - org) / 2^e) evaluated in double (exact for the
// scene's float coordinates), so the decoded box always contains the child box.
// An axis of zero extent has every plane at org (q = 0) whatever its step; it takes the largest step
// of the node's other axes (or, with all three flat, 2^-16 of the largest |org|), because q_axis pads
// a decoded plane by 2^-20 * 256 * 2^e / |d|: with the step 2^-100 that pad was too small to accept a ray
// parallel to the axis whose origin lies in the node's plane (zero-radius spheres on a line, hit by the
// ray through them); with the node's own scale it exceeds every distance for such a ray and stays
// 2^-12 of a step of the other axes for all others.
__device__ __forceinline__ WideNode quantize_wide(const WideBoxes& b, int n, uint32_t parent) {
  WideNode o;
  float org[3];
  int es[3];
  bool flat[3];
  uint32_t ex = (uint32_t)n << 24;
  for (int w = 0; w < 6; ++w)
    for (int j = 0; j < kQWords; ++j) o.q[w][j] = 0u;
  int emax = -101;
  for (int a = 0; a < 3; ++a) {
    float mn = b.lo[a][0], mx = b.hi[a][0];
    for (int k = 1; k < n; ++k) {
      mn = fminf(mn, b.lo[a][k]);
      mx = fmaxf(mx, b.hi[a][k]);
    }
    org[a] = mn;
    const double ext = (double)mx - (double)mn;
    int e = -100;
    flat[a] = !(ext > 0.0);
    if (ext > 0.0) {
      int x;
      (void)frexp(ext / 255.0, &x);  // ext / 255 in (2^(x-1), 2^x]
      e = x;
      if (ext <= 255.0 * ldexp(1.0, e - 1)) --e;
      e = e < -100 ? -100 : (e > 60 ? 60 : e);
      emax = e > emax ? e : emax;
    }
    es[a] = e;
  }
  if (emax < -100) {  // a point: the scale of its coordinates
    const float m = fmaxf(fmaxf(fabsf(org[0]), fabsf(org[1])), fabsf(org[2]));
    int x = -84;
    if (m > 0.0f) (void)frexp((double)m, &x);
    emax = x - 16;
    emax = emax < -100 ? -100 : (emax > 60 ? 60 : emax);
  }
  for (int a = 0; a < 3; ++a) {
    const float mn = org[a];
    const int e = flat[a] ? emax : es[a];
    ex |= (uint32_t)(e + 127) << (8 * a);
    const double inv_step = ldexp(1.0, -e);
    for (int k = 0; k < n; ++k) {
      double l = floor(((double)b.lo[a][k] - (double)mn) * inv_step), h = ceil(((double)b.hi[a][k] - (double)mn) * inv_step);
      l = l < 0.0 ? 0.0 : (l > 255.0 ? 255.0 : l);
      h = h < 0.0 ? 0.0 : (h > 255.0 ? 255.0 : h);
      o.q[2 * a][k / 4] |= (uint32_t)l << (8 * (k % 4));
      o.q[2 * a + 1][k / 4] |= (uint32_t)h << (8 * (k % 4));
    }
  }
  o.ox = org[0];
  o.oy = org[1];
  o.oz = org[2];
  o.ex = ex;
  for (int k = 0; k < kWide; ++k) o.link[k] = b.link[k];
  o.parent = parent;
  for (uint32_t& x : o.pad) x = 0u;
  return o;
}

// Greedy surface-area collapse, top-down one wide level per launch pair: a wide
// node's child list starts as its BVH2 node's two children and grows, up to kWide entries, by
// opening the internal entry whose box has the largest surface area (lowest slot on ties) — it is
// replaced in place by its left and right children, so the list stays in left-to-right order.
// Unlike a fixed two-level collapse this fills nodes whose grandchildren include leaves and spends
// the wide levels where the big boxes are, so deep LBVH chains give shallower wide trees.
// Its internal entries become the next level's wide nodes.
__device__ __forceinline__ float box_area(const WideBoxes& b, int e) {
  const float dx = b.hi[0][e] - b.lo[0][e], dy = b.hi[1][e] - b.lo[1][e], dz = b.hi[2][e] - b.lo[2][e];
  return dx * dy + dy * dz + dz * dx;
}
__device__ __forceinline__ void put_child(WideBoxes& b, int e, const BvhNode& nd, bool right) {
  if (!right) {
    b.link[e] = nd.link.x;
    b.lo[0][e] = nd.lxy.x; b.hi[0][e] = nd.lxy.y; b.lo[1][e] = nd.lxy.z; b.hi[1][e] = nd.lxy.w;
    b.lo[2][e] = nd.z.x;   b.hi[2][e] = nd.z.y;
  } else {
    b.link[e] = nd.link.y;
    b.lo[0][e] = nd.rxy.x; b.hi[0][e] = nd.rxy.y; b.lo[1][e] = nd.rxy.z; b.hi[1][e] = nd.rxy.w;
    b.lo[2][e] = nd.z.z;   b.hi[2][e] = nd.z.w;
  }
}
// kTrack: src[e] = (BVH2 node << 1) | side that entry e's box and link were read from (the table a
// refit re-emits the wide node from); otherwise src is not touched
template <bool kTrack>
__device__ int expand_greedy_t(const BvhNode* nodes, uint32_t node, WideBoxes& b, uint32_t* src) {
  for (int k = 0; k < kWide; ++k) {
    b.link[k] = kNoHit;
    for (int a = 0; a < 3; ++a) b.lo[a][k] = b.hi[a][k] = 0.0f;
    if (kTrack) src[k] = kNoHit;
  }
  const BvhNode nd = nodes[node];
  put_child(b, 0, nd, false);
  put_child(b, 1, nd, true);
  if (kTrack) {
    src[0] = node << 1;
    src[1] = (node << 1) | 1u;
  }
  int n = 2;
  while (n < kWide) {
    int best = -1;
    float ba = -1.0f;
    for (int e = 0; e < n; ++e)
      if (!(b.link[e] & kLeafBit)) {
        const float a = box_area(b, e);
        if (a > ba) {
          ba = a;
          best = e;
        }
      }
    if (best < 0) break;
    const uint32_t open = b.link[best];
    const BvhNode cn = nodes[open];
    for (int e = n; e > best + 1; --e) {
      b.link[e] = b.link[e - 1];
      if (kTrack) src[e] = src[e - 1];
      for (int a = 0; a < 3; ++a) {
        b.lo[a][e] = b.lo[a][e - 1];
        b.hi[a][e] = b.hi[a][e - 1];
      }
    }
    put_child(b, best, cn, false);
    put_child(b, best + 1, cn, true);
    if (kTrack) {
      src[best] = open << 1;
      src[best + 1] = (open << 1) | 1u;
    }
    ++n;
  }
  return n;
}
__device__ __forceinline__ int expand_greedy(const BvhNode* nodes, uint32_t node, WideBoxes& b) {
  return expand_greedy_t<false>(nodes, node, b, nullptr);
}

}  // namespace sptr
