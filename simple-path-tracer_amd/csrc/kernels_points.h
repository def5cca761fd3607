// kernels_points.h — closest-point queries on caller buffers (sptr_query_points): the walk kernel k_pointquery and
// the sort-key kernel k_point_keys.  Included by kernels_wavefront.hip inside namespace sptr after kernels_query.h,
// whose staging, grid-stride loop, gather / scatter by `order`, id resolution (HitKey) and key cells it shares.
//
// The definition is csrc/closest_point.h: a candidate per primitive, the result the candidate with the smallest key
// (d2, geomID, primID) within the point's radius.  The walk skips a subtree only when cp_node_bound of its box is
// strictly greater than the best d2 so far (initially max_dist^2), and a candidate replaces the best iff its key
// is smaller, so the result is a function of the scene and the point: not of the tree or the order of the visits.
// The walk carries (d2, primitive reference); the ids are resolved only on an exact tie in d2, and the candidate's
// point, weights and normal are computed again, by the same function, once after the walk.
//
// Stack: an entry is a node and its bound, two LDS words in two columns per thread (the ray walks' column and a
// second one of the same shape), entries beyond the LDS depth in two private arrays.  The bound is kept because a
// popped entry is dropped when the best d2 has fallen below it meanwhile, which a ray walk cannot do either
// without the box; recomputing would need the parent node again.  Cost: 12 KiB more static LDS per block.
//
// Memory traffic per point: 16 B in; out 4 geom + 4 prim + 4 dist2 + 4 dist + 12 point + 8 uv + 12 Ng = 48 B.

struct PointBest {
  float d2;      // the best key's d2; max_dist^2 while ref == kNoHit
  uint32_t ref;  // primitive reference, kNoHit: none yet
};

template <int N>
struct PointStack {
  uint32_t *node, *bound;  // &s_stack.e[0][threadIdx.x], &s_bound.e[0][threadIdx.x]
  uint32_t spill_node[kStack - N];
  float spill_bound[kStack - N];
  __device__ __forceinline__ void put(int i, uint32_t n, float b) {
    if (i < N) {
      node[i * kBlock] = n;
      bound[i * kBlock] = __float_as_uint(b);
    } else {
      spill_node[i - N] = n;
      spill_bound[i - N] = b;
    }
  }
  __device__ __forceinline__ uint32_t get_node(int i) const { return i < N ? node[i * kBlock] : spill_node[i - N]; }
  __device__ __forceinline__ float get_bound(int i) const { return i < N ? __uint_as_float(bound[i * kBlock]) : spill_bound[i - N]; }
};

// leaf_test's loop over a leaf's primitives: each one's candidate d2 against the best key
template <bool kCount, bool kDirect>
__device__ __forceinline__ void leaf_points(uint32_t link, const uint32_t* prim_ref, const float4* tris, const float4* sph,
                                            const vec3& p, const HitKey& key, PointBest& best, Visits& vc) {
  const bool direct = kDirect && (link & kLeafDirect) != 0u;
  const uint32_t start = (link & ~kLeafBit) >> kLeafCountBits, cnt = direct ? 1u : (link & kLeafRangeMask) + 1u;
  for (uint32_t j = 0; j < cnt; ++j) {
    const uint32_t pr = direct ? (start | ((link & kLeafDirectSphere) ? kSphereBit : 0u)) : prim_ref[start + j];
    const uint32_t idx = pr & kIndexMask;
    float d2;
    if (pr & kSphereBit) {
      if (kCount) ++vc.sph;
      const float4 s = sph[idx];
      d2 = cp_sphere_d2(v3(s.x, s.y, s.z), s.w, p);
    } else {
      if (kCount) ++vc.tris;
      const float4 ta = tris[3 * idx + 0], tb = tris[3 * idx + 1], tc = tris[3 * idx + 2];
      if (!cp_triangle_live(v3(tc.y, tc.z, tc.w))) continue;
      d2 = cp_triangle(v3(ta.x, ta.y, ta.z), v3(ta.w, tb.x, tb.y), v3(tb.z, tb.w, tc.x), p).d2;
    }
    bool take = d2 < best.d2;
    if (!take && d2 == best.d2 && pr != best.ref)  // an exact tie: by the ids (no primitive yet: any id wins)
      take = best.ref == kNoHit || key(pr) < key(best.ref);
    if (take) {
      best.d2 = d2;
      best.ref = pr;
    }
  }
}

template <bool kCount, int N>
__device__ __forceinline__ void bvh2_walk_points(uint32_t root, PointStack<N>& stack, const BvhNode* nodes,
                                                 const uint32_t* prim_ref, const float4* tris, const float4* sph,
                                                 const vec3& p, float M, const HitKey& key, PointBest& best, Visits& vc) {
  uint32_t cur = root;
  int sp = 0;
  for (;;) {
    const BvhNode* nd = nodes + cur;
    const float4 lxy = nd->lxy, rxy = nd->rxy, z = nd->z;
    const uint4 ln = nd->link;
    if (kCount) ++vc.nodes;
    float bl = cp_node_bound(p, v3(lxy.x, lxy.z, z.x), v3(lxy.y, lxy.w, z.y), M);
    float br = cp_node_bound(p, v3(rxy.x, rxy.z, z.z), v3(rxy.y, rxy.w, z.w), M);
    uint32_t L = ln.x, R = ln.y;
    if (br < bl) {  // L: the child with the smaller bound
      const uint32_t s = L;
      L = R;
      R = s;
      const float b = bl;
      bl = br;
      br = b;
    }
    bool hl = !(bl > best.d2);
    if (hl && (L & kLeafBit)) {
      leaf_points<kCount, false>(L, prim_ref, tris, sph, p, key, best, vc);
      hl = false;
    }
    bool hr = !(br > best.d2);
    if (hr && (R & kLeafBit)) {
      leaf_points<kCount, false>(R, prim_ref, tris, sph, p, key, best, vc);
      hr = false;
    }
    hl = hl && !(bl > best.d2);
    if (hl && hr) {
      if (sp < kStack) stack.put(sp++, R, br);
      else vc.stack_overflow = 1u;
      cur = L;
    } else if (hl) {
      cur = L;
    } else if (hr) {
      cur = R;
    } else {
      for (;;) {
        if (sp == 0) return;
        --sp;
        if (!(stack.get_bound(sp) > best.d2)) break;
      }
      cur = stack.get_node(sp);
    }
  }
}

// every node from `nodes` (staged, or L2/HBM); the child planes decoded in float32 (cp_wide_plane)
template <bool kCount, int N>
__device__ __forceinline__ void wide_walk_points(uint32_t root, PointStack<N>& stack, const WideNode* nodes,
                                                 const uint32_t* prim_ref, const float4* tris, const float4* sph,
                                                 const vec3& p, float M, const HitKey& key, PointBest& best, Visits& vc) {
  uint32_t cur = root;
  int sp = 0;
  for (;;) {
    const uint4* nq = reinterpret_cast<const uint4*>(nodes + cur);
    const uint4 h = nq[0], l4 = nq[1], q4 = nq[2];
    const uint2 q2 = *reinterpret_cast<const uint2*>(nq + 3);
    const uint32_t ln[4] = {l4.x, l4.y, l4.z, l4.w};
    if (kCount) ++vc.nodes;
    const float ox = __uint_as_float(h.x), oy = __uint_as_float(h.y), oz = __uint_as_float(h.z);
    const uint32_t ex = h.w & 0xFFu, ey = (h.w >> 8) & 0xFFu, ez = (h.w >> 16) & 0xFFu;
    float b[kWide];
    bool hc[kWide];
#pragma unroll
    for (int k = 0; k < kWide; ++k) {
      const uint32_t sh = 8u * (uint32_t)k;
      const vec3 lo = v3(cp_wide_plane(ox, ex, (q4.x >> sh) & 0xFFu), cp_wide_plane(oy, ey, (q4.z >> sh) & 0xFFu),
                         cp_wide_plane(oz, ez, (q2.x >> sh) & 0xFFu));
      const vec3 hi = v3(cp_wide_plane(ox, ex, (q4.y >> sh) & 0xFFu), cp_wide_plane(oy, ey, (q4.w >> sh) & 0xFFu),
                         cp_wide_plane(oz, ez, (q2.y >> sh) & 0xFFu));
      b[k] = cp_node_bound(p, lo, hi, M);
      hc[k] = ln[k] != kNoHit;
    }
#pragma unroll
    for (int k = 0; k < kWide; ++k) {
      if (hc[k] && (ln[k] & kLeafBit)) {
        if (!(b[k] > best.d2)) leaf_points<kCount, true>(ln[k], prim_ref, tris, sph, p, key, best, vc);
        hc[k] = false;
      }
    }
    int kn = kWide;
    float bn = __builtin_huge_valf();
    uint32_t npush = 0u;
#pragma unroll
    for (int k = 0; k < kWide; ++k) {
      hc[k] = hc[k] && !(b[k] > best.d2);
      if (hc[k] && (kn == kWide || b[k] < bn)) {
        bn = b[k];
        kn = k;
      }
      npush += hc[k] ? 1u : 0u;
    }
    if (kn < kWide) {
      if (sp + (int)npush - 1 > kStack) vc.stack_overflow = 1u;
#pragma unroll
      for (int k = kWide - 1; k >= 0; --k)
        if (hc[k] && k != kn && sp < kStack) stack.put(sp++, ln[k], b[k]);
      cur = ln[kn];
    } else {
      for (;;) {
        if (sp == 0) return;
        --sp;
        if (!(stack.get_bound(sp) > best.d2)) break;
      }
      cur = stack.get_node(sp);
    }
  }
}

// --------------------------------------------------------------------------------- k_pointquery
// Thread j of a resident grid answers point order[j] (kIndexed) or j, grid-striding, and writes every output at the
// point's own index.  kCount (SPTR_POINT_COUNT): node visits and primitive tests are summed per wave and added to
// q.counters[0] and [1] with one atomic each per wave; without it the counting is compiled out.
template <bool kLds, bool kW4, bool kIndexed, bool kCount>
__global__ void __launch_bounds__(kBlock) k_pointquery(SceneView sv, PointQueryView q) {
  __shared__ KernelStack<kLds> s_stack;
  __shared__ KernelStack<kLds> s_bound;
  extern __shared__ float4 lds[];
  const Staged sc = stage_scene<kLds>(sv, lds);
  __syncthreads();
  Visits vc;
  const HitKey key{sv.tri_geom, sv.sph_geom, q.tri_orig, q.geom_first};
  const uint32_t root = kW4 ? sv.root4 : sv.root;
  // the scene's largest absolute coordinate, from the root box: both child boxes of the BVH2 root (kept and refitted
  // for wide scenes too, as k_ray_keys reads them); a root that is a leaf is tested without a bound
  float mroot = 0.0f;
  if (root != kNoHit && !(root & kLeafBit) && sv.num_nodes != 0u && !(sv.root & kLeafBit)) {
    const BvhNode nd = sv.nodes[sv.root];
    const float f[12] = {nd.lxy.x, nd.lxy.y, nd.lxy.z, nd.lxy.w, nd.rxy.x, nd.rxy.y, nd.rxy.z, nd.rxy.w, nd.z.x, nd.z.y, nd.z.z, nd.z.w};
#pragma unroll
    for (int k = 0; k < 12; ++k) mroot = fmax_g(mroot, fabsf(f[k]));
  }
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < q.n; j += grid_threads()) {
    const uint32_t i = kIndexed ? q.order[j] : j;
    const float4 a = q.points[i];  // p.xyz, max_dist
    const vec3 p = v3(a.x, a.y, a.z);
    PointBest best{a.w * a.w, kNoHit};
    if (cp_point_valid(p, a.w) && root != kNoHit) {
      if (root & kLeafBit) {
        leaf_points<kCount, false>(root, sc.prim_ref, sc.tris, sc.sph, p, key, best, vc);
      } else {
        const float M = fmax_g(cp_abs_max(p), mroot);
        PointStack<kLds ? kLdsStack : kLdsStackG> stack;
        stack.node = &s_stack.e[0][threadIdx.x];
        stack.bound = &s_bound.e[0][threadIdx.x];
        if constexpr (kW4) wide_walk_points<kCount>(root, stack, sc.nodes4, sc.prim_ref, sc.tris, sc.sph, p, M, key, best, vc);
        else bvh2_walk_points<kCount>(root, stack, sc.nodes, sc.prim_ref, sc.tris, sc.sph, p, M, key, best, vc);
      }
    }
    // the record of the primitive finally chosen, once per point and outside the walk
    uint2 id = make_uint2(kNoHit, kNoHit);
    vec3 ng = v3(0.0f, 0.0f, 0.0f), pt = v3(0.0f, 0.0f, 0.0f);
    float u = 0.0f, v = 0.0f, d2 = __builtin_huge_valf();
    if (best.ref != kNoHit) {
      const uint32_t idx = best.ref & kIndexMask;
      d2 = best.d2;
      if (q.geom || q.prim) id = key.ids(best.ref);
      if (best.ref & kSphereBit) {
        const float4 s = sc.sph[idx];
        const CpCand c = cp_sphere(v3(s.x, s.y, s.z), s.w, p, ng);
        pt = c.q;
      } else {
        const float4 ta = sc.tris[3 * idx + 0], tb = sc.tris[3 * idx + 1], tc = sc.tris[3 * idx + 2];
        const CpCand c = cp_triangle(v3(ta.x, ta.y, ta.z), v3(ta.w, tb.x, tb.y), v3(tb.z, tb.w, tc.x), p);
        pt = c.q;
        u = c.u;
        v = c.v;
        ng = v3(tc.y, tc.z, tc.w);
      }
    }
    if (q.geom) q.geom[i] = id.x;
    if (q.prim) q.prim[i] = id.y;
    if (q.dist2) q.dist2[i] = d2;
    if (q.dist) q.dist[i] = sq_root(d2);
    if (q.point) {
      float* o3 = q.point + (size_t)i * 3;
      o3[0] = pt.x;
      o3[1] = pt.y;
      o3[2] = pt.z;
    }
    if (q.uv) {
      q.uv[(size_t)i * 2 + 0] = u;
      q.uv[(size_t)i * 2 + 1] = v;
    }
    if (q.ng) {
      float* n3 = q.ng + (size_t)i * 3;
      n3[0] = ng.x;
      n3[1] = ng.y;
      n3[2] = ng.z;
    }
  }
  if (__ballot(vc.stack_overflow != 0u) && lane_id() == 0u) *q.stack_overflow = 1u;
  if constexpr (kCount) {
    unsigned long long nv = vc.nodes, nt = (unsigned long long)vc.tris + vc.sph;
    for (int off = 32; off > 0; off >>= 1) {
      nv += __shfl_xor(nv, off);
      nt += __shfl_xor(nt, off);
    }
    if (lane_id() == 0u) {
      atomicAdd(&q.counters[0], nv);
      atomicAdd(&q.counters[1], nt);
    }
  }
}

void launch_pointquery(const SceneView& sv, const PointQueryView& q, hipStream_t s, uint32_t* lds_bytes) {
  if (q.n == 0u) return;
  const bool L = sv.lds_bytes != 0;
  const unsigned lb = L ? sv.lds_bytes : 16u;
  const unsigned need = (unsigned)(((uint64_t)q.n + kBlock - 1) / kBlock);
  dispatch(
      [&](auto fl) -> unsigned {
        return [&]<bool Lc, bool Wc, bool Ic, bool Cc>(Flags<Lc, Wc, Ic, Cc>) {
          const unsigned g = std::max(1u, std::min<unsigned>(resident_grid((const void*)&k_pointquery<Lc, Wc, Ic, Cc>, lb), need));
          hipLaunchKernelGGL((k_pointquery<Lc, Wc, Ic, Cc>), dim3(g), dim3(kBlock), lb, s, sv, q);
          *lds_bytes = (uint32_t)(2u * sizeof(KernelStack<Lc>)) + lb;
          return g;
        }(fl);
      },
      Flags<>{}, L, sv.width == (uint32_t)kWide, q.order != nullptr, q.counters != nullptr);
}

// --------------------------------------------------------------------------------- k_point_keys
// Sort key of a point: k_ray_keys' origin part, the 30-bit Morton code of p over the doubled root box.
__device__ __forceinline__ void key_root_box(const SceneView& sv, vec3& lo, vec3& ext) {
  lo = v3(0.0f, 0.0f, 0.0f);
  ext = v3(0.0f, 0.0f, 0.0f);
  if (sv.num_nodes != 0u && !(sv.root & kLeafBit)) {
    const BvhNode nd = sv.nodes[sv.root];
    const vec3 l = v3(fminf(nd.lxy.x, nd.rxy.x), fminf(nd.lxy.z, nd.rxy.z), fminf(nd.z.x, nd.z.z));
    const vec3 h = v3(fmaxf(nd.lxy.y, nd.rxy.y), fmaxf(nd.lxy.w, nd.rxy.w), fmaxf(nd.z.y, nd.z.w));
    ext = v3((h.x - l.x) * 2.0f, (h.y - l.y) * 2.0f, (h.z - l.z) * 2.0f);
    lo = v3(l.x - (h.x - l.x) * 0.5f, l.y - (h.y - l.y) * 0.5f, l.z - (h.z - l.z) * 0.5f);
  }
}
__device__ __forceinline__ uint32_t key_morton30(float x, float y, float z, const vec3& lo, const vec3& ext) {
  return spread3_10(key_cell(x, lo.x, ext.x, 1024u)) | (spread3_10(key_cell(y, lo.y, ext.y, 1024u)) << 1) |
         (spread3_10(key_cell(z, lo.z, ext.z, 1024u)) << 2);
}

__global__ void __launch_bounds__(kBlock) k_point_keys(SceneView sv, const float4* points, uint32_t n, uint64_t* keys,
                                                       uint32_t* index) {
  vec3 lo, ext;
  key_root_box(sv, lo, ext);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += grid_threads()) {
    const float4 a = points[i];
    keys[i] = (uint64_t)key_morton30(a.x, a.y, a.z, lo, ext);
    index[i] = i;
  }
}

void launch_point_keys(const SceneView& sv, const float4* points, uint32_t n, uint64_t* keys, uint32_t* index, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_point_keys, dim3(grid_for(n)), dim3(kBlock), 0, s, sv, points, n, keys, index);
}
