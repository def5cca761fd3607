// kernels_query.h — batched ray queries on caller buffers (sptr_query_rays, sptr_query_multi_hit): the trace
// kernels k_rayquery and k_rayquery_multi and the sort-key kernel k_ray_keys.  Included by
// kernels_wavefront.hip inside namespace sptr, after its traversal helpers and launch utilities, which these kernels share: k_rayquery walks the BVH through
// traverse_w exactly as the render kernels and k_aov do (LDS-staged scenes are staged, wide scenes take the
// BVH4 walk), so a ray's hit is the renderer's hit.
//
// Memory traffic per ray: 32 B in (two 16-B loads); out 4 geom + 4 prim + 4 t + 12 Ng + 8 uv = 32 B for a
// closest hit (less for NULL outputs), 1 B for any-hit; a sorted query adds 8 B of key and 4 B of index,
// written by k_ray_keys and then moved by the radix sort's eight passes (kernels_sort.hip).

// --------------------------------------------------------------------------------- k_rayquery
// Thread j of a resident grid traces ray order[j] (kIndexed) or ray j, grid-striding over the batch, and
// writes every output at the ray's own index: a sorted batch is gathered in and scattered out, no ray is
// copied.  order is the value array of a sort of the identity indices 0..n-1, a permutation of them.
template <bool kLds, bool kW4, bool kAny, bool kIndexed>
__global__ void __launch_bounds__(kBlock) k_rayquery(SceneView sv, RayQueryView q) {
  __shared__ KernelStack<kLds> s_stack;
  extern __shared__ float4 lds[];
  const Staged sc = stage_scene<kLds>(sv, lds);
  __syncthreads();
  Visits vc;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < q.n; j += grid_threads()) {
    const uint32_t i = kIndexed ? q.order[j] : j;
    const float4 a = q.rays[2 * (size_t)i], b = q.rays[2 * (size_t)i + 1];  // o.xyz d.x | d.yz tnear tfar
    const vec3 o = v3(a.x, a.y, a.z), d = v3(a.w, b.x, b.y);
    const Ray r = make_ray(o, d);
    float tfar = b.w;
    uint32_t ref = kNoHit;
    const bool hit = traverse_w<kW4, kAny, false>(sc, sv, r, b.z, tfar, ref, vc, s_stack);
    if constexpr (kAny) {
      q.occ[i] = hit ? 1 : 0;
    } else {
      // the record of the primitive finally hit, once per ray and outside the walk
      uint2 id = make_uint2(kNoHit, kNoHit);
      vec3 ng = v3(0.0f, 0.0f, 0.0f);
      float u = 0.0f, v = 0.0f;
      if (hit) {
        const uint32_t idx = ref & kIndexMask;
        if (ref & kSphereBit) {  // as k_query: the reference's sphere callbacks set Ng, no u or v
          const float4 s = sc.sph[idx];
          const vec3 P = o + tfar * d;
          ng = v3((P.x - s.x) / s.w, (P.y - s.y) / s.w, (P.z - s.z) / s.w);
          id = make_uint2(sv.sph_geom[idx], 0u);
        } else {
          const float4 ta = sc.tris[3 * idx + 0], tb = sc.tris[3 * idx + 1], tc = sc.tris[3 * idx + 2];
          ng = v3(tc.y, tc.z, tc.w);
          if (q.geom || q.prim) {
            const uint32_t g = sv.tri_geom[idx];
            id = make_uint2(g, q.tri_orig[idx] - q.geom_first[g]);
          }
          if (q.uv) {  // tri_hit4's U, V and den for this triangle; u = U / |den|, v = V / |den|
            const vec3 v0 = v3(ta.x, ta.y, ta.z), e1 = v3(ta.w, tb.x, tb.y), e2 = v3(tb.z, tb.w, tc.x);
            const vec3 R = e_cross(v0 - o, d);
            const float den = e_dot(ng, d);
            const float aden = fabsf(den);
            u = xorsign(e_dot(R, e2), den) / aden;
            v = xorsign(e_dot(R, e1), den) / aden;
          }
        }
      }
      if (q.geom) q.geom[i] = id.x;
      if (q.prim) q.prim[i] = id.y;
      if (q.t) q.t[i] = hit ? tfar : __builtin_huge_valf();
      if (q.ng) {
        float* n3 = q.ng + (size_t)i * 3;
        n3[0] = ng.x;
        n3[1] = ng.y;
        n3[2] = ng.z;
      }
      if (q.uv) {  // (scalar stores: only the ray buffer has an alignment rule)
        q.uv[(size_t)i * 2 + 0] = u;
        q.uv[(size_t)i * 2 + 1] = v;
      }
    }
  }
  if (__ballot(vc.stack_overflow != 0u) && lane_id() == 0u) *q.stack_overflow = 1u;
}

void launch_rayquery(const SceneView& sv, const RayQueryView& q, bool anyhit, hipStream_t s) {
  if (q.n == 0u) return;
  const bool L = sv.lds_bytes != 0;
  const unsigned lb = L ? sv.lds_bytes : 16u;
  const unsigned need = (unsigned)(((uint64_t)q.n + kBlock - 1) / kBlock);
  dispatch(
      [&](auto fl) -> unsigned {
        return [&]<bool Lc, bool Wc, bool Ac, bool Ic>(Flags<Lc, Wc, Ac, Ic>) {
          const unsigned g = std::max(1u, std::min<unsigned>(resident_grid((const void*)&k_rayquery<Lc, Wc, Ac, Ic>, lb), need));
          hipLaunchKernelGGL((k_rayquery<Lc, Wc, Ac, Ic>), dim3(g), dim3(kBlock), lb, s, sv, q);
          return g;
        }(fl);
      },
      Flags<>{}, L, sv.width == (uint32_t)kWide, anyhit, q.order != nullptr);
}

// --------------------------------------------------------------------------------- k_rayquery_multi
// sptr_query_multi_hit: per ray the K nearest candidate hits in ascending (t, geomID, primID) (include/sptr_hip.h
// states the contract).  The staging, the grid-stride loop and the gather / scatter by `order` are k_rayquery's;
// the walks below are its walks (bvh2_walk, wide_walk_inl) with a leaf routine that inserts into a list instead
// of shrinking tfar.  They are functions of their own, so that the render kernels' traversal code does not move.
//
// The list (hit_list.h) lives in LDS, one column per thread and entry-major like the traversal stack: entry e of
// thread x is words s_list.e[2e][x] (t) and s_list.e[2e + 1][x] (ref), so a wave's accesses at one position fall
// in 64 distinct banks and a run-time position is an address, not a register index (no scratch).  2 KiB per entry
// of capacity per block; kCap is the smallest instantiated capacity (4, 8, 16) that holds K.
//
// Pruning: primitives are always tested against the ray's own (tnear, tfar); only the boxes are pruned, by tfar
// while the list holds fewer than K entries and by the K-th t once it is full (hit_list_bound).  The slab tests
// are inclusive with slack, so a candidate at exactly the K-th distance, which may still enter by its ids, is
// reached.
template <int kCap>
struct alignas(16) LdsHitList {
  uint32_t e[2 * kCap][kBlock];
};
struct LdsHitStore {
  uint32_t* col;  // &s_list.e[0][threadIdx.x]
  __device__ __forceinline__ float t(uint32_t i) const { return __uint_as_float(col[(2u * i) * kBlock]); }
  __device__ __forceinline__ uint32_t ref(uint32_t i) const { return col[(2u * i + 1u) * kBlock]; }
  __device__ __forceinline__ void set(uint32_t i, float t, uint32_t ref) {
    col[(2u * i) * kBlock] = __float_as_uint(t);
    col[(2u * i + 1u) * kBlock] = ref;
  }
};
// (geomID, primID) of a list entry's ref, as the outputs report them; read on exact ties in t and once per slot
struct HitKey {
  const uint32_t *tri_geom, *sph_geom, *tri_orig, *geom_first;
  __device__ __forceinline__ uint2 ids(uint32_t ref) const {
    const uint32_t idx = ref & kIndexMask;
    if (ref & kSphereBit) return make_uint2(sph_geom[idx], ref >> 31);
    const uint32_t g = tri_geom[idx];
    return make_uint2(g, tri_orig[idx] - geom_first[g]);
  }
  __device__ __forceinline__ uint64_t operator()(uint32_t ref) const {
    const uint2 id = ids(ref);
    return ((uint64_t)id.x << 32) | id.y;
  }
};
// one ray's list and the distance its boxes are pruned by
struct MultiHit {
  LdsHitStore hs;
  HitKey key;
  uint32_t n, k;
  float tprune;
};

// leaf_test's loop over a leaf's primitives, each tested on the ray's own interval and inserted
template <bool kDirect>
__device__ __forceinline__ void leaf_collect(uint32_t link, const uint32_t* prim_ref, const float4* tris, const float4* sph,
                                             const Ray& r, float tnear, float tfar, MultiHit& m) {
  const bool direct = kDirect && (link & kLeafDirect) != 0u;
  const uint32_t start = (link & ~kLeafBit) >> kLeafCountBits, cnt = direct ? 1u : (link & kLeafRangeMask) + 1u;
  for (uint32_t j = 0; j < cnt; ++j) {
    const uint32_t pr = direct ? (start | ((link & kLeafDirectSphere) ? kSphereBit : 0u)) : prim_ref[start + j];
    const uint32_t idx = pr & kIndexMask;
    if (pr & kSphereBit) {
      const float4 s = sph[idx];
      hit_list_sphere([&](float tn, float tf, float& t) { return sphere_hit(s, r, tn, tf, t); }, tnear, tfar,
                      [&](float t, uint32_t flag) { hit_list_insert(m.hs, m.n, m.k, t, pr | flag, m.key); });
    } else {
      float t;
      if (tri_hit(tris, idx, r, tnear, tfar, t)) hit_list_insert(m.hs, m.n, m.k, t, pr, m.key);
    }
  }
  m.tprune = hit_list_bound(m.hs, m.n, m.k, tfar);
}

// bvh2_walk, to the end, collecting
template <int N>
__device__ __forceinline__ void bvh2_walk_multi(uint32_t root, TravStack<N>& stack, const BvhNode* nodes,
                                                const uint32_t* prim_ref, const float4* tris, const float4* sph,
                                                const Ray& r, float tnear, float tfar, MultiHit& m, Visits& vc) {
  uint32_t cur = root;
  int sp = 0;
  for (;;) {
    const BvhNode* nd = nodes + cur;
    const float4 lxy = nd->lxy, rxy = nd->rxy, z = nd->z;
    const uint4 ln = nd->link;
    float tl, tr;
    bool hl = slab(lxy.x, lxy.y, lxy.z, lxy.w, z.x, z.y, r, tnear, m.tprune, tl);
    bool hr = slab(rxy.x, rxy.y, rxy.z, rxy.w, z.z, z.w, r, tnear, m.tprune, tr);
    uint32_t L = ln.x, R = ln.y;
    if (hl && (L & kLeafBit)) {
      leaf_collect<false>(L, prim_ref, tris, sph, r, tnear, tfar, m);
      hl = false;
    }
    if (hr && (R & kLeafBit)) {
      leaf_collect<false>(R, prim_ref, tris, sph, r, tnear, tfar, m);
      hr = false;
    }
    if (hl && hr) {
      if (tr < tl) {
        const uint32_t s = L;
        L = R;
        R = s;
      }
      if (sp < kStack) stack.put(sp++, R);
      else vc.stack_overflow = 1u;
      cur = L;
    } else if (hl) {
      cur = L;
    } else if (hr) {
      cur = R;
    } else {
      if (sp == 0) return;
      cur = stack.get(--sp);
    }
  }
}

// wide_walk_inl (every node from `nodes`: staged, or L2/HBM), to the end, collecting
template <int N>
__device__ __forceinline__ void wide_walk_multi(uint32_t root, TravStack<N>& stack, const WideNode* nodes,
                                                const uint32_t* prim_ref, const float4* tris, const float4* sph,
                                                const Ray& r, float tnear, float tfar, MultiHit& m, Visits& vc) {
  uint32_t cur = root;
  int sp = 0;
  for (;;) {
    const uint4* nq = reinterpret_cast<const uint4*>(nodes + cur);
    const uint4 h = nq[0], l4 = nq[1], q4 = nq[2];
    const uint2 q2 = *reinterpret_cast<const uint2*>(nq + 3);
    const uint32_t ln[4] = {l4.x, l4.y, l4.z, l4.w};
    const uint32_t qw[6] = {q4.x, q4.y, q4.z, q4.w, q2.x, q2.y};
    const QAxis ax = q_axis(__uint_as_float(h.x), h.w & 0xFFu, qw + 0, qw + 1, r.o.x, r.inv.x);
    const QAxis ay = q_axis(__uint_as_float(h.y), (h.w >> 8) & 0xFFu, qw + 2, qw + 3, r.o.y, r.inv.y);
    const QAxis az = q_axis(__uint_as_float(h.z), (h.w >> 16) & 0xFFu, qw + 4, qw + 5, r.o.z, r.inv.z);
    float t[kWide];
    bool hc[kWide];
#pragma unroll
    for (int k = 0; k < kWide; ++k) hc[k] = q_slab(k, ax, ay, az, tnear, m.tprune, t[k]) && ln[k] != kNoHit;
#pragma unroll
    for (int k = 0; k < kWide; ++k) {
      if (hc[k] && (ln[k] & kLeafBit)) {
        leaf_collect<true>(ln[k], prim_ref, tris, sph, r, tnear, tfar, m);
        hc[k] = false;
      }
    }
    int kn = kWide;
    float tn = __builtin_huge_valf();
    uint32_t npush = 0u;
#pragma unroll
    for (int k = 0; k < kWide; ++k) {
      if (hc[k] && (kn == kWide || t[k] < tn)) {
        tn = t[k];
        kn = k;
      }
      npush += hc[k] ? 1u : 0u;
    }
    if (kn < kWide) {
      if (sp + (int)npush - 1 > kStack) vc.stack_overflow = 1u;
#pragma unroll
      for (int k = kWide - 1; k >= 0; --k)
        if (hc[k] && k != kn && sp < kStack) stack.put(sp++, ln[k]);
      cur = ln[kn];
    } else {
      if (sp == 0) return;
      cur = stack.get(--sp);
    }
  }
}

template <bool kLds, bool kW4, bool kIndexed, int kCap>
__global__ void __launch_bounds__(kBlock) k_rayquery_multi(SceneView sv, RayMultiView q) {
  __shared__ KernelStack<kLds> s_stack;
  __shared__ LdsHitList<kCap> s_list;
  extern __shared__ float4 lds[];
  const Staged sc = stage_scene<kLds>(sv, lds);
  __syncthreads();
  Visits vc;
  const uint32_t K = q.k < (uint32_t)kCap ? q.k : (uint32_t)kCap;  // (the launcher picks kCap >= k)
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < q.n; j += grid_threads()) {
    const uint32_t i = kIndexed ? q.order[j] : j;
    const float4 a = q.rays[2 * (size_t)i], b = q.rays[2 * (size_t)i + 1];  // o.xyz d.x | d.yz tnear tfar
    const vec3 o = v3(a.x, a.y, a.z), d = v3(a.w, b.x, b.y);
    const Ray r = make_ray(o, d);
    const float tnear = b.z, tfar = b.w;
    MultiHit m{LdsHitStore{&s_list.e[0][threadIdx.x]}, HitKey{sv.tri_geom, sv.sph_geom, q.tri_orig, q.geom_first}, 0u, K, tfar};
    const uint32_t root = kW4 ? sv.root4 : sv.root;
    if (root != kNoHit) {
      if (root & kLeafBit) {
        leaf_collect<false>(root, sc.prim_ref, sc.tris, sc.sph, r, tnear, tfar, m);
      } else {
        TravStack<kLds ? kLdsStack : kLdsStackG> stack;
        stack.lds = &s_stack.e[0][threadIdx.x];
        if constexpr (kW4) wide_walk_multi(root, stack, sc.nodes4, sc.prim_ref, sc.tris, sc.sph, r, tnear, tfar, m, vc);
        else bvh2_walk_multi(root, stack, sc.nodes, sc.prim_ref, sc.tris, sc.sph, r, tnear, tfar, m, vc);
      }
    }
    // the records of the listed hits, once per ray and outside the walk, as k_rayquery writes its one
    q.count[i] = m.n;
    for (uint32_t e = 0; e < q.k; ++e) {
      const size_t at = (size_t)i * q.k + e;
      uint2 id = make_uint2(kNoHit, kNoHit);
      vec3 ng = v3(0.0f, 0.0f, 0.0f);
      float u = 0.0f, v = 0.0f, t = __builtin_huge_valf();
      if (e < m.n) {
        t = m.hs.t(e);
        const uint32_t ref = m.hs.ref(e), idx = ref & kIndexMask;
        if (q.geom || q.prim) id = m.key.ids(ref);
        if (ref & kSphereBit) {
          const float4 s = sc.sph[idx];
          const vec3 P = o + t * d;
          ng = v3((P.x - s.x) / s.w, (P.y - s.y) / s.w, (P.z - s.z) / s.w);
        } else {
          const float4 ta = sc.tris[3 * idx + 0], tb = sc.tris[3 * idx + 1], tc = sc.tris[3 * idx + 2];
          ng = v3(tc.y, tc.z, tc.w);
          if (q.uv) {  // as k_rayquery
            const vec3 v0 = v3(ta.x, ta.y, ta.z), e1 = v3(ta.w, tb.x, tb.y), e2 = v3(tb.z, tb.w, tc.x);
            const vec3 R = e_cross(v0 - o, d);
            const float den = e_dot(ng, d);
            const float aden = fabsf(den);
            u = xorsign(e_dot(R, e2), den) / aden;
            v = xorsign(e_dot(R, e1), den) / aden;
          }
        }
      }
      if (q.geom) q.geom[at] = id.x;
      if (q.prim) q.prim[at] = id.y;
      if (q.t) q.t[at] = t;
      if (q.ng) {
        float* n3 = q.ng + at * 3;
        n3[0] = ng.x;
        n3[1] = ng.y;
        n3[2] = ng.z;
      }
      if (q.uv) {
        q.uv[at * 2 + 0] = u;
        q.uv[at * 2 + 1] = v;
      }
    }
  }
  if (__ballot(vc.stack_overflow != 0u) && lane_id() == 0u) *q.stack_overflow = 1u;
}

void launch_rayquery_multi(const SceneView& sv, const RayMultiView& q, hipStream_t s, uint32_t* list_capacity,
                           uint32_t* lds_bytes) {
  if (q.n == 0u) return;
  const bool L = sv.lds_bytes != 0;
  const unsigned lb = L ? sv.lds_bytes : 16u;
  const unsigned need = (unsigned)(((uint64_t)q.n + kBlock - 1) / kBlock);
  dispatch(
      [&](auto fl) -> unsigned {
        return [&]<bool Lc, bool Wc, bool Ic, bool Over4, bool Over8>(Flags<Lc, Wc, Ic, Over4, Over8>) {
          constexpr int cap = Over8 ? 16 : Over4 ? 8 : 4;
          static_assert(SPTR_MULTI_HIT_MAX <= 16, "the largest instantiated capacity holds every max_hits");
          const unsigned g = std::max(1u, std::min<unsigned>(resident_grid((const void*)&k_rayquery_multi<Lc, Wc, Ic, cap>, lb), need));
          hipLaunchKernelGGL((k_rayquery_multi<Lc, Wc, Ic, cap>), dim3(g), dim3(kBlock), lb, s, sv, q);
          *list_capacity = (uint32_t)cap;
          *lds_bytes = (uint32_t)(sizeof(KernelStack<Lc>) + sizeof(LdsHitList<cap>)) + lb;
          return g;
        }(fl);
      },
      Flags<>{}, L, sv.width == (uint32_t)kWide, q.order != nullptr, q.k > 4u, q.k > 8u);
}

// --------------------------------------------------------------------------------- k_ray_keys
// Sort key of a ray, most significant part first: a 30-bit Morton code of the origin (10 bits per axis,
// quantised over the BVH root box doubled about its centre, clamped to it; a coordinate that is not finite
// goes to cell 0), the direction's sign octant (3 bits), a 16-bit Morton code of the direction's octahedral
// coordinates inside that octant (8 bits each).  A batch with one origin sorts by direction, a scattered
// batch by place first.  Keys are only sorted; none addresses memory.
__device__ __forceinline__ uint32_t spread3_10(uint32_t x) {  // 10 bits -> every third bit
  x &= 0x3FFu;
  x = (x | (x << 16)) & 0x030000FFu;
  x = (x | (x << 8)) & 0x0300F00Fu;
  x = (x | (x << 4)) & 0x030C30C3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}
__device__ __forceinline__ uint32_t spread2_8(uint32_t x) {  // 8 bits -> every second bit
  x &= 0xFFu;
  x = (x | (x << 4)) & 0x0F0Fu;
  x = (x | (x << 2)) & 0x3333u;
  x = (x | (x << 1)) & 0x5555u;
  return x;
}
// cell of x among `cells` equal cells of [lo, lo + size); outside: the nearest cell; x or the box not finite: 0
__device__ __forceinline__ uint32_t key_cell(float x, float lo, float size, uint32_t cells) {
  const float big = 3.402823466e+38f;
  if (!(fabsf(x) <= big) || !(size > 0.0f) || !(size <= big)) return 0u;
  const float f = (x - lo) / size * float(cells);
  if (!(f >= 0.0f)) return 0u;
  return f < float(cells) ? (uint32_t)f : cells - 1u;
}

__global__ void __launch_bounds__(kBlock) k_ray_keys(SceneView sv, const float4* rays, uint32_t n, uint64_t* keys,
                                                     uint32_t* index) {
  // the root box: both child boxes of the BVH2 root (kept for wide scenes too, and refitted with them)
  vec3 lo = v3(0.0f, 0.0f, 0.0f), ext = v3(0.0f, 0.0f, 0.0f);
  if (sv.num_nodes != 0u && !(sv.root & kLeafBit)) {
    const BvhNode nd = sv.nodes[sv.root];
    const vec3 l = v3(fminf(nd.lxy.x, nd.rxy.x), fminf(nd.lxy.z, nd.rxy.z), fminf(nd.z.x, nd.z.z));
    const vec3 h = v3(fmaxf(nd.lxy.y, nd.rxy.y), fmaxf(nd.lxy.w, nd.rxy.w), fmaxf(nd.z.y, nd.z.w));
    ext = v3((h.x - l.x) * 2.0f, (h.y - l.y) * 2.0f, (h.z - l.z) * 2.0f);  // doubled about the centre
    lo = v3(l.x - (h.x - l.x) * 0.5f, l.y - (h.y - l.y) * 0.5f, l.z - (h.z - l.z) * 0.5f);
  }
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += grid_threads()) {
    const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
    const uint32_t m30 = spread3_10(key_cell(a.x, lo.x, ext.x, 1024u)) | (spread3_10(key_cell(a.y, lo.y, ext.y, 1024u)) << 1) |
                         (spread3_10(key_cell(a.z, lo.z, ext.z, 1024u)) << 2);
    const float dx = a.w, dy = b.x, dz = b.y;
    const uint32_t oct = (__float_as_uint(dx) >> 31) | ((__float_as_uint(dy) >> 31) << 1) | ((__float_as_uint(dz) >> 31) << 2);
    const float l1 = fabsf(dx) + fabsf(dy) + fabsf(dz);
    const uint32_t m16 = spread2_8(key_cell(fabsf(dx), 0.0f, l1, 256u)) | (spread2_8(key_cell(fabsf(dy), 0.0f, l1, 256u)) << 1);
    keys[i] = ((uint64_t)m30 << 19) | ((uint64_t)oct << 16) | (uint64_t)m16;
    index[i] = i;
  }
}

void launch_ray_keys(const SceneView& sv, const float4* rays, uint32_t n, uint64_t* keys, uint32_t* index, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_ray_keys, dim3(grid_for(n)), dim3(kBlock), 0, s, sv, rays, n, keys, index);
}
