// kernels_query.h — batched ray queries on caller buffers (sptr_query_rays): the trace kernel k_rayquery and
// the sort-key kernel k_ray_keys.  Included by kernels_wavefront.hip inside namespace sptr, after its
// traversal helpers and launch utilities, which these kernels share: k_rayquery walks the BVH through
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
