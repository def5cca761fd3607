// kernels_signed.hip — sptr_query_signed_distance on the device (DESIGN.md par. 6m): the table of angle-weighted
// pseudonormals, built at upload and after every geometry update, and the sign pass after a point query.
// csrc/pseudonormal.h defines every value; this file only arranges the work.  All arrays are in uploaded order:
// triangle t, corner c = 3t + k, edge slot e = 3t + k (nc = 3 * num_tris of each).
//
// Build (signed_build), on the context's stream:
//   k_sg_tris    : one thread per triangle: its three corners (gathered through the index triple, through its
//                  geometry's matrix for sptr_update_transforms, or the kept corners), live, n_t, the three
//                  angle_c * n_t, and the corners' sort keys (y | z) and (geomID | x); corners of triangles that
//                  are not live take kPnDeadKey and sort last
//   radix sort by (y | z), k_sg_gather, radix sort by (geomID | x): stable, so corners with equal keys stay in
//                  ascending corner index
//   k_sg_vhead   : a sorted corner starts a welded vertex unless it has its predecessor's geomID and compares
//                  equal to it (pn_same_pos: a NaN starts a vertex of its own); scan_u32 numbers the vertices
//   k_sg_vsum    : one thread per welded vertex: N_v summed over its run in order, written to each of its corners
//   k_sg_ekeys   : edge slot keys from the welded ids (pn_edge_key); radix sort, stable: ascending (t, k) per edge
//   k_sg_esum    : one thread per edge: N_e summed over its run in order, written to each of its slots; the
//                  incidences and their directions give the open and irregular counts
// Plain loads and vector stores; the four counts are 64-bit atomic adds, one per wave.  Every sum is sequential in
// one thread, so its bits do not depend on scheduling.
//
// k_point_sign: a resident grid with a grid-stride loop; per point p, geomID and primID of the point query: the
// triangle's corners, cp_triangle_feature, N from the table, the three outputs at the point's index.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "sptr_internal.h"
#include "xform_point.h"

namespace sptr {

namespace {

#define SG_HIP(x)                                                           \
  do {                                                                      \
    hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess) {                                                 \
      c.err = std::string("signed distance: ") + #x + ": " + hipGetErrorString(e_); \
      return SPTR_ERR_HIP;                                                  \
    }                                                                       \
  } while (0)

inline unsigned sg_grid(uint64_t work) {
  const uint64_t blocks = (work + kBlock - 1) / kBlock;
  const uint64_t cap = 256ull * 8ull;  // 256 CUs x 8 resident blocks
  return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}
__device__ __forceinline__ uint32_t sg_threads() { return gridDim.x * blockDim.x; }
__device__ __forceinline__ vec3 ld3(const float* a, size_t i) { return v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]); }
__device__ __forceinline__ void st3(float* a, size_t i, vec3 v) {
  a[3 * i] = v.x;
  a[3 * i + 1] = v.y;
  a[3 * i + 2] = v.z;
}
// one 64-bit add per wave of the lanes' 0 / 1 flags
__device__ __forceinline__ void count_wave(bool flag, unsigned long long* counter) {
  const unsigned long long m = __ballot(flag);
  if (m != 0ull && (__lane_id() == (unsigned)__builtin_ctzll(m))) atomicAdd(counter, (unsigned long long)__popcll(m));
}

struct TriIn {
  const float* pos;          // vertex positions, or null: the kept corners (cpos) are the input
  const uint32_t* idx;       // 3 per triangle
  const uint32_t* tri_geom;  // geomID per triangle
  const float* xf;           // 16 floats per triangle geometry, or null
  uint32_t nt;
};

__global__ void __launch_bounds__(kBlock) k_sg_tris(TriIn in, float* cpos, float* nhat, float* contrib, uint32_t* live,
                                                    uint64_t* key_a, uint64_t* key_b, uint32_t* val) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < in.nt; t += sg_threads()) {
    vec3 v[3];
    const uint32_t g = in.tri_geom[t];
    if (in.pos) {
      for (int k = 0; k < 3; ++k) v[k] = ld3(in.pos, in.idx[3 * (size_t)t + k]);
      if (in.xf) {
        const float* m = in.xf + 16 * (size_t)g;
        for (int k = 0; k < 3; ++k) v[k] = xform_point(m, v[k]);
      }
      for (int k = 0; k < 3; ++k) st3(cpos, 3 * (size_t)t + k, v[k]);
    } else {
      for (int k = 0; k < 3; ++k) v[k] = ld3(cpos, 3 * (size_t)t + k);
    }
    const vec3 ng = pn_tri_ng(v[0], v[1], v[2]);
    const bool lv = cp_triangle_live(ng);
    live[t] = lv ? 1u : 0u;
    const vec3 n = lv ? pn_unit_normal(ng) : v3(0.0f, 0.0f, 0.0f);
    st3(nhat, t, n);
    for (uint32_t k = 0; k < 3; ++k) {
      const size_t c = 3 * (size_t)t + k;
      st3(contrib, c, lv ? n * pn_corner_angle(v[0], v[1], v[2], k) : v3(0.0f, 0.0f, 0.0f));
      key_a[c] = lv ? ((uint64_t)pn_pos_bits(v[k].y) << 32) | pn_pos_bits(v[k].z) : kPnDeadKey;
      key_b[c] = lv ? ((uint64_t)g << 32) | pn_pos_bits(v[k].x) : kPnDeadKey;
      val[c] = (uint32_t)c;
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_sg_gather(const uint64_t* key, const uint32_t* order, uint32_t n, uint64_t* out) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += sg_threads()) out[j] = key[order[j]];
}

// head[j] = 1 where sorted corner j starts a welded vertex
__global__ void __launch_bounds__(kBlock) k_sg_vhead(const uint32_t* order, uint32_t nc, const uint32_t* live,
                                                     const uint32_t* tri_geom, const float* cpos, uint32_t* head) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nc; j += sg_threads()) {
    const uint32_t c = order[j];
    uint32_t h = 0u;
    if (live[c / 3u]) {
      h = 1u;
      if (j != 0u) {
        const uint32_t b = order[j - 1u];  // (live: the corners that are not sort last)
        if (live[b / 3u] && tri_geom[b / 3u] == tri_geom[c / 3u] && pn_same_pos(ld3(cpos, b), ld3(cpos, c))) h = 0u;
      }
    }
    head[j] = h;
  }
}

__global__ void __launch_bounds__(kBlock) k_sg_vsum(const uint32_t* order, uint32_t nc, const uint32_t* live,
                                                    const uint32_t* head, const uint32_t* wofs, const float* nhat,
                                                    const float* contrib, float* nv, uint32_t* wid,
                                                    unsigned long long* counts) {
  const uint32_t j0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t base = 0; base < nc; base += sg_threads()) {  // (whole waves stay in the loop for the ballot)
    const uint32_t j = base + j0;
    const bool is_head = j < nc && head[j] != 0u;
    if (is_head) {
      uint32_t e = j + 1u;
      while (e < nc && head[e] == 0u && live[order[e] / 3u]) ++e;
      vec3 sum = v3(0.0f, 0.0f, 0.0f);
      for (uint32_t i = j; i < e; ++i) {
        const uint32_t c = order[i];
        if (pn_finite3(ld3(nhat, c / 3u))) sum = sum + ld3(contrib, c);
      }
      const uint32_t id = wofs[j];  // exclusive scan of head: the heads before this one
      for (uint32_t i = j; i < e; ++i) {
        const uint32_t c = order[i];
        st3(nv, c, sum);
        wid[c] = id;
      }
    }
    count_wave(is_head, &counts[0]);
  }
}

__global__ void __launch_bounds__(kBlock) k_sg_ekeys(uint32_t nt, const uint32_t* live, const uint32_t* wid, uint64_t* key,
                                                     uint32_t* val) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += sg_threads()) {
    const bool lv = live[t] != 0u;
    for (uint32_t k = 0; k < 3; ++k) {
      const size_t e = 3 * (size_t)t + k;
      key[e] = lv ? pn_edge_key(wid[3 * (size_t)t + pn_edge_lo(k)], wid[3 * (size_t)t + pn_edge_hi(k)]) : kPnDeadKey;
      val[e] = (uint32_t)e;
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_sg_esum(const uint64_t* key, const uint32_t* order, uint32_t nc,
                                                    const uint32_t* wid, const float* nhat, float* ne,
                                                    unsigned long long* counts) {
  const uint32_t j0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t base = 0; base < nc; base += sg_threads()) {
    const uint32_t j = base + j0;
    bool is_head = false, open = false, irregular = false;
    if (j < nc) {
      const uint64_t kj = key[j];
      is_head = kj != kPnDeadKey && (j == 0u || key[j - 1u] != kj);
      if (is_head) {
        uint32_t e = j + 1u;
        while (e < nc && key[e] == kj) ++e;
        vec3 sum = v3(0.0f, 0.0f, 0.0f);
        uint32_t fwd = 0u, bwd = 0u;
        for (uint32_t i = j; i < e; ++i) {
          const uint32_t s = order[i], t = s / 3u, k = s - 3u * t;
          const vec3 n = ld3(nhat, t);
          if (pn_finite3(n)) sum = sum + n;
          if (pn_edge_forward(k, wid[3 * (size_t)t + pn_edge_lo(k)], wid[3 * (size_t)t + pn_edge_hi(k)])) ++fwd;
          else ++bwd;
        }
        for (uint32_t i = j; i < e; ++i) st3(ne, order[i], sum);
        open = e - j == 1u;
        irregular = !(fwd == 1u && bwd == 1u);
      }
    }
    count_wave(is_head, &counts[1]);
    count_wave(open, &counts[2]);
    count_wave(irregular, &counts[3]);
  }
}

__global__ void __launch_bounds__(kBlock) k_point_sign(PointSignView v) {
  const float inf = __builtin_huge_valf();
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n; i += sg_threads()) {
    const float4 a = v.points[i];
    const vec3 p = v3(a.x, a.y, a.z);
    const uint32_t g = v.geom[i], pr = v.prim[i];
    float sd = inf;
    vec3 n = v3(0.0f, 0.0f, 0.0f);
    uint32_t f = kCpMiss;
    if (g != kNoHit) {
      if (g < v.num_tri_geoms) {
        const uint64_t t = (uint64_t)v.geom_first[g] + pr;
        if (t < v.num_tris)  // (always, for ids the point query wrote)
          sd = pn_triangle_result(ld3(v.cpos, 3 * t), ld3(v.cpos, 3 * t + 1), ld3(v.cpos, 3 * t + 2), v.nv + 9 * t, v.ne + 9 * t, p,
                                  v.flip != 0u, n, f);
      } else if (g - v.num_tri_geoms < v.num_sph) {
        const float4 s = v.sph[g - v.num_tri_geoms];
        sd = pn_sphere_result(v3(s.x, s.y, s.z), s.w, p, n);
        f = kCpSphere;
      }
    }
    if (v.signed_dist) v.signed_dist[i] = sd;
    if (v.normal) st3(v.normal, i, n);
    if (v.feature) v.feature[i] = f;
  }
}

// The tables from the inputs `in` describes (in.pos null: the kept corners), on c.stream; returns when done.
int signed_build(Context& c, const TriIn& in) {
  SignedState& g = c.sg;
  const uint32_t nt = g.num_tris, nc = 3u * nt;
  hipStream_t s = c.stream;
  g.valid = false;  // until the new tables stand
  for (DevEvent& e : g.ev)
    if (!e) SG_HIP(hipEventCreate(e.put()));
  SG_HIP(g.counts.ensure(32));
  SG_HIP(hipEventRecord(g.ev[0], s));
  SG_HIP(hipMemsetAsync(g.counts.p, 0, 32, s));
  if (nt != 0u) {
    size_t sort_bytes = 0, scan_bytes = 0;
    SG_HIP(radix_sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, nc, s));
    SG_HIP(scan_u32(nullptr, scan_bytes, nullptr, nullptr, nc, s));
    SG_HIP(g.temp.ensure(std::max(sort_bytes, scan_bytes)));
    SG_HIP(g.nv.ensure((size_t)nc * 12));
    SG_HIP(g.ne.ensure((size_t)nc * 12));
    SG_HIP(g.contrib.ensure((size_t)nc * 12));
    SG_HIP(g.nhat.ensure((size_t)nt * 12));
    SG_HIP(g.live.ensure((size_t)nt * 4));
    SG_HIP(g.key_a.ensure((size_t)nc * 8));
    SG_HIP(g.key_b.ensure((size_t)nc * 8));
    SG_HIP(g.key_s.ensure((size_t)nc * 8));
    for (DevBuf* b : {&g.val0, &g.val1, &g.val2, &g.head, &g.wofs, &g.wid}) SG_HIP(b->ensure((size_t)nc * 4));
    float *cpos = static_cast<float*>(g.cpos.p), *nhat = static_cast<float*>(g.nhat.p), *contrib = static_cast<float*>(g.contrib.p);
    float *nv = static_cast<float*>(g.nv.p), *ne = static_cast<float*>(g.ne.p);
    uint32_t *live = static_cast<uint32_t*>(g.live.p), *val0 = static_cast<uint32_t*>(g.val0.p),
             *val1 = static_cast<uint32_t*>(g.val1.p), *val2 = static_cast<uint32_t*>(g.val2.p),
             *head = static_cast<uint32_t*>(g.head.p), *wofs = static_cast<uint32_t*>(g.wofs.p),
             *wid = static_cast<uint32_t*>(g.wid.p);
    uint64_t *key_a = static_cast<uint64_t*>(g.key_a.p), *key_b = static_cast<uint64_t*>(g.key_b.p),
             *key_s = static_cast<uint64_t*>(g.key_s.p);
    unsigned long long* counts = static_cast<unsigned long long*>(g.counts.p);
    const uint32_t* tri_geom = static_cast<const uint32_t*>(g.tri_geom.p);
    // corners of triangles that are not live keep 0 in both tables and no welded id
    SG_HIP(hipMemsetAsync(nv, 0, (size_t)nc * 12, s));
    SG_HIP(hipMemsetAsync(ne, 0, (size_t)nc * 12, s));
    SG_HIP(hipMemsetAsync(wid, 0xFF, (size_t)nc * 4, s));
    hipLaunchKernelGGL(k_sg_tris, dim3(sg_grid(nt)), dim3(kBlock), 0, s, in, cpos, nhat, contrib, live, key_a, key_b, val0);
    size_t tb = g.temp.bytes;
    SG_HIP(radix_sort_pairs_u64(g.temp.p, tb, key_a, key_s, val0, val1, nc, s));
    hipLaunchKernelGGL(k_sg_gather, dim3(sg_grid(nc)), dim3(kBlock), 0, s, key_b, val1, nc, key_a);
    tb = g.temp.bytes;
    SG_HIP(radix_sort_pairs_u64(g.temp.p, tb, key_a, key_s, val1, val2, nc, s));
    hipLaunchKernelGGL(k_sg_vhead, dim3(sg_grid(nc)), dim3(kBlock), 0, s, val2, nc, live, tri_geom, cpos, head);
    tb = g.temp.bytes;
    SG_HIP(scan_u32(g.temp.p, tb, head, wofs, nc, s));
    hipLaunchKernelGGL(k_sg_vsum, dim3(sg_grid(nc)), dim3(kBlock), 0, s, val2, nc, live, head, wofs, nhat, contrib, nv, wid, counts);
    // (val0 is rewritten with the identity: the corner sort's first pass left it alone, but the names stay honest)
    hipLaunchKernelGGL(k_sg_ekeys, dim3(sg_grid(nt)), dim3(kBlock), 0, s, nt, live, wid, key_a, val0);
    tb = g.temp.bytes;
    SG_HIP(radix_sort_pairs_u64(g.temp.p, tb, key_a, key_s, val0, val1, nc, s));
    hipLaunchKernelGGL(k_sg_esum, dim3(sg_grid(nc)), dim3(kBlock), 0, s, key_s, val1, nc, wid, nhat, ne, counts);
    SG_HIP(hipGetLastError());
  }
  SG_HIP(hipEventRecord(g.ev[1], s));
  SG_HIP(hipMemcpyAsync(g.counts_h, g.counts.p, 32, hipMemcpyDeviceToHost, s));
  SG_HIP(hipStreamSynchronize(s));
  float ms = 0.0f;
  SG_HIP(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
  g.ms_build = ms;
  ++g.builds;
  g.valid = true;
  return SPTR_OK;
}

}  // namespace

void signed_release(Context& c) {
  SignedState& g = c.sg;
  g.valid = false;
  for (DevBuf* b : {&g.cpos, &g.idx, &g.tri_geom, &g.sph, &g.nv, &g.ne, &g.pos, &g.contrib, &g.nhat, &g.live, &g.key_a, &g.key_b,
                    &g.key_s, &g.val0, &g.val1, &g.val2, &g.head, &g.wofs, &g.wid, &g.temp})
    b->release();
  for (uint64_t& x : g.counts_h) x = 0;
}

int signed_build_upload(Context& c, const float* h_pos, uint32_t nverts, const uint32_t* h_idx, uint32_t ntris,
                        const float* h_sph, uint32_t nsph, const uint32_t* h_tri_geom, uint32_t num_tri_geoms) {
  SignedState& g = c.sg;
  g.valid = false;
  g.num_tris = ntris;
  g.num_sph = nsph;
  g.num_tri_geoms = num_tri_geoms;
  hipStream_t s = c.stream;
  SG_HIP(g.cpos.ensure((size_t)ntris * 36));
  SG_HIP(g.idx.ensure((size_t)ntris * 12));
  SG_HIP(g.tri_geom.ensure((size_t)ntris * 4));
  SG_HIP(g.pos.ensure((size_t)nverts * 12));
  SG_HIP(g.sph.ensure((size_t)nsph * 16));
  if (ntris) {
    SG_HIP(hipMemcpyAsync(g.pos.p, h_pos, (size_t)nverts * 12, hipMemcpyHostToDevice, s));
    SG_HIP(hipMemcpyAsync(g.idx.p, h_idx, (size_t)ntris * 12, hipMemcpyHostToDevice, s));
    SG_HIP(hipMemcpyAsync(g.tri_geom.p, h_tri_geom, (size_t)ntris * 4, hipMemcpyHostToDevice, s));
  }
  if (nsph) SG_HIP(hipMemcpyAsync(g.sph.p, h_sph, (size_t)nsph * 16, hipMemcpyHostToDevice, s));
  TriIn in{static_cast<const float*>(g.pos.p), static_cast<const uint32_t*>(g.idx.p), static_cast<const uint32_t*>(g.tri_geom.p),
           nullptr, ntris};
  return signed_build(c, in);  // (returns after the stream drained: the host arrays are free again)
}

int signed_rebuild(Context& c, const float* d_pos, const float* d_xf, const float4* d_sph) {
  SignedState& g = c.sg;
  if (!g.valid) return SPTR_OK;
  if (d_sph && g.num_sph)
    SG_HIP(hipMemcpyAsync(g.sph.p, d_sph, (size_t)g.num_sph * 16, hipMemcpyDeviceToDevice, c.stream));
  TriIn in{d_pos, static_cast<const uint32_t*>(g.idx.p), static_cast<const uint32_t*>(g.tri_geom.p), d_pos ? d_xf : nullptr,
           g.num_tris};
  return signed_build(c, in);
}

void launch_point_sign(const PointSignView& v, hipStream_t s) {
  if (v.n) hipLaunchKernelGGL(k_point_sign, dim3(sg_grid(v.n)), dim3(kBlock), 0, s, v);
}

}  // namespace sptr
