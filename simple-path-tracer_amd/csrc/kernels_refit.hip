// kernels_refit.hip — in-place refit of an uploaded scene whose coordinates moved
// (sptr_update_geometry, DESIGN.md "Dynamic scenes").  The tree topology, the slot order and every link
// stay the upload's; three passes recompute what depends on coordinates:
//   k_refit_slots : one thread per sorted position: the triangle record (tri_record, the function
//                   k_leaves calls) through the slot-order index triples, or the sphere, written in
//                   place, and the position's box
//   k_refit_nodes : BVH2 child boxes, one launch per subtree height (ascending): a child box is the
//                   union of a leaf range's position boxes, or of the child node's two boxes, which an
//                   earlier launch finished.  k_refit_nodes_block: the same for trees of at most
//                   kRefitBlockNodes nodes (the scenes staged in LDS), one block walking the heights
//                   with __syncthreads() between them
//   k_refit_wide  : every wide node re-quantised (quantize_wide, the function k_wide_emit calls) from
//                   the BVH2 boxes its children were collapsed from (the source table k_wide_sources
//                   wrote at upload)
// k_refit_slots<true> (sptr_update_transforms) is the slot pass reading a kept rest pose and moving each
// triangle's vertices by its geometry's matrix first; k_tree_cost (sptr_tree_cost) sums the BVH2's child box
// areas in a fixed shape ("Transforms").
// No kernel here waits for, or hands data to, another workgroup of its launch: kernel boundaries and
// __syncthreads() are the only synchronisation.  fminf / fmaxf are exact, so a box does not depend on
// the order its parts are merged in (the build's k_refit merges in tree order), up to the sign of a zero.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "lbvh_shared.h"
#include "sptr_internal.h"
#include "xform_point.h"

namespace sptr {

namespace {

#define RF_CHECK(x)                                                    \
  do {                                                                 \
    hipError_t e_ = (x);                                               \
    if (e_ != hipSuccess) {                                            \
      c.err = std::string("refit: ") + #x + ": " + hipGetErrorString(e_); \
      return SPTR_ERR_HIP;                                             \
    }                                                                  \
  } while (0)

constexpr uint32_t kRefitBlockNodes = 1024;  // trees up to this many nodes: one block walks the heights

struct SlotIn {
  const float* pos;          // vertex positions, or null: triangles keep their records and boxes
  const float4* sph_in;      // spheres in upload order, or null: spheres keep theirs
  const uint32_t* idx;       // 3 vertex indices per triangle slot
  const uint32_t* sph_orig;  // sphere slot -> index in the upload
  const uint32_t* prim_ref;  // sorted position -> [kSphereBit] | slot
  uint32_t n;                // sorted positions
};

// kXf (sptr_update_transforms): in.pos is the rest pose, and a triangle's three gathered vertices go through
// its geometry's matrix (xform_point, the host flattening's arithmetic) before the record and the box:
// tri_geom[slot] = the slot's geomID, xf = 16 floats per triangle geometry (glm layout; 12 are read).  A
// vertex shared by triangles of two geometries is transformed per triangle; no position is written back.
// Without kXf the two tables are not read, and the code is the kernel's as it was before the template.
template <bool kXf>
__global__ void __launch_bounds__(256) k_refit_slots(SlotIn in, float4* tris, float4* sph, float4* box_lo, float4* box_hi,
                                                     const uint32_t* tri_geom, const float* xf) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < in.n; i += gridDim.x * blockDim.x) {
    const uint32_t ref = in.prim_ref[i], slot = ref & kIndexMask;
    vec3 lo, hi;
    if (ref & kSphereBit) {
      if (!in.sph_in) continue;
      const float4 s = in.sph_in[in.sph_orig[slot]];
      sph[slot] = s;
      sphere_box(s, lo, hi);
    } else {
      if (!in.pos) continue;
      const uint32_t a = in.idx[3 * slot], b = in.idx[3 * slot + 1], c = in.idx[3 * slot + 2];
      vec3 v0 = v3(in.pos[3 * a], in.pos[3 * a + 1], in.pos[3 * a + 2]);
      vec3 v1 = v3(in.pos[3 * b], in.pos[3 * b + 1], in.pos[3 * b + 2]);
      vec3 v2 = v3(in.pos[3 * c], in.pos[3 * c + 1], in.pos[3 * c + 2]);
      if (kXf) {
        // (slots are in tree order, so most of a wave reads one geometry's matrix: one cache line)
        const float* m = xf + 16 * (size_t)tri_geom[slot];
        v0 = xform_point(m, v0);
        v1 = xform_point(m, v1);
        v2 = xform_point(m, v2);
      }
      float4 rec[3];
      tri_record(v0, v1, v2, rec);
      tris[3 * slot + 0] = rec[0];
      tris[3 * slot + 1] = rec[1];
      tris[3 * slot + 2] = rec[2];
      tri_box(v0, v1, v2, lo, hi);
    }
    box_lo[i] = make_float4(lo.x, lo.y, lo.z, 0.0f);
    box_hi[i] = make_float4(hi.x, hi.y, hi.z, 0.0f);
  }
}

// idx_out[3 * slot ..] = the uploaded triple of the slot's triangle
__global__ void k_slot_indices(uint32_t nslots, const uint32_t* tri_orig, const uint32_t* idx, uint32_t* idx_out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += gridDim.x * blockDim.x) {
    const uint32_t p = tri_orig[i];
    idx_out[3 * i] = idx[3 * p];
    idx_out[3 * i + 1] = idx[3 * p + 1];
    idx_out[3 * i + 2] = idx[3 * p + 2];
  }
}

struct Box6 {
  float lo[3], hi[3];
};
// the box of a BVH2 child link: a leaf range of sorted positions, or a node of a smaller height
__device__ __forceinline__ Box6 child_box(uint32_t link, const BvhNode* nodes, const float4* box_lo, const float4* box_hi) {
  Box6 b;
  if (link & kLeafBit) {
    const uint32_t start = (link & ~kLeafBit) >> kLeafCountBits, cnt = (link & kLeafRangeMask) + 1u;
    const float4 l0 = box_lo[start], h0 = box_hi[start];
    b.lo[0] = l0.x; b.lo[1] = l0.y; b.lo[2] = l0.z;
    b.hi[0] = h0.x; b.hi[1] = h0.y; b.hi[2] = h0.z;
    for (uint32_t k = 1; k < cnt; ++k) {
      const float4 l = box_lo[start + k], h = box_hi[start + k];
      b.lo[0] = fminf(b.lo[0], l.x); b.lo[1] = fminf(b.lo[1], l.y); b.lo[2] = fminf(b.lo[2], l.z);
      b.hi[0] = fmaxf(b.hi[0], h.x); b.hi[1] = fmaxf(b.hi[1], h.y); b.hi[2] = fmaxf(b.hi[2], h.z);
    }
  } else {
    const BvhNode* cn = nodes + link;
    const float4 l = cn->lxy, r = cn->rxy, z = cn->z;
    b.lo[0] = fminf(l.x, r.x); b.hi[0] = fmaxf(l.y, r.y);
    b.lo[1] = fminf(l.z, r.z); b.hi[1] = fmaxf(l.w, r.w);
    b.lo[2] = fminf(z.x, z.z); b.hi[2] = fmaxf(z.y, z.w);
  }
  return b;
}
__device__ __forceinline__ void refit_node(uint32_t x, BvhNode* nodes, const float4* box_lo, const float4* box_hi) {
  const uint4 link = nodes[x].link;
  const Box6 l = child_box(link.x, nodes, box_lo, box_hi), r = child_box(link.y, nodes, box_lo, box_hi);
  nodes[x].lxy = make_float4(l.lo[0], l.hi[0], l.lo[1], l.hi[1]);
  nodes[x].rxy = make_float4(r.lo[0], r.hi[0], r.lo[1], r.hi[1]);
  nodes[x].z = make_float4(l.lo[2], l.hi[2], r.lo[2], r.hi[2]);
}

// the nodes of one height: order[0 .. count)
__global__ void __launch_bounds__(256) k_refit_nodes(const uint32_t* order, uint32_t count, BvhNode* nodes, const float4* box_lo,
                                                     const float4* box_hi) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x)
    refit_node(order[i], nodes, box_lo, box_hi);
}
// one block, every height: nodes of height h are order[hoff[h] .. hoff[h + 1]); the barrier (with its
// workgroup-scope fence) makes height h's boxes visible to the threads that read them for height h + 1
__global__ void __launch_bounds__(256) k_refit_nodes_block(const uint32_t* order, const uint32_t* hoff, uint32_t max_h,
                                                           BvhNode* nodes, const float4* box_lo, const float4* box_hi) {
  for (uint32_t h = 1; h <= max_h; ++h) {
    const uint32_t lo = hoff[h], hi = hoff[h + 1];
    for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) refit_node(order[i], nodes, box_lo, box_hi);
    __syncthreads();
  }
}

// wide node base + j of one level: where each of its child boxes is read from
__global__ void k_wide_sources(uint32_t ncur, const uint2* cur, uint32_t base, const BvhNode* nodes, uint32_t* wsrc) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < ncur; j += gridDim.x * blockDim.x) {
    WideBoxes b;
    uint32_t src[kWide];
    (void)expand_greedy_t<true>(nodes, cur[j].x, b, src);
    for (int e = 0; e < kWide; ++e) wsrc[(size_t)(base + j) * kWide + e] = src[e];
  }
}

__global__ void __launch_bounds__(256) k_refit_wide(uint32_t nw, WideNode* nodes4, const uint32_t* wsrc, const BvhNode* nodes) {
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += gridDim.x * blockDim.x) {
    const WideNode old = nodes4[w];
    const int n = (int)(old.ex >> 24);
    WideBoxes b;
    for (int e = 0; e < kWide; ++e) {
      b.link[e] = old.link[e];
      for (int a = 0; a < 3; ++a) b.lo[a][e] = b.hi[a][e] = 0.0f;
      const uint32_t s = wsrc[(size_t)w * kWide + e];
      if (e >= n || s == kNoHit) continue;
      const BvhNode* nd = nodes + (s >> 1);
      const float4 xy = (s & 1u) ? nd->rxy : nd->lxy, z = nd->z;
      b.lo[0][e] = xy.x; b.hi[0][e] = xy.y; b.lo[1][e] = xy.z; b.hi[1][e] = xy.w;
      b.lo[2][e] = (s & 1u) ? z.z : z.x;
      b.hi[2][e] = (s & 1u) ? z.w : z.y;
    }
    // the child count as a constant: quantize_wide's loops unroll and the child arrays stay in registers
    // (with a variable count they live in scratch); the same function either way, so the same bits
    WideNode o;
    if (n == 2) o = quantize_wide(b, 2, old.parent);
    else if (n == 3) o = quantize_wide(b, 3, old.parent);
    else o = quantize_wide(b, kWide, old.parent);
    nodes4[w] = o;
  }
}

unsigned blocks_for(size_t n) {
  size_t b = (n + 255) / 256;
  if (b < 1) b = 1;
  if (b > 4096) b = 4096;
  return (unsigned)b;
}

// d_xf == null: d_pos holds world positions; else d_pos is the rest pose and d_xf the matrix table
void launch_slots(Context& c, const float* d_pos, const float4* d_sph, const float* d_xf = nullptr) {
  const uint32_t n = c.num_tri_refs + c.num_sph;
  SlotIn in{d_pos, d_sph, static_cast<const uint32_t*>(c.rf.idx.p), static_cast<const uint32_t*>(c.sph_orig.p),
            static_cast<const uint32_t*>(c.prim_ref.p), n};
  float4 *tris = static_cast<float4*>(c.tris.p), *sph = static_cast<float4*>(c.sph.p);
  float4 *blo = static_cast<float4*>(c.rf.box_lo.p), *bhi = static_cast<float4*>(c.rf.box_hi.p);
  if (d_xf)
    hipLaunchKernelGGL(k_refit_slots<true>, dim3(blocks_for(n)), dim3(256), 0, c.stream, in, tris, sph, blo, bhi,
                       static_cast<const uint32_t*>(c.tri_geom.p), d_xf);
  else
    hipLaunchKernelGGL(k_refit_slots<false>, dim3(blocks_for(n)), dim3(256), 0, c.stream, in, tris, sph, blo, bhi,
                       static_cast<const uint32_t*>(nullptr), static_cast<const float*>(nullptr));
}

// ---- tree cost (sptr_tree_cost) ------------------------------------------------------------------
// Sum over the BVH2's inner nodes, over both child boxes b, of w * A(b): A = 2 (dx dy + dy dz + dz dx) in
// double from the float extents, w = 1 for an inner child, the range's primitive count for a leaf child.
// A node counts when the walk can reach it: more than leaf_max primitives below it (a smaller subtree is
// its parent's leaf range; link.w, k_karras).  The shape is fixed by the node count alone: thread t of the
// grid adds its nodes in ascending order, a block folds its 256 sums as a binary tree in LDS and stores one
// partial, and the host adds the partials in block order; so one tree gives one result, bit for bit, on
// every call.  No atomics.  partial[gridDim.x] = the area of the union of the root's two child boxes.
__device__ __forceinline__ double box_area_d(float lx, float hx, float ly, float hy, float lz, float hz) {
  const double dx = (double)hx - (double)lx, dy = (double)hy - (double)ly, dz = (double)hz - (double)lz;
  return 2.0 * (dx * dy + dy * dz + dz * dx);
}
__device__ __forceinline__ double link_weight(uint32_t link) {
  return (link & kLeafBit) ? (double)((link & kLeafRangeMask) + 1u) : 1.0;
}
__global__ void __launch_bounds__(256) k_tree_cost(uint32_t nn, uint32_t leaf_max, const BvhNode* nodes, double* partial) {
  __shared__ double s_sum[256];
  double acc = 0.0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
    const uint4 link = nodes[i].link;
    if (link.w <= leaf_max) continue;
    const float4 l = nodes[i].lxy, r = nodes[i].rxy, z = nodes[i].z;
    acc += link_weight(link.x) * box_area_d(l.x, l.y, l.z, l.w, z.x, z.y);
    acc += link_weight(link.y) * box_area_d(r.x, r.y, r.z, r.w, z.z, z.w);
  }
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) s_sum[threadIdx.x] += s_sum[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s_sum[0];
    if (blockIdx.x == 0) {
      const float4 l = nodes[0].lxy, r = nodes[0].rxy, z = nodes[0].z;
      partial[gridDim.x] = box_area_d(fminf(l.x, r.x), fmaxf(l.y, r.y), fminf(l.z, r.z), fmaxf(l.w, r.w), fminf(z.x, z.z),
                                      fmaxf(z.y, z.w));
    }
  }
}
constexpr unsigned kCostBlocksMax = 1024;

}  // namespace

void refit_release(Context& c) {
  RefitState& r = c.rf;
  for (DevBuf* b : {&r.idx, &r.box_lo, &r.box_hi, &r.order, &r.hoff, &r.wsrc, &r.in_pos, &r.in_sph, &r.snap, &r.rest, &r.in_xf,
                    &r.cost_part})
    b->release();
  r.xf_valid = false;
  r.hoff_h.clear();
  r.valid = false;
}

// Two device-to-device copies: 48 B per triangle slot, then 16 B per sphere.
int refit_snapshot(Context& c) {
  RefitState& r = c.rf;
  hipStream_t s = c.stream;
  for (DevEvent& e : r.snap_ev)
    if (!e) RF_CHECK(hipEventCreate(e.put()));
  const size_t tb = (size_t)c.num_tri_refs * 48, sb = (size_t)c.num_sph * 16;
  RF_CHECK(r.snap.ensure(tb + sb > 0 ? tb + sb : 16));
  RF_CHECK(hipEventRecord(r.snap_ev[0], s));
  if (tb) RF_CHECK(hipMemcpyAsync(r.snap.p, c.tris.p, tb, hipMemcpyDeviceToDevice, s));
  if (sb) RF_CHECK(hipMemcpyAsync(static_cast<char*>(r.snap.p) + tb, c.sph.p, sb, hipMemcpyDeviceToDevice, s));
  RF_CHECK(hipEventRecord(r.snap_ev[1], s));
  RF_CHECK(hipStreamSynchronize(s));
  float ms = 0.0f;
  RF_CHECK(hipEventElapsedTime(&ms, r.snap_ev[0], r.snap_ev[1]));
  r.ms_snapshot = ms;
  ++r.snapshots;
  return SPTR_OK;
}

int refit_retain_slots(Context& c, const float* d_pos, const uint32_t* d_idx, const float4* d_sph) {
  const uint32_t n = c.num_tri_refs + c.num_sph;
  RF_CHECK(c.rf.idx.ensure((size_t)c.num_tri_refs * 12));
  RF_CHECK(c.rf.box_lo.ensure((size_t)n * 16));
  RF_CHECK(c.rf.box_hi.ensure((size_t)n * 16));
  if (c.num_tri_refs)
    hipLaunchKernelGGL(k_slot_indices, dim3(blocks_for(c.num_tri_refs)), dim3(256), 0, c.stream, c.num_tri_refs,
                       static_cast<const uint32_t*>(c.tri_orig.p), d_idx, static_cast<uint32_t*>(c.rf.idx.p));
  // the first boxes (and, bit for bit, the records k_leaves just wrote): a later update of the positions
  // or of the spheres alone finds the other kind's boxes here
  launch_slots(c, c.num_tri_refs ? d_pos : nullptr, c.num_sph ? d_sph : nullptr);
  RF_CHECK(hipGetLastError());
  return SPTR_OK;
}

void launch_wide_sources(uint32_t ncur, const uint2* cur, uint32_t base, const BvhNode* nodes, uint32_t* wsrc, hipStream_t s) {
  hipLaunchKernelGGL(k_wide_sources, dim3(blocks_for(ncur)), dim3(256), 0, s, ncur, cur, base, nodes, wsrc);
}

int refit_lbvh(Context& c, const float* d_pos, const float4* d_sph, const float* d_xf) {
  const auto t0 = std::chrono::steady_clock::now();
  RefitState& r = c.rf;
  hipStream_t s = c.stream;
  for (DevEvent& e : r.ev)
    if (!e) RF_CHECK(hipEventCreate(e.put()));
  BvhNode* nodes = static_cast<BvhNode*>(c.nodes.p);
  const float4 *blo = static_cast<const float4*>(r.box_lo.p), *bhi = static_cast<const float4*>(r.box_hi.p);
  RF_CHECK(hipEventRecord(r.ev[0], s));
  if (c.num_tri_refs + c.num_sph) launch_slots(c, c.num_tri_refs ? d_pos : nullptr, c.num_sph ? d_sph : nullptr, d_xf);
  RF_CHECK(hipEventRecord(r.ev[1], s));
  if (c.num_nodes) {
    const uint32_t* order = static_cast<const uint32_t*>(r.order.p);
    if (c.num_nodes <= kRefitBlockNodes) {
      hipLaunchKernelGGL(k_refit_nodes_block, dim3(1), dim3(256), 0, s, order, static_cast<const uint32_t*>(r.hoff.p), r.max_h,
                         nodes, blo, bhi);
    } else {
      for (uint32_t h = 1; h <= r.max_h; ++h) {
        const uint32_t lo = r.hoff_h[h], cnt = r.hoff_h[h + 1] - lo;
        if (cnt) hipLaunchKernelGGL(k_refit_nodes, dim3(blocks_for(cnt)), dim3(256), 0, s, order + lo, cnt, nodes, blo, bhi);
      }
    }
  }
  RF_CHECK(hipEventRecord(r.ev[2], s));
  if (c.num_nodes4)
    hipLaunchKernelGGL(k_refit_wide, dim3(blocks_for(c.num_nodes4)), dim3(256), 0, s, c.num_nodes4,
                       static_cast<WideNode*>(c.nodes4.p), static_cast<const uint32_t*>(r.wsrc.p), nodes);
  RF_CHECK(hipGetLastError());
  RF_CHECK(hipEventRecord(r.ev[3], s));
  RF_CHECK(hipStreamSynchronize(s));
  float ms = 0.0f;
  for (int k = 0; k < 3; ++k) {
    RF_CHECK(hipEventElapsedTime(&ms, r.ev[k], r.ev[k + 1]));
    r.ms_stage[k] = ms;
  }
  RF_CHECK(hipEventElapsedTime(&ms, r.ev[0], r.ev[3]));
  r.ms_device = ms;
  ++r.refits;
  r.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // SPTR_REFIT_STAGES=1: the device ms of the three passes, for the measurements of DESIGN.md
  static const bool print = std::getenv("SPTR_REFIT_STAGES") != nullptr;
  if (print)
    std::fprintf(stderr, "refit %u: slots %.4f ms, bvh2 %.4f ms (%u heights), wide %.4f ms, wall %.4f ms\n", r.refits,
                 r.ms_stage[0], r.ms_stage[1], r.max_h, r.ms_stage[2], r.ms_wall);
  return SPTR_OK;
}

// One k_tree_cost launch on c.stream and the in-order sum of its partials on the host; returns when done.
int refit_tree_cost(Context& c, double* cost, double* root_area) {
  RefitState& r = c.rf;
  *cost = *root_area = 0.0;
  if (!c.num_nodes) return SPTR_OK;  // a single primitive: no inner node
  hipStream_t s = c.stream;
  for (DevEvent& e : r.cost_ev)
    if (!e) RF_CHECK(hipEventCreate(e.put()));
  const unsigned blocks = std::min(blocks_for(c.num_nodes), kCostBlocksMax);
  RF_CHECK(r.cost_part.ensure((size_t)(kCostBlocksMax + 1) * sizeof(double)));
  RF_CHECK(hipEventRecord(r.cost_ev[0], s));
  hipLaunchKernelGGL(k_tree_cost, dim3(blocks), dim3(256), 0, s, c.num_nodes, c.leaf_used, static_cast<const BvhNode*>(c.nodes.p),
                     static_cast<double*>(r.cost_part.p));
  RF_CHECK(hipGetLastError());
  RF_CHECK(hipEventRecord(r.cost_ev[1], s));
  double part[kCostBlocksMax + 1];
  RF_CHECK(hipMemcpyAsync(part, r.cost_part.p, (size_t)(blocks + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
  RF_CHECK(hipStreamSynchronize(s));
  float ms = 0.0f;
  RF_CHECK(hipEventElapsedTime(&ms, r.cost_ev[0], r.cost_ev[1]));
  r.ms_cost = ms;
  double sum = 0.0;
  for (unsigned b = 0; b < blocks; ++b) sum += part[b];
  *cost = sum;
  *root_area = part[blocks];
  static const bool print = std::getenv("SPTR_REFIT_STAGES") != nullptr;
  if (print) std::fprintf(stderr, "tree cost: %.4f ms (%u nodes, %u blocks)\n", r.ms_cost, c.num_nodes, blocks);
  return SPTR_OK;
}

}  // namespace sptr
