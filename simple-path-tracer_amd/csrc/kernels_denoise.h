// kernels_denoise.h — first-hit AOVs (k_aov) and the edge-avoiding a-trous denoiser (k_dn_mean, k_atrous,
// k_dn_resolve) of sptr_set_denoise / sptr_read_aov.  Included by kernels_wavefront.hip inside namespace
// sptr, after its traversal, shading and resolve helpers, which these kernels share (k_aov walks the BVH
// exactly as k_pathtracer does; k_dn_mean and k_dn_resolve take the resolve's own first and last steps).
//
// All four kernels work in image space (pixel i = y * W + x), not in a shard's tile order: the filter
// reads neighbours up to 2 * 2^4 pixels away.  Arithmetic rule (DESIGN.md "Denoiser"): + - x, IEEE
// division, max and compares only, no contraction, so tests/denoise_ref.py restates the filter bit for
// bit in numpy float32.

// --------------------------------------------------------------------------------- k_aov
// One closest-hit query per image pixel along the pixel-centre ray.
template <bool kLds, bool kW4>
__global__ void __launch_bounds__(kBlock, SPTR_PT_WAVES) k_aov(SceneView sv, FrameView f, AovView a) {
  __shared__ KernelStack<kLds> s_stack;
  extern __shared__ float4 lds[];
  const Staged sc = stage_scene<kLds>(sv, lds);
  __syncthreads();
  const ImageDiv idiv = image_div(f);
  Visits vc;
  const uint32_t N = (uint32_t)f.W * (uint32_t)f.H;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += grid_threads()) {
    const uint32_t yu = i / (uint32_t)f.W;
    const int x = (int)(i - yu * (uint32_t)f.W), y = (int)yu;
    const vec3 d = camera_dir(f, div_nrm(float(x) + 0.5f, idiv.w), div_nrm(float(y) + 0.5f, idiv.h));
    const Ray r = make_ray(f.cam_pos, d);
    float t = __builtin_huge_valf();
    uint32_t ref = kNoHit;
    const bool hit = traverse_w<kW4, false, false>(sc, sv, r, 0.0f, t, ref, vc, s_stack);
    float4 nz = make_float4(0.0f, 0.0f, 0.0f, -1.0f), al = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint2 id = make_uint2(kNoHit, kNoHit);
    if (hit) {
      const uint32_t idx = ref & kIndexMask;
      vec3 ng;
      if (ref & kSphereBit) {  // as surface_at
        const float4 c = sv.sph[idx];
        const vec3 P = f.cam_pos + t * d;
        ng = v3((P.x - c.x) / c.w, (P.y - c.y) / c.w, (P.z - c.z) / c.w);
        id = make_uint2(sv.sph_geom[idx], 0u);
      } else {
        const float4 c = sv.tris[3 * idx + 2];
        ng = v3(c.y, c.z, c.w);
        const uint32_t g = sv.tri_geom[idx];
        id = make_uint2(g, a.tri_orig[idx] - a.geom_first[g]);
      }
      vec3 n = safe_normalize(ng);
      if (dot(n, d) > 0.0f) n = -n;
      nz = f4(n, t);
      const DevMaterial& m = a.mats[a.geom_mat[id.x]];
      al = make_float4(m.albedo[0], m.albedo[1], m.albedo[2], 0.0f);
    }
    a.nz[i] = nz;
    a.albedo[i] = al;
    a.ids[i] = id;
  }
  if (__ballot(vc.stack_overflow != 0u) && lane_id() == 0u) *a.stack_overflow = 1u;
}

void launch_aov(const SceneView& sv, const FrameView& f, const AovView& a, hipStream_t s) {
  const bool L = sv.lds_bytes != 0;
  const unsigned lb = L ? sv.lds_bytes : 16u;
  const unsigned need = (unsigned)(((uint64_t)f.W * f.H + kBlock - 1) / kBlock);
  dispatch(
      [&](auto fl) -> unsigned {
        return [&]<bool Lc, bool Wc>(Flags<Lc, Wc>) {
          const unsigned g = std::max(1u, std::min<unsigned>(resident_grid((const void*)&k_aov<Lc, Wc>, lb), need));
          hipLaunchKernelGGL((k_aov<Lc, Wc>), dim3(g), dim3(kBlock), lb, s, sv, f, a);
          return g;
        }(fl);
      },
      Flags<>{}, L, sv.width == (uint32_t)kWide);
}

// --------------------------------------------------------------------------------- the filter
__device__ __forceinline__ bool dn_finite(float4 c) {
  const float big = 3.402823466e+38f;  // FLT_MAX: false for an infinity or a NaN
  return fabsf(c.x) <= big && fabsf(c.y) <= big && fabsf(c.z) <= big;
}

// c_0: the mean the resolve computes from the accumulation (resolve_rgba's first step), gathered from
// the tile-packed sums of the call's one or two pixel lanes (lane r holds shard r of G).
__global__ void __launch_bounds__(kBlock) k_dn_mean(DenoiseView v, const float4* accum0, const float4* accum1, int G,
                                                    float4* out) {
  const uint32_t N = (uint32_t)v.W * (uint32_t)v.H;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += grid_threads()) {
    const uint32_t yu = i / (uint32_t)v.W;
    uint32_t r, l;
    pixel_shard(v.W, G, (int)(i - yu * (uint32_t)v.W), (int)yu, r, l);
    const vec3 c = xyz((r ? accum1 : accum0)[l]) / float(v.n);
    out[i] = f4(c, 0.0f);
  }
}

// One a-trous iteration with step s: 5x5 taps s pixels apart, summed in (dy, dx) row-major order.
// The block's pixels form a 32 x 8 patch (a wave covers two rows), so that a tap's loads are row
// segments of 512 B and vertically neighbouring taps of a block share cache lines.
// The taps read global memory: the working set (133 MB at 1080p) stays in L2 / MALL.  (Staging the patch and
// its 2 s halo in LDS for s = 1, 2 measured slower)
constexpr int kDnTileW = 32, kDnTileH = kBlock / kDnTileW;
__global__ void __launch_bounds__(kBlock) k_atrous(DenoiseView v, const float4* __restrict__ cin, float4* __restrict__ cout, int s,
                                                   float S2) {
  const int x = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x % kDnTileW);
  const int y = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  if (x >= v.W || y >= v.H) return;
  const uint32_t p = (uint32_t)y * (uint32_t)v.W + (uint32_t)x;
  const float4 cp = cin[p];
  const float4 np = v.nz[p];
  if (np.w < 0.0f || !dn_finite(cp)) {  // the environment, or a mean that is not finite: passed through
    cout[p] = cp;
    return;
  }
  const float4 ap = v.albedo[p];
  const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  vec3 sum = v3(0.0f, 0.0f, 0.0f);
  float wsum = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + dy * s;
    if (qy < 0 || qy >= v.H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + dx * s;
      if (qx < 0 || qx >= v.W) continue;
      const uint32_t q = (uint32_t)qy * (uint32_t)v.W + (uint32_t)qx;
      const float4 cq = cin[q];
      const float4 nq = v.nz[q];
      if (nq.w < 0.0f || !dn_finite(cq)) continue;  // w = 0
      const float4 aq = v.albedo[q];
      float wn = fmax_g(0.0f, dot(xyz(np), xyz(nq)));
      for (uint32_t k = 0; k < v.normal_log2; ++k) wn = wn * wn;
      const float e = fabsf(np.w - nq.w) / (v.sigma_z * fmax_g(np.w, nq.w));
      const float wz = 1.0f / (1.0f + e * e);
      const vec3 da = xyz(ap) - xyz(aq);
      const float wa = 1.0f / (1.0f + dot(da, da) / v.sigma_a2);
      const vec3 dc = xyz(cp) - xyz(cq);
      const float wc = 1.0f / (1.0f + dot(dc, dc) / S2);
      const float w = h[dy + 2] * h[dx + 2] * wn * wz * wa * wc;
      sum = sum + w * xyz(cq);
      wsum = wsum + w;
    }
  }
  cout[p] = f4(sum / wsum, 0.0f);
}

// The resolve's last steps (ACES, gamma, 8 bit) on the filtered mean: resolve_rgba with a count of 1.
__global__ void __launch_bounds__(kBlock) k_dn_resolve(DenoiseView v, const float4* c, uint8_t* image) {
  const uint32_t N = (uint32_t)v.W * (uint32_t)v.H;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += grid_threads()) {
    const uint32_t px = resolve_rgba(xyz(c[i]), 1u);
    uint8_t* o = image + (size_t)i * 3;
    o[0] = (uint8_t)(px & 0xFF);
    o[1] = (uint8_t)((px >> 8) & 0xFF);
    o[2] = (uint8_t)((px >> 16) & 0xFF);
  }
}

void launch_dn_mean(const DenoiseView& v, const float4* accum0, const float4* accum1, int G, float4* out, hipStream_t s) {
  hipLaunchKernelGGL(k_dn_mean, dim3(grid_for((uint64_t)v.W * v.H)), dim3(kBlock), 0, s, v, accum0, accum1, G, out);
}
void launch_atrous(const DenoiseView& v, const float4* cin, float4* cout, int step, float S2, hipStream_t s) {
  const dim3 grid((unsigned)((v.W + kDnTileW - 1) / kDnTileW), (unsigned)((v.H + kDnTileH - 1) / kDnTileH));
  hipLaunchKernelGGL(k_atrous, grid, dim3(kBlock), 0, s, v, cin, cout, step, S2);
}
void launch_dn_resolve(const DenoiseView& v, const float4* c, uint8_t* image, hipStream_t s) {
  hipLaunchKernelGGL(k_dn_resolve, dim3(grid_for((uint64_t)v.W * v.H)), dim3(kBlock), 0, s, v, c, image);
}
