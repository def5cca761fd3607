// kernels_denoise.h — first-hit AOVs (k_aov) and the edge-avoiding a-trous denoiser (k_dn_mean, k_atrous,
// k_dn_resolve) of sptr_set_denoise / sptr_read_aov.  Included by kernels_wavefront.hip inside namespace
// sptr, after its traversal, shading and resolve helpers, which these kernels share (k_aov walks the BVH
// exactly as k_pathtracer does; k_dn_mean and k_dn_resolve take the resolve's own first and last steps).
//
// All four kernels work in image space (pixel i = y * W + x), not in a shard's tile order: the filter
// reads neighbours up to 2 * 2^4 pixels away.  Arithmetic rule (DESIGN.md "Denoiser"): + - x, IEEE
// division, max and compares only, no contraction, so tests/denoise_ref.py restates the filter bit for
// bit in numpy float32.
// k_dn_reproject (sptr_set_denoise_history, DESIGN.md "Temporal reprojection") integrates an earlier pass's
// image into k_dn_mean's output under the same rule, with sqrtf and floorf besides (tests/temporal_ref.py);
// k_dn_reproject<true> (sptr_set_history_motion, DESIGN.md "Motion vectors") does so through the geometry that
// pass saw (tests/motion_ref.py).

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
    float bu = 0.0f, bv = 0.0f;
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
        if (a.ruv) {  // as k_rayquery: tri_hit4's U, V and den for this triangle
          const float4 ta = sv.tris[3 * idx + 0], tb = sv.tris[3 * idx + 1];
          const vec3 v0 = v3(ta.x, ta.y, ta.z), e1 = v3(ta.w, tb.x, tb.y), e2 = v3(tb.z, tb.w, c.x);
          const vec3 R = e_cross(v0 - f.cam_pos, d);
          const float den = e_dot(ng, d);
          const float aden = fabsf(den);
          bu = xorsign(e_dot(R, e2), den) / aden;
          bv = xorsign(e_dot(R, e1), den) / aden;
        }
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
    if (a.ruv) a.ruv[i] = make_float4(__uint_as_float(ref), bu, bv, 0.0f);
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
// kPerPixel (history on, k_dn_reproject ran): the colour image's w holds the pixel's effective frame count
// n_eff and S2 holds sigma_c 2^-i, so that S = S2 / n_eff(p) for the centre pixel; w rides through.
constexpr int kDnTileW = 32, kDnTileH = kBlock / kDnTileW;
template <bool kPerPixel>
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
  if constexpr (kPerPixel) {
    const float S = S2 / cp.w;
    S2 = S * S;
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
  cout[p] = f4(sum / wsum, kPerPixel ? cp.w : 0.0f);
}

// --------------------------------------------------------------------------------- temporal reprojection
// One pixel of the history integration: the first hit's world position, projected into the
// carry's camera, takes that pass's integrated colour t_0' and history length m' through the four bilinear
// taps that show the same surface, and mixes them into this pass's mean c_0 = r.c0:
//   t_0 = (n c_0 + m h) / (n + m), m' = n + m.
// A miss, a mean that is not finite, or no acceptable tap: t_0 = c_0 bit-unchanged (m' = n, or 0 where the
// filter passes the pixel through).  32 x 8 pixel blocks as k_atrous; no LDS; every tap is bounds-checked
// before its loads.  Pixels that took history are counted with one ballot and one atomic per wave.
// kMotion (sptr_set_history_motion): the carry saw the geometry of the snapshot.  The surface
// point is carried there (a triangle's through its barycentrics and the snapshot's record, a sphere's through
// its unit offset from the centre), that point is projected, its distance and the snapshot's normal there
// take the place of dist and N_p in the taps' weights, and the offset of the projection from the pixel is
// written out.  A reference beyond the snapshot's slots takes no history; no snapshot load comes before that check.
template <bool kMotion>
__global__ void __launch_bounds__(kBlock) k_dn_reproject(DenoiseView v, FrameView f, ReprojView r) {
  const int x = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x % kDnTileW);
  const int y = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  bool took = false;
  if (x < v.W && y < v.H) {
    const uint32_t p = (uint32_t)y * (uint32_t)v.W + (uint32_t)x;
    const float4 c0 = r.c0[p];
    const float4 np = v.nz[p];
    const float nf = float(v.n);
    float4 out = f4(xyz(c0), 0.0f);
    float2 mv = make_float2(__uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u));
    if (!(np.w < 0.0f) && dn_finite(c0)) {
      out.w = nf;
      if (r.hist_prev) {
        const ImageDiv idiv = image_div(f);
        const vec3 d = camera_dir(f, div_nrm(float(x) + 0.5f, idiv.w), div_nrm(float(y) + 0.5f, idiv.h));  // as k_aov
        vec3 P = f.cam_pos + np.w * d;
        vec3 nrm = xyz(np);
        bool known = true;
        if constexpr (kMotion) {
          const float4 ru = r.ruv[p];
          const uint32_t ref = __float_as_uint(ru.x), slot = ref & kIndexMask;
          if (ref & kSphereBit) {
            known = slot < r.num_sph;
            if (known) {
              const float4 c = r.sph[slot], cp = r.sph_prev[slot];
              const vec3 g = v3((P.x - c.x) / c.w, (P.y - c.y) / c.w, (P.z - c.z) / c.w);
              P = v3(cp.x + cp.w * g.x, cp.y + cp.w * g.y, cp.z + cp.w * g.z);
              nrm = safe_normalize(g);
            }
          } else {
            known = slot < r.num_tris;
            if (known) {
              const float4 ta = r.tris_prev[3 * slot + 0], tb = r.tris_prev[3 * slot + 1], tc = r.tris_prev[3 * slot + 2];
              const vec3 v0 = v3(ta.x, ta.y, ta.z), e1 = v3(ta.w, tb.x, tb.y), e2 = v3(tb.z, tb.w, tc.x);
              P = (v0 - ru.y * e1) + ru.z * e2;  // e1 = v0 - v1
              nrm = safe_normalize(v3(tc.y, tc.z, tc.w));
            }
          }
        }
        const vec3 vv = P - r.pos;
        if constexpr (kMotion) {
          if (dot(nrm, vv) > 0.0f) nrm = -nrm;
        }
        const float zf = dot(vv, r.fw);
        const float nx = dot(vv, r.rt) / (zf * r.hw);
        const float ny = dot(vv, r.up) / (zf * r.hh);
        const float fx = (nx * 0.5f + 0.5f) * float(v.W) - 0.5f;
        const float fy = (0.5f - ny * 0.5f) * float(v.H) - 0.5f;
        if constexpr (kMotion) {
          if (known) mv = make_float2(fx - float(x), fy - float(y));
        }
        // (written so that a NaN or an infinity fails: no conversion to int and no load before it)
        if (known && zf > 0.0f && fx > -1.0f && fx < float(v.W) && fy > -1.0f && fy < float(v.H)) {
          const float x0f = floorf(fx), y0f = floorf(fy);
          const float a = fx - x0f, b = fy - y0f;
          const int x0 = (int)x0f, y0 = (int)y0f;
          const float dist = sqrtf(dot(vv, vv));
          const uint32_t gp = r.ids[p].x;
          float ws = 0.0f, ms = 0.0f;
          vec3 hs = v3(0.0f, 0.0f, 0.0f);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int qy = y0 + j;
            const float wy = j ? b : 1.0f - b;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              const int qx = x0 + i;
              if (qx < 0 || qx >= v.W || qy < 0 || qy >= v.H) continue;
              const uint32_t q = (uint32_t)qy * (uint32_t)v.W + (uint32_t)qx;
              const float4 hq = r.hist_prev[q];
              const float4 nq = r.nz_prev[q];
              if (nq.w < 0.0f || !dn_finite(hq) || r.ids_prev[q].x != gp) continue;
              float wn = fmax_g(0.0f, dot(nrm, xyz(nq)));
              for (uint32_t k = 0; k < v.normal_log2; ++k) wn = wn * wn;
              const float e = fabsf(dist - nq.w) / (v.sigma_z * fmax_g(dist, nq.w));
              const float wz = 1.0f / (1.0f + e * e);
              if (!(wn * wz >= 0.5f)) continue;
              const float w = (i ? a : 1.0f - a) * wy;
              ws = ws + w;
              hs = hs + w * xyz(hq);
              ms = ms + w * hq.w;
            }
          }
          if (ws > 0.0f) {
            vec3 h = hs / ws;
            if (r.clip > 0.0f) {
              // the view changed, and with it whatever the surface reflects: h is clipped to mu -+ clip sd of
              // c_0 over the 3 x 3 neighbours on the same geometry (the centre always counts)
              vec3 s1 = v3(0.0f, 0.0f, 0.0f), s2 = v3(0.0f, 0.0f, 0.0f);
              float cnt = 0.0f;
#pragma unroll
              for (int dy = -1; dy <= 1; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= v.H) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                  const int qx = x + dx;
                  if (qx < 0 || qx >= v.W) continue;
                  const uint32_t q = (uint32_t)qy * (uint32_t)v.W + (uint32_t)qx;
                  const float4 cq = r.c0[q];
                  if (v.nz[q].w < 0.0f || !dn_finite(cq) || r.ids[q].x != gp) continue;
                  s1 = s1 + xyz(cq);
                  s2 = s2 + xyz(cq) * xyz(cq);
                  cnt = cnt + 1.0f;
                }
              }
              const vec3 mu = s1 / cnt;
              const vec3 var = s2 / cnt - mu * mu;
              // (max(0, var) written so that a NaN, from sums that overflowed, gives 0)
              const vec3 sd = v3(sqrtf(fmax_g(0.0f, var.x)), sqrtf(fmax_g(0.0f, var.y)), sqrtf(fmax_g(0.0f, var.z)));
              const vec3 lo = mu - r.clip * sd, hi = mu + r.clip * sd;
              h = v3(fmin_g(fmax_g(h.x, lo.x), hi.x), fmin_g(fmax_g(h.y, lo.y), hi.y), fmin_g(fmax_g(h.z, lo.z), hi.z));
            }
            float m = ms / ws;
            m = m < r.max_history ? m : r.max_history;
            if (m > 0.0f) {
              const float neff = nf + m;
              out = f4((nf * xyz(c0) + m * h) / neff, neff);
              took = true;
            }
          }
        }
      }
    }
    r.hist[p] = out;
    if constexpr (kMotion) r.motion[p] = mv;
  }
  const unsigned long long bal = __ballot(took);
  if (bal != 0ull && lane_id() == 0u) atomicAdd(r.count, (uint32_t)__popcll(bal));
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
  hipLaunchKernelGGL(k_atrous<false>, grid, dim3(kBlock), 0, s, v, cin, cout, step, S2);
}
void launch_atrous_history(const DenoiseView& v, const float4* cin, float4* cout, int step, float Si, hipStream_t s) {
  const dim3 grid((unsigned)((v.W + kDnTileW - 1) / kDnTileW), (unsigned)((v.H + kDnTileH - 1) / kDnTileH));
  hipLaunchKernelGGL(k_atrous<true>, grid, dim3(kBlock), 0, s, v, cin, cout, step, Si);
}
void launch_dn_reproject(const DenoiseView& v, const FrameView& f, const ReprojView& r, hipStream_t s) {
  const dim3 grid((unsigned)((v.W + kDnTileW - 1) / kDnTileW), (unsigned)((v.H + kDnTileH - 1) / kDnTileH));
  hipLaunchKernelGGL(k_dn_reproject<false>, grid, dim3(kBlock), 0, s, v, f, r);
}
void launch_dn_reproject_motion(const DenoiseView& v, const FrameView& f, const ReprojView& r, hipStream_t s) {
  const dim3 grid((unsigned)((v.W + kDnTileW - 1) / kDnTileW), (unsigned)((v.H + kDnTileH - 1) / kDnTileH));
  hipLaunchKernelGGL(k_dn_reproject<true>, grid, dim3(kBlock), 0, s, v, f, r);
}
void launch_dn_resolve(const DenoiseView& v, const float4* c, uint8_t* image, hipStream_t s) {
  hipLaunchKernelGGL(k_dn_resolve, dim3(grid_for((uint64_t)v.W * v.H)), dim3(kBlock), 0, s, v, c, image);
}
