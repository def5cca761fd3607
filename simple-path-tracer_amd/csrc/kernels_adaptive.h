// kernels_adaptive.h — adaptive sampling (sptr_render_adaptive): the selection of the active
// pixels (k_adapt_count, k_adapt_scatter), the producer k_adapt_inject and the consumer k_adapt_gather around the
// chain's depth-0 entry (as kernels_rays.h), and the resolve by each pixel's own count.  Included by
// kernels_wavefront.hip inside namespace sptr, after kernels_rays.h.  The rule itself is adaptive_rule.h's.
//
// State per local pixel l: S = f.accum[l].xyz, E = a.E[l].xyz, n = a.n[l] (20 B beside the accumulation).
// Memory traffic: a selection reads 36 B per pixel twice (count, scatter) and writes 4 B per listed pixel; the
// producer reads 8 B per path and writes what k_rays_inject writes (64 B); the consumer reads 16 B per path and
// 40 B per entry and writes 36 B per entry.

// --------------------------------------------------------------------------------- selection
// A fixed grid of nb <= kMaxSegs blocks, block b owning the contiguous local pixels [b * per, (b + 1) * per)
// (per a multiple of kBlock).  k_adapt_count leaves per block, in a.bstat[b * kAdaptStat ..]: the pixels of the
// group (active, key == K), the active pixels, the smallest active key below and above K, and the smallest and
// largest n of its valid pixels.  k_adapt_scatter, same grid: every block sums the group counts of the blocks
// before it, then walks its range again in rounds of kBlock pixels and writes the group's pixels to the list in
// ascending local index: ballot and popcount inside a wave, the wave totals in LDS, a running base per block.
// Block 0 also folds the per-block words into a.result, which the host reads.  No global atomics, and no block
// waits for another: the two launches are ordered by the stream.
constexpr uint32_t kAdaptStat = kAdaptiveStatWords;  // words per block in bstat
constexpr uint32_t kAdaptGuard = kAdaptiveGuardWords;
constexpr uint32_t kAdaptGuardWord = kAdaptiveGuardValue;
static_assert(4u * kAdaptGuard == 64u, "k_adapt_scatter checks the four guard runs with one wave");

struct AdaptView {
  float4* E;          // per local pixel: the even samples' sum
  uint32_t* n;        // per local pixel: samples taken
  uint32_t* list;     // the group's local pixels, ascending
  uint32_t* bstat;    // [kMaxSegs * kAdaptStat]
  uint32_t* result;   // [kAdaptiveResWords]
  const uint32_t* guards;  // the start of the state block: 4 guard runs at guard_off[]
  uint32_t guard_off[4];   // in words
  AdaptiveRule rule;
  uint32_t key;       // K of this selection
  uint32_t per;       // pixels per selection block
};

// the key of local pixel l if it is active, 0 otherwise (no active pixel has key 0); nv: its n if it is valid
__device__ __forceinline__ uint32_t adapt_pixel_key(const AdaptView& a, const FrameView& f, uint32_t l, bool& valid,
                                                    uint32_t& nv) {
  int x, y;
  valid = local_pixel(f, l, x, y);
  nv = 0u;
  if (!valid) return 0u;
  nv = a.n[l];
  if (nv >= a.rule.max_samples) return 0u;
  if (nv >= a.rule.min_samples && !adaptive_active(a.rule, xyz(f.accum[l]), xyz(a.E[l]), nv)) return 0u;
  return adaptive_key(a.rule, nv);
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor(v, off);
  return v;
}
// the six statistics of a block's threads, reduced into s[0..5] (sum, sum, min, min, min, max); barriers inside
__device__ __forceinline__ void adapt_block_reduce(uint32_t v[6], uint32_t (*s_w)[6]) {
  v[0] = wave_sum(v[0]);
  v[1] = wave_sum(v[1]);
  v[2] = wave_min(v[2]);
  v[3] = wave_min(v[3]);
  v[4] = wave_min(v[4]);
  v[5] = wave_max(v[5]);
  const uint32_t wv = threadIdx.x >> 6;
  if (lane_id() == 0u)
    for (int k = 0; k < 6; ++k) s_w[wv][k] = v[k];
  __syncthreads();
  for (uint32_t o = 0; o < kBlock / 64; ++o) {
    if (o == wv) continue;
    v[0] += s_w[o][0];
    v[1] += s_w[o][1];
    v[2] = min(v[2], s_w[o][2]);
    v[3] = min(v[3], s_w[o][3]);
    v[4] = min(v[4], s_w[o][4]);
    v[5] = max(v[5], s_w[o][5]);
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kBlock) k_adapt_count(AdaptView a, FrameView f) {
  __shared__ uint32_t s_w[kBlock / 64][6];
  const uint32_t lo = blockIdx.x * a.per, hi = min(f.P, lo + a.per);
  uint32_t v[6] = {0u, 0u, ~0u, ~0u, ~0u, 0u};
  for (uint32_t l = lo + threadIdx.x; l < hi; l += kBlock) {
    bool valid;
    uint32_t nv;
    const uint32_t key = adapt_pixel_key(a, f, l, valid, nv);
    if (valid) {
      v[4] = min(v[4], nv);
      v[5] = max(v[5], nv);
    }
    if (key) {
      ++v[1];
      if (key == a.key) ++v[0];
      else if (key < a.key) v[2] = min(v[2], key);
      else v[3] = min(v[3], key);
    }
  }
  adapt_block_reduce(v, s_w);
  if (threadIdx.x == 0u) {
    uint32_t* t = a.bstat + blockIdx.x * kAdaptStat;
    for (int k = 0; k < 6; ++k) t[k] = v[k];
  }
}

__global__ void __launch_bounds__(kBlock) k_adapt_scatter(AdaptView a, FrameView f) {
  __shared__ uint32_t s_w[kBlock / 64][6];
  __shared__ uint32_t s_cnt[kBlock / 64];
  // the group's pixels in the blocks before this one; block 0: every block's words, folded
  uint32_t v[6] = {0u, 0u, ~0u, ~0u, ~0u, 0u};
  const uint32_t nb = blockIdx.x == 0u ? gridDim.x : blockIdx.x;
  for (uint32_t b = threadIdx.x; b < nb; b += kBlock) {
    const uint32_t* t = a.bstat + b * kAdaptStat;
    v[0] += t[0];
    if (blockIdx.x == 0u) {
      v[1] += t[1];
      v[2] = min(v[2], t[2]);
      v[3] = min(v[3], t[3]);
      v[4] = min(v[4], t[4]);
      v[5] = max(v[5], t[5]);
    }
  }
  adapt_block_reduce(v, s_w);
  uint32_t base = v[0];
  if (blockIdx.x == 0u) {
    base = 0u;
    if (threadIdx.x == 0u)
      for (int k = 0; k < 6; ++k) a.result[k] = v[k];
    // the guard words around E, n and the list: any that changed (a write out of bounds) is reported
    uint32_t bad = 0u;
    if (threadIdx.x < 4u * kAdaptGuard)
      bad = a.guards[a.guard_off[threadIdx.x / kAdaptGuard] + threadIdx.x % kAdaptGuard] != kAdaptGuardWord ? 1u : 0u;
    if (threadIdx.x < 64u) {
      const uint32_t any = __ballot(bad != 0u) != 0ull ? 1u : 0u;
      if (threadIdx.x == 0u) a.result[kAdaptiveResGuardBad] = any;
    }
  }
  const uint32_t lo = blockIdx.x * a.per, hi = min(f.P, lo + a.per);
  const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
  for (uint32_t r = lo; r < hi; r += kBlock) {  // (uniform over the block: barriers inside)
    const uint32_t l = r + threadIdx.x;
    bool valid = false;
    uint32_t nv;
    const bool in = l < hi && adapt_pixel_key(a, f, l, valid, nv) == a.key;
    const unsigned long long m = __ballot(in);
    if (lane == 0u) s_cnt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), tot = 0u;
    for (uint32_t o = 0; o < kBlock / 64; ++o) {
      if (o < wv) off += s_cnt[o];
      tot += s_cnt[o];
    }
    if (in && off < f.P) a.list[off] = l;  // (off < the group's size <= P: the bound is a guard)
    base += tot;
    __syncthreads();
  }
}

// --------------------------------------------------------------------------------- k_adapt_inject
// k_rays_inject for list entries: thread j of a chunk (grid-striding) takes path j = s * nrays + entry (adaptive_
// path) and writes the camera ray of sample n[l] + 1 + s of the entry's pixel l — primary_at for accumulation
// index n[l] + 1 + s + seed_offset, origin the camera position, throughput 1, rad = +0 — into stream slot j of
// rs[0], with the segment counts and the prepared work words exactly as k_rays_inject leaves them.
struct AdaptInjectView {
  const uint32_t* list;
  const uint32_t* n;
  RayChunk ck;
  uint32_t seed_offset;
  uint32_t nseg, per;  // segments published, paths per segment
};

__global__ void __launch_bounds__(kBlock) k_adapt_inject(AdaptInjectView v, FrameView f, WaveView w) {
  const uint32_t np = v.ck.nrays * v.ck.ns;
  const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 < v.nseg) {
    const uint32_t lo = t0 * v.per;
    w.segN.cnt[t0] = lo < np ? min(v.per, np - lo) : 0u;
    if (t0 == 0u) *w.segN.per = v.per;
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x < kXcds) w.work[kWorkTraceQueue + threadIdx.x * 32u] = 0u;
    if (threadIdx.x >= 128 && threadIdx.x < 128 + kStragBounces) w.work[kWorkStrag + (threadIdx.x - 128) * 32u] = 0u;
  }
  const RayStream rs = w.rs[0];
  const ImageDiv dv = image_div(f);
  for (uint32_t j = t0; j < np; j += grid_threads()) {
    uint32_t e, sl;
    adaptive_path(v.ck, j, e, sl);
    const uint32_t l = v.list[e];
    int x, y;
    (void)local_pixel(f, l, x, y);  // (a listed pixel is valid)
    Primary pr;
    primary_at(f, dv, x, y, (uint32_t)(y * f.W + x), v.n[l] + 1u + sl + v.seed_offset, pr);
    rs.o[j] = f4(f.cam_pos, __uint_as_float(pr.rng));
    rs.d[j] = f4(pr.d, __uint_as_float(j));
    rs.thr[j] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(0u));
    w.rad[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// --------------------------------------------------------------------------------- k_adapt_gather
// One thread per list entry of the chunk (grid-striding): the chunk's samples of the pixel added to S in index
// order, one add each, the ones with an even index to E as well, and n advanced by the chunk's samples — the
// state is the carry of a split sample range.  Block 0 folds the query tallies as k_rays_gather does.
struct AdaptGatherView {
  const uint32_t* list;
  float4* E;
  uint32_t* n;
  RayChunk ck;
};

__global__ void __launch_bounds__(kBlock) k_adapt_gather(AdaptGatherView v, FrameView f, WaveView w) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.ck.nrays; i += grid_threads()) {
    const uint32_t l = v.list[v.ck.ray0 + i];
    const uint32_t n0 = v.n[l];
    vec3 S = xyz(f.accum[l]), E = xyz(v.E[l]);
    for (uint32_t s = 0; s < v.ck.ns; ++s) {
      const vec3 L = xyz(w.rad[(size_t)s * v.ck.nrays + i]);
      S = S + L;
      if (adaptive_even(n0 + 1u + s)) E = E + L;
    }
    f.accum[l] = f4(S, 0.0f);
    v.E[l] = f4(E, 0.0f);
    v.n[l] = n0 + v.ck.ns;
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x < kXcds) w.work[kWorkTraceQueue + threadIdx.x * 32u] = 0u;
    if (threadIdx.x >= 128 && threadIdx.x < 128 + kStragBounces) w.work[kWorkStrag + (threadIdx.x - 128) * 32u] = 0u;
    unsigned long long s = 0ull, c = 0ull;
    for (uint32_t b = threadIdx.x; b < kMaxSegs; b += kBlock) {
      s += w.bstat[b];
      c += w.bstat_closest[b];
      w.bstat[b] = 0ull;
      w.bstat_closest[b] = 0ull;
    }
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_xor(s, off);
      c += __shfl_xor(c, off);
    }
    if (lane_id() == 0u) {
      atomicAdd(&w.tot[kTotShadow], s);
      atomicAdd(&w.tot[kTotClosest], c);
      atomicAdd(&w.tot[kTotTail], c);
    }
  }
}

// --------------------------------------------------------------------------------- k_adapt_resolve
// k_resolve with each pixel's own count: resolve_rgba(S, n) into the tiles and the RGB8 image.
__global__ void __launch_bounds__(kBlock) k_adapt_resolve(FrameView f, const uint32_t* n, uint32_t* tiles, uint8_t* image) {
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < f.P; l += grid_threads()) {
    int x, y;
    const bool valid = local_pixel(f, l, x, y);
    const uint32_t c = valid ? n[l] : 0u;
    const uint32_t px = c ? resolve_rgba(xyz(f.accum[l]), c) : 0u;
    tiles[l] = px;
    if (valid && image) {
      uint8_t* o = image + ((size_t)y * f.W + x) * 3;
      o[0] = (uint8_t)(px & 0xFF);
      o[1] = (uint8_t)((px >> 8) & 0xFF);
      o[2] = (uint8_t)((px >> 16) & 0xFF);
    }
  }
}

// --------------------------------------------------------------------------------- launchers
static AdaptView adapt_view(const AdaptiveBufs& b, const AdaptiveRule& rule, uint32_t key, uint32_t P, unsigned& grid) {
  AdaptView a{};
  a.E = b.E;
  a.n = b.n;
  a.list = b.list;
  a.bstat = b.bstat;
  a.result = b.result;
  a.guards = b.base;
  for (int k = 0; k < 4; ++k) a.guard_off[k] = b.guard_off[k];
  a.rule = rule;
  a.key = key;
  grid = (unsigned)std::min<uint64_t>(kMaxSegs, ((uint64_t)P + kBlock - 1) / kBlock);
  if (grid < 1u) grid = 1u;
  a.per = (uint32_t)(((uint64_t)P + (uint64_t)grid * kBlock - 1) / ((uint64_t)grid * kBlock)) * kBlock;
  return a;
}

void launch_adapt_select(const AdaptiveBufs& b, const AdaptiveRule& rule, uint32_t key, const FrameView& f, hipStream_t s) {
  unsigned grid;
  const AdaptView a = adapt_view(b, rule, key, f.P, grid);
  hipLaunchKernelGGL(k_adapt_count, dim3(grid), dim3(kBlock), 0, s, a, f);
  hipLaunchKernelGGL(k_adapt_scatter, dim3(grid), dim3(kBlock), 0, s, a, f);
}

unsigned launch_adapt_inject(const AdaptiveBufs& b, const RayChunk& ck, uint32_t seed_offset, const FrameView& f,
                             const WaveView& w, hipStream_t s) {
  AdaptInjectView v{};
  v.list = b.list;
  v.n = b.n;
  v.ck = ck;
  v.seed_offset = seed_offset;
  ray_segments(ck.nrays * ck.ns, v.nseg, v.per);
  hipLaunchKernelGGL(k_adapt_inject, dim3(v.nseg), dim3(kBlock), 0, s, v, f, w);
  return v.nseg;
}

void launch_adapt_gather(const AdaptiveBufs& b, const RayChunk& ck, const FrameView& f, const WaveView& w, hipStream_t s) {
  AdaptGatherView v{};
  v.list = b.list;
  v.E = b.E;
  v.n = b.n;
  v.ck = ck;
  hipLaunchKernelGGL(k_adapt_gather, dim3(grid_for(ck.nrays)), dim3(kBlock), 0, s, v, f, w);
}

void launch_adapt_resolve(const AdaptiveBufs& b, const FrameView& f, uint32_t* tiles, uint8_t* image, hipStream_t s) {
  hipLaunchKernelGGL(k_adapt_resolve, dim3(grid_for(f.P)), dim3(kBlock), 0, s, f, b.n, tiles, image);
}
