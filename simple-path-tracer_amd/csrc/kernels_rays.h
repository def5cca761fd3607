// kernels_rays.h — path-traced radiance for caller-supplied rays (sptr_render_rays): the producer
// k_rays_inject and the consumer k_rays_gather.  Included by kernels_wavefront.hip inside namespace sptr, after
// its launch utilities.  Between the two runs the integrator's own chain, entered at depth 0 through its
// non-primary instantiations (launch_trace / launch_shade with stream_rays): from bounce 1 on every stage reads
// its rays from the block-segmented ray stream, and a slot with throughput (1, 1, 1) and rad[p] = +0 makes a
// non-primary stage at depth 0 perform the float operations of the primary stage on the same ray.
//
// Memory traffic per path: in 32 B of ray (two 16-B loads; once per sample) and 4 B of seed; out the stream slot
// {o, rng} {d, p} {thr} (48 B) and rad[p] (16 B).  The gather reads 16 B per path and writes 12 B per ray.

// --------------------------------------------------------------------------------- k_rays_inject
// Thread j of a chunk (grid-striding) takes path p = j = s_local * nrays + i_local (ray_batch.h) and writes
// stream slot j of rs[0] in the layout k_shade writes continuation rays in: block-segmented, segment b the
// slots [b * per, b * per + cnt[b]), with the counts and the stride published in w.segN, which is what
// k_trace(d) / k_trace_dyn(d) / k_tail(d) scan.  The segments here are simply consecutive runs of `per` paths,
// so compacted index = slot = path id.  It also leaves prepared what a batch's k_accum leaves prepared for the
// next depth-0 trace: the per-XCD trace-queue words and the straggler counts, zeroed.
struct RayInjectView {
  const float4* rays;     // two per ray: o.xyz d.x | d.yz - -
  const uint32_t* seeds;  // per ray, or null
  RayChunk ck;
  uint32_t samples;       // of the call (ray_rng's rule)
  uint32_t frame_index;
  uint32_t normalize;     // SPTR_RAYS_NORMALIZE
  uint32_t nseg, per;     // segments published, paths per segment
};

__global__ void __launch_bounds__(kBlock) k_rays_inject(RayInjectView v, WaveView w) {
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
  for (uint32_t j = t0; j < np; j += grid_threads()) {
    const uint32_t sl = j / v.ck.nrays, il = j - sl * v.ck.nrays;
    const uint32_t i = v.ck.ray0 + il;
    const float4 a = v.rays[2 * (size_t)i], b = v.rays[2 * (size_t)i + 1];
    vec3 d = v3(a.w, b.x, b.y);
    if (v.normalize) d = safe_normalize(d);
    const uint32_t rng = ray_rng(v.seeds != nullptr, v.samples, v.seeds ? v.seeds[i] : 0u, i, v.frame_index, v.ck.s0 + sl);
    rs.o[j] = make_float4(a.x, a.y, a.z, __uint_as_float(rng));
    rs.d[j] = f4(d, __uint_as_float(j));
    rs.thr[j] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(0u));
    w.rad[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// --------------------------------------------------------------------------------- k_rays_gather
// One thread per ray of the chunk (grid-striding): the ray's samples summed in order, one add each, the adds
// k_accum makes — from +0, or from the ray's carried sum when the chunk continues a split sample range — and
// then stored, added to the caller's three floats (SPTR_RAYS_ACCUMULATE), or carried to the ray's next chunk.
// Block 0 folds the per-block query tallies of the chunk into the call's own totals (w.tot is the call's block,
// not the render totals) and zeroes them and the work words, as k_accum does for a batch.
struct RayGatherView {
  RayChunk ck;
  uint32_t samples;     // of the call: the chunk ends the ray's samples when s0 + ns == samples
  uint32_t accumulate;  // SPTR_RAYS_ACCUMULATE
  float* radiance;      // n x 3, the caller's
  float4* carry;        // per ray of a chunk with a split sample range: the running sum
};

__global__ void __launch_bounds__(kBlock) k_rays_gather(RayGatherView v, WaveView w) {
  const bool first = v.ck.s0 == 0u, last = v.ck.s0 + v.ck.ns == v.samples;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.ck.nrays; i += grid_threads()) {
    vec3 a = first ? v3(0.0f, 0.0f, 0.0f) : xyz(v.carry[i]);
    for (uint32_t s = 0; s < v.ck.ns; ++s) a = a + xyz(w.rad[(size_t)s * v.ck.nrays + i]);
    if (last) {
      float* o = v.radiance + (size_t)(v.ck.ray0 + i) * 3;  // (scalar accesses: the output has no alignment rule)
      if (v.accumulate) a = v3(o[0] + a.x, o[1] + a.y, o[2] + a.z);
      o[0] = a.x;
      o[1] = a.y;
      o[2] = a.z;
    } else {
      v.carry[i] = f4(a, 0.0f);
    }
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

// segments of a chunk of np paths and the paths per segment: nseg * per >= np, nseg <= kMaxSegs
static void ray_segments(uint32_t np, uint32_t& nseg, uint32_t& per) {
  nseg = grid_for(np);
  per = (uint32_t)(((uint64_t)np + (uint64_t)nseg * kBlock - 1) / ((uint64_t)nseg * kBlock)) * kBlock;
}

unsigned launch_rays_inject(const RayBatchView& b, const RayChunk& ck, const WaveView& w, hipStream_t s) {
  RayInjectView v{};
  v.rays = b.rays;
  v.seeds = b.seeds;
  v.ck = ck;
  v.samples = b.samples;
  v.frame_index = b.frame_index;
  v.normalize = b.normalize;
  ray_segments(ck.nrays * ck.ns, v.nseg, v.per);
  hipLaunchKernelGGL(k_rays_inject, dim3(v.nseg), dim3(kBlock), 0, s, v, w);
  return v.nseg;
}

void launch_rays_gather(const RayBatchView& b, const RayChunk& ck, const WaveView& w, hipStream_t s) {
  RayGatherView v{};
  v.ck = ck;
  v.samples = b.samples;
  v.accumulate = b.accumulate;
  v.radiance = b.radiance;
  v.carry = b.carry;
  hipLaunchKernelGGL(k_rays_gather, dim3(grid_for(ck.nrays)), dim3(kBlock), 0, s, v, w);
}
