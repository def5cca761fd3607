// sptr_api.cpp — C ABI of libsptr_hip (include/sptr_hip.h): context, uploads, and the per-call
// wavefront schedule.  This is the replacement for OptixBackend::render's orchestration
// (src/backends/OptixBackend.cpp:1506-1850): where the reference does three blocking host round
// trips per bounce (queue counter readbacks + a LaunchParams upload), here every stage reads its
// queue length from device memory, so a whole render call is enqueued without a host sync.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "query_stage.h"
#include "sptr_internal.h"

#include <dlfcn.h>
#include <execinfo.h>
#include <csignal>
#include <ucontext.h>
#include <unistd.h>

struct sptr_ctx {
  sptr::Context c;
  // Pixel lanes (sptr_set_pixel_lanes): a second context, with its own buffers and streams, renders the
  // odd half of this context's tiles beside this one's launch chain, so that each chain's launch tails
  // run beside the other's work.  Only for scenes staged into LDS (the lane holds a copy of the scene).
  sptr_ctx* lane = nullptr;
  bool is_lane = false;
  uint32_t lanes_req = 0;   // 0: automatic, 1: one chain, 2: two lanes
  bool lane_scene = false;  // the lane context holds this context's scene
  bool split = false;       // the current accumulation runs in two lanes
  sptr::DevEvent lane_fork, lane_join;
  sptr::DevBuf tiles_full;  // with split: this context's tiles, interleaved from the two lanes'
  uint32_t full_tiles = 0;
  int full_G = 1, full_R = 0;
  // the triangle list's geomID offsets on the device, beside the scene they mirror (c.geom_first): k_aov
  // and k_rayquery derive primIDs from them (ensure_geom_first; invalidated by sptr_upload_scene)
  sptr::DevBuf geom_first;
  bool geom_first_valid = false;
  // sptr_read_rgb8_lagged: two device snapshots of the RGB8 image, alternately written; a copy stream and
  // the registered host destination (created / registered on first use)
  struct Snap {
    sptr::DevBuf buf;
    sptr::DevEvent ready;
    int W = 0, H = 0;
    bool valid = false;
  } snap[2];
  uint32_t snap_cur = 0;
  sptr::DevStream copy_stream;
  sptr::DevEvent copy_done;
  void* reg_ptr = nullptr;
  size_t reg_bytes = 0;
  // sptr_set_denoise / sptr_read_aov (the caller's context; a pixel lane holds none).  Everything is in
  // image space: the AOV planes with the key they were computed for (as the cull mask's), the filter's two
  // ping-pong colour images and the second RGB8 image the readbacks return while the denoiser is on.
  struct Denoise {
    sptr_denoise_params p{};  // iterations 0: off
    sptr::DevBuf nz, albedo, ids, flag, col[2], image;
    uint64_t aov_epoch = 0;
    sptr_camera aov_cam{};
    int aov_W = 0, aov_H = 0;
    uint32_t aov_passes = 0;
    sptr_camera last_cam{};  // the last render call's camera and size (sptr_read_aov)
    int last_W = 0, last_H = 0;
    bool ran = false;        // the last render call ran the pass: `image` and col[final] hold its result
    uint32_t final_col = 0;
    sptr::DevEvent ev[4];                                     // AOV begin / end, filter begin / end
    bool aov_timed = false, filter_timed = false;             // ... recorded by the last pass
    // sptr_set_denoise_history.  The {N, z} and id planes are double-buffered: nz / ids above
    // are side 0, nz1 / ids1 side 1 (allocated with the history images); aov_side is the side the cached
    // planes (aov_cam ...) are in, and a recomputation never writes the side the carry's planes are in.
    sptr_history_params hp{};  // max_history 0: off
    sptr::DevBuf nz1, ids1, hist[2], hcount;
    int aov_side = 0;
    struct Pass {  // a pass's history image with the planes, camera, size and state it ran for
      bool valid = false;
      int slot = 0, side = 0;
      sptr_camera cam{};
      int W = 0, H = 0;
      uint64_t epoch = 0;
      uint64_t gen = 0;  // the geometry generation it ran on
    } last, carry;  // the last pass, and the pass the current accumulation takes its history from
    bool hist_ran = false;     // the last render call ran a pass with history on
    bool hist_carried = false; // ... and that pass had a carry to read
    uint32_t hist_slot = 0;    // ... and wrote hist[hist_slot]
    sptr::DevEvent hev[2];     // k_dn_reproject begin / end
    // sptr_set_history_motion.  geom_gen counts sptr_update_geometry calls; the snapshot
    // (Context::rf.snap) holds the records of generation snap_gen.  ruv: k_aov's reference / barycentric
    // plane of the cached planes (aov_uv: it was written with them); motion: k_dn_reproject<true>'s vectors.
    bool motion_on = false;
    uint64_t geom_gen = 0, snap_gen = 0;
    bool snap_valid = false;
    sptr::DevBuf ruv, motion;
    bool aov_uv = false;
    bool motion_used = false;  // the last pass with history on took the motion path
  } dn;
  // What every query kind keeps of its last run, which may still be running on a caller's stream
  struct QueryRun {
    sptr::DevEvent ev[3];  // begin, after the sort, end
    bool issued = false;   // ev[0] and ev[2] (sorted: ev[1] too) are recorded
    bool sorted = false;
    uint32_t count = 0;
  };
  // sptr_query_rays (the caller's context; a pixel lane holds none): scratch that grows on demand (sort keys
  // and identity indices, their sorted copies, the radix sort's temporaries, the stack-overflow flag, the
  // staging of host-pointer queries), shared by every kind so that consecutive enqueued queries share a stream
  struct RayQuery {
    sptr::DevBuf keys, index, keys_sorted, order, temp, flag, stage_in, stage_out;
    QueryRun run;
  } rq;
  // sptr_query_multi_hit: the facts of its last query for sptr_multi_hit_info
  struct MultiHit {
    QueryRun run;
    uint32_t list_capacity = 0, lds_bytes = 0;
  } mh;
  // sptr_query_points: the facts of its last query for sptr_point_query_info, and the two 64-bit counters of a
  // SPTR_POINT_COUNT query (allocated by the first such query)
  struct PointQuery {
    QueryRun run;
    sptr::DevBuf counters;
    bool counted = false;
    uint32_t lds_bytes = 0;
  } pq;
  // sptr_query_signed_distance: the point query's ids when the caller takes none (scratch that grows on demand) and
  // the run of the last sign pass (never sorted: ev[0] and ev[2])
  struct SignedQuery {
    sptr::DevBuf geom, prim;
    QueryRun run;
  } sq;
  // Waits for the last query of every kind, on whichever stream it was enqueued, and returns the first error.  Whoever
  // frees or regrows what an enqueued query may still use goes through here, so a new kind adds its run to this list only.
  hipError_t wait_queries() {
    hipError_t first = hipSuccess;
    for (QueryRun* r : {&rq.run, &mh.run, &pq.run, &sq.run}) {
      const hipError_t e = r->issued ? hipEventSynchronize(r->ev[2]) : hipSuccess;
      if (first == hipSuccess) first = e;
    }
    return first;
  }
  // sptr_render_rays (the caller's context; a pixel lane holds none): the call's own totals block (WaveView::tot
  // of its launches, so that the render totals never see them), the carried sum of a ray whose sample range is
  // split, the staging of host-pointer calls, and the events of the last call: begin and end on the context's
  // stream, and the fork recorded on a caller's stream or on the pending renders' stream
  struct RayRender {
    sptr::DevBuf tot, carry, stage_rays, stage_seeds, stage_out;
    sptr::DevEvent ev[3];  // begin, end, fork
    bool issued = false;
    uint32_t chunks = 0;
  } rr;
  // sptr_render_adaptive (the caller's context; a pixel lane holds none): the state beside the accumulation, the
  // list and the selection's words in one block with guard runs (AdaptiveBufs), the call's own totals block, and
  // what a call with SPTR_ADAPTIVE_CONTINUE must find unchanged.  The state is valid while Context::last_samples
  // holds kAdaptiveMark: every render call and every new pixel layout overwrites that.
  struct Adaptive {
    sptr::DevBuf state, tot;
    sptr::AdaptiveBufs bufs{};
    uint32_t P = 0;  // the local pixels `state` is laid out for
    sptr::DevEvent ev[2];
    bool valid = false;
    sptr_camera cam{};
    int W = 0, H = 0, G = 0, R = 0;
    uint32_t max_depth = 0;
    uint64_t epoch = 0;
  } ad;
  // Waits for everything that may still use this context's resources, then lets the lane go; the members
  // free themselves after that (in reverse order of declaration: c, with its streams, last).
  ~sptr_ctx() {
    (void)hipSetDevice(c.device);
    // this context's stream before the lane goes: after an asynchronous two-lane call it may still run
    // k_interleave_tiles, which reads the lane's tiles
    if (c.pending) (void)hipStreamSynchronize(c.pending_stream);
    if (c.stream) (void)hipStreamSynchronize(c.stream);
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);  // the lagged readback's copy
    // a query enqueued on a caller's stream (the caller synchronises it first; this costs nothing then)
    (void)wait_queries();
    if (reg_ptr) (void)hipHostUnregister(reg_ptr);
    delete lane;
  }
};

namespace sptr {
namespace {

int fail(Context& c, int code, const std::string& msg) {
  c.err = msg;
  return code;
}
int sync_pending(Context& c);

#define API_HIP(x)                                                                          \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) return fail(c, SPTR_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// The context whose shading state (materials and their device table, the geomID -> material table,
// lights, environment, debug mode) a render of c uses: a pixel lane reads its parent's (ADVICE r05:
// a copy per lane put the HDR cubemap into HBM twice, also for scenes the lane never renders).
inline const Context& shading(const Context& c) { return c.parent ? *c.parent : c; }

// One wavefront batch holds up to 2^29 paths (160 B of path state each with one light: 86 GB, under
// a third of the 288 GB of HBM).  Every batch pays the secondary bounces' latency floor once: their
// queues are short (C3: ~1% of the primary rays survive) and each launch lasts as long as its
// longest traversal (~0.2-0.3 ms in the rattan chair), so fewer, larger batches win.  Measured on
// MI355X (C3, 1080p x 256 spp; profiles/r01d_wave_sweep.txt): 2^24 paths/batch 9.8 Grays/s, 2^25
// 15.2, 2^26 22.1, 2^27 29.4, 2^28 37.1, 2^29 42.8.  The default is further capped by free memory.
constexpr uint64_t kDefaultWavePaths = 1ull << 29;
constexpr double kWaveMemFraction = 0.5;  // at most this share of the free HBM for the default batch
// Bounces 0 .. T-1 run as wavefront stages (trace, shade, shadow launches over dense queues); from
// bounce T on, k_tail carries each surviving path to its end in one launch.
// Automatic policy (tail_depth 0), measured on MI355X (C2, profiles/r01d_shards_c2.txt): with a
// full 2^27-path batch the deep-bounce launches are large enough to pay for themselves and the
// wavefront wins (no tail: 4.20 ms vs 4.34 ms with a tail from bounce 4); in the small per-rank
// batches of a sharded frame the fixed cost of the 3 launches per deep bounce dominates, and the
// tail from bounce 4 wins (8-way shard: 0.723 ms vs 0.794; 4-way: 1.208 vs 1.238).
// Scenes traversed from L2/HBM (wide BVH): the late bounces hold few rays, but every wavefront launch
// lasts as long as its longest traversal (the 64-255-visit grazing rays of a 10M-triangle mesh: ~0.25
// ms per trace or shadow launch however few rays it holds), so the tail takes over early whatever
// the batch size.  Measured r03 (SPTR_TAIL_WAVES 4): C3 (L2-resident) tail from bounce 2 4.22 vs 5.07
// ms/step without a tail (from 3: 4.58); C5 (HBM) from bounce 3 10.67 vs 11.58 (from 2: 12.12).  LDS
// scenes keep the batch-size rule (C2 1 GPU: no tail 3.21, from 4 3.31, from 3 3.48 ms).
constexpr uint32_t kSmallBatchTailDepth = 4;
constexpr uint64_t kSmallBatchPaths = 1ull << 25;  // batches up to this many paths take the tail
uint32_t auto_tail_depth(uint64_t batch_paths, const SceneView& sv) {
  if (sv.lds_bytes == 0u) return sv.scene_bytes <= (4ull << 20) ? 2u : 3u;
  return batch_paths <= kSmallBatchPaths ? kSmallBatchTailDepth : (uint32_t)kMaxDepth;
}
// Bounces 1 .. T-1 of an LDS-staged one-light scene as one launch whose blocks trace the continuation rays
// they wrote themselves (k_bounce_chain) instead of k_bounce01 and one k_bounce per bounce
// (sptr_set_bounce_chain: 1 never, 2 wherever those kernels run).
// Automatic policy (mode 0): off.  Measured on MI355X, bench.py runs alternated on one box (C2, two lanes,
// ms/step, separate launches -> chain; profiles/r07_chain_ab.txt).  The chain is bounces 1 .. 3 in the sharded
// frames (tail from bounce 4) and 1 .. 5 on one GPU:
//   8-way shard (2^23 paths per lane batch), same build with the chain off / on, five runs each:
//   0.452-0.454 -> 0.452-0.457; against the parent build 0.457-0.461 -> 0.443-0.451 on one box and
//   0.450-0.455 -> 0.448-0.454 on another: not told from the spread;
//   4-way (2^24) 0.720-0.725 -> 0.723-0.726 and 2-way (2^25) 1.319-1.325 -> 1.321-1.333: inside the spread;
//   1 GPU (2^26) 2.286-2.286 -> 2.347-2.355: slower.  Nothing re-deals the rays between the phases, and one
//   launch bound serves both k_bounce01's registers (96, 5 waves/SIMD) and k_bounce's occupancy (80, 6): at 5
//   the 8-way shard was 0.449-0.454 -> 0.455-0.458 and 1 GPU 2.294-2.298 -> 2.468-2.472, so the chain runs at 6.
// No batch size gains outside the spread, so only mode 2 takes the chain.
bool bounce_chain_on(const Context& c, uint64_t batch_paths) {
  (void)batch_paths;
  return c.bounce_chain == 2u;
}
// The culled bulk of a lane-group bounce 0 with a cull mask, summed thread per pixel by k_sky's list mode while
// k_trace_wp walks the remaining items (sky_split.h; sptr_set_sky_split: 1 never, 2 wherever that bounce 0 runs).
// Returns the bulk thread count T of the batch, 0 for no split.
// T: three quarters of the list mode's resident threads.  The launch runs as the batch's last before k_accum (below),
// beside the other lane's late bounces or alone, so it wants most of the machine's thread slots; a larger T also
// leaves more culled pixels (up to T - 1) to the lane groups.  Measured on MI355X, C2 (two lanes) and its 2-way
// shard, ms/step, split off 2.096-2.107 / 1.235: T = 64 K, 128 K, 192 K, 256 K, 384 K, 512 K threads (the resident
// grid is 512 K) 2.154-2.162, 2.117-2.122, 2.071-2.073, 2.010-2.018, 1.982-1.994, 1.987-1.996 / 1.187, 1.129-1.132,
// 1.171-1.178, 1.152-1.153, 1.124-1.125, 1.225-1.227 (512 K exceed the shard lane's culled pixels: no bulk).
// Rule: the culled count is known only on the device, so the batch's pixels stand in for it: on from 5/4 pixels
// per bulk thread, from where every thread has a pixel if four fifths of the pixels are culled (C2: 88 %).  That
// takes the lanes of a 1080p frame and of its 2-way shard (1.04 M and 522 K pixels against T = 384 K) and leaves
// the 4-way shard's (261 K) and everything smaller to the parent's launches.  With fewer culled pixels than T,
// m = 0: the item list is every valid pixel, the parent's work, and the list launch only marks the tile slots
// outside the image.  DESIGN.md section 9.3, profiles/r10_sky_split_ab.txt.
#ifndef SPTR_SKY_SPLIT_TNUM
#define SPTR_SKY_SPLIT_TNUM 3  // T = resident threads * TNUM / TDIV
#endif
#ifndef SPTR_SKY_SPLIT_TDIV
#define SPTR_SKY_SPLIT_TDIV 4
#endif
constexpr uint64_t kSkySplitPixelsNum = 5, kSkySplitPixelsDen = 4;  // pixels per bulk thread from which mode 0 splits
uint32_t sky_split_threads(const Context& c, const SceneView& sv, const ShadeView& sh, const FrameView& fv) {
  uint32_t mode = c.sky_split, threads = c.sky_split_threads;
#ifdef SPTR_EXPERIMENT_KNOBS
  if (const char* e = getenv("SPTR_SKY_SPLIT"); e && mode == 0u && threads == 0u) {  // "mode[,threads]" (A/B)
    mode = (uint32_t)atoi(e);
    if (const char* t = strchr(e, ',')) threads = (uint32_t)atoi(t + 1);
  }
#endif
  if (mode == 1u || fv.cull == nullptr || fv.pixel_major != kFoldWave || sv.lds_bytes == 0u) return 0u;
  const uint32_t T = threads ? threads
                             : std::max(1u, sky_list_resident_threads(sh) / (uint32_t)SPTR_SKY_SPLIT_TDIV * (uint32_t)SPTR_SKY_SPLIT_TNUM);
  if (mode == 2u) return T;
  return (uint64_t)fv.P * kSkySplitPixelsDen >= kSkySplitPixelsNum * T ? T : 0u;
}
// The place of the list-mode launch in the batch's chain: the last launch before k_accum.  It writes only accum
// words of pixels that are no item of k_trace_wp's, which nothing reads before k_accum, so any place is correct.
// Ahead of k_trace_wp it delays the lane's whole chain by its own length; at the end it runs beside the other
// lane's short late-bounce launches.  Measured (as above, ahead of the trace): C2 2.031-2.037, 2.027-2.042,
// 2.032-2.056, 2.049, 2.051-2.058, 2.059-2.063; 2-way shard 1.190-1.194, 1.179-1.193, 1.183-1.185, 1.203-1.206,
// 1.183-1.194, 1.225-1.227: ahead, a small T is best and gains 3 %; last, a large T gains 5.6 % / 9 %.
static bool sky_split_late() {
#ifdef SPTR_EXPERIMENT_KNOBS
  static const bool early = getenv("SPTR_SKY_SPLIT_EARLY") != nullptr;  // (A/B)
  return !early;
#else
  return true;
#endif
}
// The fused launches per bounce: k_shade_trace (shade the previous bounce's hits on dense lanes, then trace)
// for batches of more than kShadeFirstMinPaths paths, k_bounce01 + k_bounce for the others.  In a small batch
// a launch lasts as long as its longest wave, and k_shade_trace's closing launch (shade, trace, shade) is the
// heaviest kernel on the smallest stream.  Measured: DESIGN.md §4 "Shade first", profiles/r08_bounce_order_ab.txt.
#ifndef SPTR_SHADE_FIRST_MIN_PATHS
#define SPTR_SHADE_FIRST_MIN_PATHS (5ull << 22)  // 21.0 M: lost at 16.7 M and below, level at 22.3 M, ahead from 33.4 M
#endif
constexpr uint64_t kShadeFirstMinPaths = SPTR_SHADE_FIRST_MIN_PATHS;
bool shade_first_on(uint64_t batch_paths) { return batch_paths > kShadeFirstMinPaths; }

// MaterialManager::getMaterialFromHit (src/MaterialManager.cpp:91-103): the geomID's mapped
// material when it is in range, else MaterialManager::getMaterialByID(geomID) (:79-89).
// LDS-staged scenes: the material of every primitive slot of c's scene (ShadeView::prim_mat, prim_mat_table.h),
// from the geomID -> material table of the context whose shading c renders with.  The slots are c's own: a pixel
// lane holds its own build of the scene, so it gets its own table, rebuilt whenever the owner's geom_mat changes
// (sptr_upload_scene, sptr_set_materials).  Without a table (no materials yet, a scene traversed from L2/HBM)
// the kernels read geom_mat through the slot's geomID, and the bounces are not fused (shade_fuses_shadows).
int build_prim_materials(Context& c) {
  const Context& own = shading(c);
  c.prim_mat_n = 0u;
  const uint32_t n = prim_mat_entries(c.num_tri_refs, c.num_sph);
  if (!c.have_scene || n == 0u || own.mats_host.empty() || own.geom_mat.p == nullptr ||
      own.num_tri_geoms != c.num_tri_geoms || own.num_sph != c.num_sph || scene_view(c).lds_bytes == 0u)
    return SPTR_OK;
  API_HIP(hipSetDevice(c.device));
  API_HIP(c.prim_mat.ensure(prim_mat_bytes(c.num_tri_refs, c.num_sph)));
  launch_prim_materials(static_cast<const uint32_t*>(c.tri_geom.p), static_cast<const uint32_t*>(c.sph_geom.p),
                        static_cast<const uint32_t*>(own.geom_mat.p), c.num_tri_refs, c.num_sph,
                        static_cast<uint32_t*>(c.prim_mat.p), c.stream);
  API_HIP(hipGetLastError());
  API_HIP(hipStreamSynchronize(c.stream));
  c.prim_mat_n = n;
  return SPTR_OK;
}

int resolve_geom_materials(Context& c) {
  const uint32_t nm = (uint32_t)c.mats_host.size();
  const uint32_t ng = c.num_tri_geoms + c.num_sph;
  c.prim_mat_n = 0u;
  if (!c.have_scene || nm == 0) return SPTR_OK;
  std::vector<uint32_t> t(ng ? ng : 1, 0u);
  for (uint32_t g = 0; g < ng; ++g) {
    uint32_t m = ~0u;
    if (g < c.geom_material.size() && c.geom_material[g] < nm) m = c.geom_material[g];
    else m = (g < nm) ? g : g % nm;
    t[g] = m;
  }
  API_HIP(c.geom_mat.ensure(t.size() * 4));
  API_HIP(hipMemcpy(c.geom_mat.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  // scenes traversed from L2/HBM: the material of every triangle slot, so that shading a hit loads it
  // directly instead of the slot's geomID and then its material
#ifndef SPTR_TRI_MAT
#define SPTR_TRI_MAT 1
#endif
  c.tri_mat.release();
  if (SPTR_TRI_MAT && scene_view(c).lds_bytes == 0u && c.num_tri_refs) {
    API_HIP(c.tri_mat.ensure((size_t)c.num_tri_refs * 4));
    launch_tri_materials(static_cast<const uint32_t*>(c.tri_geom.p), static_cast<const uint32_t*>(c.geom_mat.p),
                         c.num_tri_refs, static_cast<uint32_t*>(c.tri_mat.p), c.stream);
    API_HIP(hipGetLastError());
    API_HIP(hipStreamSynchronize(c.stream));
  }
  return build_prim_materials(c);
}

inline bool host_local_pixel(const Context& c, uint32_t l, int& x, int& y) {
  return shard_pixel(c.W, c.H, c.G, c.R, l, x, y);
}

// segment tables (3 x (kMaxSegs + 4) u32), per-block tallies (2 x kMaxSegs u64), work counters
size_t seg_table_bytes() { return 3 * (kMaxSegs + 4) * 4 + 2 * kMaxSegs * 8 + kWorkWords * 4; }

// device bytes per path slot of a wave: ray streams 2 x (o, d, thr, ref), hit record(s), radiance, and
// L shadow tasks of ts float4s.  hrec_mult: hit-record segments per static share (2 when the trace
// takes its rays from the per-XCD queues, trace_queue_applies; else 1).
uint64_t wave_path_bytes(uint32_t L, uint32_t ts, uint32_t hrec_mult) {
  return 2 * (3 * 16 + 4) + hrec_mult * kHitBytes + 16 + (uint64_t)L * ts * 16;
}
// fixed segment slack of a wave's streams (see ensure_wave); k_slack = hit-record slack multiplier
uint64_t wave_slack_bytes(uint32_t L, uint32_t ts, uint32_t k_slack, uint32_t hrec_mult) {
  const uint64_t recs = (uint64_t)kMaxSegs * kBlock;
  return recs * (2 * (3 * 16 + 4) + (uint64_t)(L ? L : 1u) * ts * 16) + hrec_mult * recs * k_slack * kHitBytes;
}

// k_slack: the pixel-major bounce-0 trace gives each block a hit-record segment of k records per
// pixel slot of its static share, so the hit records span cap + kMaxSegs * kBlock * k (k_slack = k);
// every other producer needs cap + kMaxSegs * kBlock (k_slack = 1).  hrec_mult: see wave_path_bytes.
int ensure_wave(Context& c, uint64_t cap, uint32_t L, uint32_t ts, uint32_t k_slack, uint32_t hrec_mult) {
  WaveBufs& b = c.wb;
  L = L ? L : 1u;
  const size_t hrec_bytes = ((size_t)cap + (size_t)kMaxSegs * kBlock * k_slack) * kHitBytes * hrec_mult;
  const bool grow = b.hrec.bytes < hrec_bytes || !(b.cap >= cap && b.L * b.ts >= L * ts && b.rad.p) || !b.seg.p;
  if (grow && sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;  // pending renders may still use the old streams
  if (grow) ++c.epoch;
  if (!b.seg.p) {  // segment tables, per-block tallies and work counters, zeroed once
    API_HIP(b.seg.ensure(seg_table_bytes()));
    API_HIP(hipMemset(b.seg.p, 0, seg_table_bytes()));
  }
  // straggler records (k_trace_dyn -> k_strag, scenes beyond an XCD's L2): kStragCap per bounce
  if (strag_applies(scene_view(c))) API_HIP(b.strag.ensure((size_t)kStragHandoffBounces * kStragCap * kStragRec * 16u));
  API_HIP(b.hrec.ensure(hrec_bytes));
  if (b.cap >= cap && b.L * b.ts >= L * ts && b.rad.p) return SPTR_OK;
  // Segmented streams: a stage with G blocks writes block b's outputs at [b*per, b*per + count)
  // with per = ceil(n / (G*kBlock)) * kBlock, so the segment space G*per can exceed n by up to
  // G*kBlock - 1 records: every segmented stream carries kMaxSegs*kBlock records of slack.
  const size_t n = (size_t)cap, ns = n + (size_t)kMaxSegs * kBlock;
  for (auto& r : b.rs)
    for (DevBuf& x : r) API_HIP(x.ensure(ns * 16));
  for (DevBuf& x : b.rs_ref) API_HIP(x.ensure(ns * 4));
  API_HIP(b.rad.ensure(n * 16));
  API_HIP(b.stask.ensure(ns * L * ts * 16));
  b.cap = cap;
  b.L = L;
  b.ts = ts;
  return SPTR_OK;
}

uint32_t task_stride(const Context& c) {
  for (const DevLight& l : shading(c).lights_host)
    if (l.type != 0) return 3u;
  return 2u;
}

WaveView wave_view(Context& c) {
  const WaveBufs& wb = c.wb;
  WaveView w;
  for (int b = 0; b < 2; ++b) {
    w.rs[b].o = static_cast<float4*>(wb.rs[b][0].p);
    w.rs[b].d = static_cast<float4*>(wb.rs[b][1].p);
    w.rs[b].thr = static_cast<float4*>(wb.rs[b][2].p);
    w.rs[b].ref = static_cast<uint32_t*>(wb.rs_ref[b].p);
  }
  const uint64_t hcap = std::min<uint64_t>(wb.hrec.bytes / kHitBytes, 0xFFFFFFFFull);
  w.hrec.tr = static_cast<uint2*>(wb.hrec.p);
  w.hrec.id = reinterpret_cast<uint32_t*>(static_cast<char*>(wb.hrec.p) + hcap * 8u);
  w.rad = static_cast<float4*>(wb.rad.p);
  w.stask = static_cast<float4*>(wb.stask.p);
  uint32_t* seg = static_cast<uint32_t*>(wb.seg.p);  // 3 tables of kMaxSegs counts + 1 stride
  w.segN = SegTable{seg, seg + kMaxSegs};
  w.segH = SegTable{seg + (kMaxSegs + 4), seg + (kMaxSegs + 4) + kMaxSegs};
  w.segS = SegTable{seg + 2 * (kMaxSegs + 4), seg + 2 * (kMaxSegs + 4) + kMaxSegs};
  w.bstat = reinterpret_cast<unsigned long long*>(seg + 3 * (kMaxSegs + 4));
  w.bstat_closest = w.bstat + kMaxSegs;
  w.work = reinterpret_cast<uint32_t*>(w.bstat_closest + kMaxSegs);
  w.tot = static_cast<unsigned long long*>(c.w_tot.p);
  w.L = (uint32_t)shading(c).lights_host.size();
  w.tstride = task_stride(c);
  w.defer_miss = 0u;
  w.seg_cap = (uint32_t)(wb.cap + (uint64_t)kMaxSegs * kBlock);
  w.hrec_cap = (uint32_t)hcap;
  w.strag = static_cast<float4*>(wb.strag.p);
  w.strag_cap = wb.strag.p ? kStragCap : 0u;
  w.strag_lanes = 0u;  // set per trace launch (enqueue_wavefront)
  w.carry_depth = kNoHit;
  return w;
}

FrameView frame_view(const Context& c, const sptr_frame& f) {
  FrameView v;
  v.W = f.width;
  v.H = f.height;
  v.ntx = (f.width + kTile - 1) / kTile;
  v.G = c.G;
  v.R = c.R;
  v.P = c.P;
  v.k = 1;
  v.acc0 = f.frame_begin;
  v.max_depth = f.max_depth;
  v.div_P = make_fastdiv(c.P ? c.P : 1u);
  v.div_ntx = make_fastdiv((uint32_t)v.ntx);
  v.valid = 0;
  // (c.W == 0: the pixel buffers await their next layout — an upload or a lane change after a two-lane
  // accumulation sets it — and the callers that get here before the next render, sptr_primary_rays and
  // sptr_render_rays, read no pixel; the tile count is stale then and ntx would be 0)
  if (c.W > 0) {
    const int ntx = (c.W + kTile - 1) / kTile;
    for (uint32_t lt = 0; lt < c.local_tiles; ++lt) {
      const uint32_t t = lt * (uint32_t)c.G + (uint32_t)c.R;
      const int x0 = (int)(t % (uint32_t)ntx) * kTile, y0 = (int)(t / (uint32_t)ntx) * kTile;
      v.valid += (uint32_t)(std::min(kTile, c.W - x0) * std::min(kTile, c.H - y0));
    }
  }
  const sptr_camera& k = f.camera;
  v.cam_pos = v3(k.pos[0], k.pos[1], k.pos[2]);
  v.cam_f = v3(k.forward[0], k.forward[1], k.forward[2]);
  v.cam_r = v3(k.right[0], k.right[1], k.right[2]);
  v.cam_u = v3(k.up[0], k.up[1], k.up[2]);
  v.half_w = k.half_width;
  v.half_h = k.half_height;
#ifdef SPTR_EXPERIMENT_KNOBS
  // SPTR_ABLATE (timing experiments only: wrong images by design); experiment builds only
  static const uint32_t ablate = getenv("SPTR_ABLATE") ? (uint32_t)atoi(getenv("SPTR_ABLATE")) : 0u;
  v.ablate = ablate;
#else
  v.ablate = 0u;
#endif
  v.accum = static_cast<float4*>(c.accum.p);
  v.reset = 0;
  v.pixel_major = 0;
  v.dyn = nullptr;
  v.cull = nullptr;
  v.cull_depth = 4u;
  v.sky_fold = 0u;
  v.plist = nullptr;
  v.unculled = nullptr;
  v.entry = nullptr;
  v.split_threads = 0u;
  v.integrator = f.integrator;
  v.spf = f.samples_per_frame ? f.samples_per_frame : 4u;
  return v;
}

// The shadow entry table of cc (Context::se) is current: built for cc's scene as it stands and for the light
// direction of the one directional light the shading context holds.  What it was built for is its whole key:
// an upload, a refit, a transform update or other lights leave it unused until refresh_shadow_entries rebuilds it.
static bool shadow_entries_current(const Context& cc) {
  const Context& c = shading(cc);
  if (!cc.se.valid || cc.se.geom_rev != cc.geom_rev || c.lights_host.size() != 1u) return false;
  const DevLight& l = c.lights_host[0];
  return l.type == 0 && cc.se.light.type == 0 && std::memcmp(l.v, cc.se.light.v, sizeof(l.v)) == 0;
}

ShadeView shade_view(const Context& cc) {
  const Context& c = shading(cc);
  ShadeView s{};
  if (cc.shadow_mode != 0u && shadow_entries_current(cc) && cull_entries_apply(scene_view(cc))) {
    s.shadow_entry = static_cast<const uint32_t*>(cc.se.table.p);
    s.shadow_frame = cc.se.frame;
  }
  s.mats = static_cast<const DevMaterial*>(c.mats.p);
  s.num_mats = (uint32_t)c.mats_host.size();
  s.geom_mat = static_cast<const uint32_t*>(c.geom_mat.p);
  s.tri_mat = cc.parent ? nullptr : static_cast<const uint32_t*>(c.tri_mat.p);  // (slots are the owner's)
  // (the slots are cc's own: build_prim_materials)
  const bool pm = cc.prim_mat_n != 0u && cc.prim_mat_n == prim_mat_entries(cc.num_tri_refs, cc.num_sph);
  s.prim_mat = pm ? static_cast<const uint32_t*>(cc.prim_mat.p) : nullptr;
  s.pm_lds_bytes = pm ? prim_mat_lds_bytes(scene_view(cc).lds_bytes, cc.num_tri_refs, cc.num_sph, kLdsSceneBytes) : 0u;
  s.num_lights = (uint32_t)c.lights_host.size();
  for (uint32_t i = 0; i < s.num_lights; ++i) s.lights[i] = c.lights_host[i];
  s.env.env = static_cast<const float4*>(c.env.p);
  s.env.env_size = c.env_size;
  s.env.env_intensity = c.env_intensity;
  s.env.env_clamp = c.env_clamp;
  s.env.debug_mode = c.debug_mode;
  s.debug_mode = c.debug_mode;
  return s;
}

// Stage events on the render stream, kept in the context's pool until collected.  Stages: 0 whole
// render call, 1 trace (bounce >= 1), 2 shade (>= 1), 3 shadow, 4 accum + resolve, 5 trace bounce 0
// (raygen fused), 6 shade bounce 0, 7 tail, 8 pixel cull, 9 fused bounce (k_shade_trace, or k_bounce01 / k_bounce: the trace and the
// shading of a bounce in one launch, counted with the trace launches); 0-9 with SPTR_FRAME_TIMING,
// 1, 3, 5 and 9 with SPTR_FRAME_TIMING_TRACE.
constexpr int kStages = 10;
#ifndef SPTR_CALL_SPAN
#define SPTR_CALL_SPAN 1  // untimed direct calls' span: 0 = event records, 1 = dispatch events, 2 = none (A/B)
#endif
struct StageTimer {
  Context& c;
  bool on;                  // SPTR_FRAME_TIMING or SPTR_FRAME_TIMING_TRACE
  bool trace_only;          // SPTR_FRAME_TIMING_TRACE alone: the trace (1, 5) and shadow (3) launches only
  hipStream_t s;
  hipError_t err = hipSuccess;
  std::string what;         // the call that set err
  size_t open = SIZE_MAX;   // index in c.marks of the stage being recorded
  size_t call = SIZE_MAX;   // index in c.marks of this call's stage-0 span
  size_t alloc() {  // a pool event for this call (not recorded)
    if (c.events_used == c.events.size()) {
      DevEvent e;
      const hipError_t r = hipEventCreate(e.put());
      if (r != hipSuccess) {
        if (err == hipSuccess) {
          err = r;
          what = "stage event create";
        }
        return SIZE_MAX;
      }
      c.events.push_back(std::move(e));
    }
    return c.events_used++;
  }
  bool capturing = false;  // inside a graph capture: no stage events (run_call), the streams are the cap_* ones
  size_t next() {
    const size_t i = alloc();
    if (i != SIZE_MAX && err == hipSuccess) {
      err = hipEventRecord(c.events[i], s);
      if (err != hipSuccess) what = "stage event record";
    }
    return i;
  }
  // the stages that are exactly one launch: timed by the launch itself (g_launch_timing), the others
  // by events recorded on s around them (an event record between two launches idles the GPU for
  // ~5-10 us: r05 8-way C2 shard, 6 records per step -> 2 without the cull and call spans)
  static bool one_launch(int stage) { return stage == 1 || stage == 5 || stage == 9 || stage == 3; }
  bool launch_timed = false;
  bool quiet = false, quiet_open = false;  // untimed launch with dispatch events (run_call)
  void begin(int stage) {
    if (quiet && !on && !capturing && one_launch(stage)) {
      g_launch_timing = LaunchTiming{c.quiet_ev[0], c.quiet_ev[1]};
      quiet_open = true;
      return;
    }
    if (!on || capturing || (trace_only && !one_launch(stage))) return;
    // timed by the dispatch's events (g_launch_timing): the pixel lanes' launches, and the shadow launches,
    // which run on a side stream beside the bounce traces and may wait there after their dispatch for
    // the CUs: a slot's start (block 0 running) leaves that wait out, a dispatch event and rocprofv3's
    // kernel trace count it (C5 r05i: shadow frac 0.48 from slots vs 0.29 from the kernel trace)
    if (one_launch(stage) && (c.time_by_events || stage == 3)) {
      const size_t b = alloc(), e = alloc();
      if (b == SIZE_MAX || e == SIZE_MAX) return;
      open = c.marks.size();
      c.marks.push_back(StageMark{stage, b, e});
      g_launch_timing = LaunchTiming{c.events[b], c.events[e]};
      launch_timed = true;
      return;
    }
    if (one_launch(stage)) {  // timed by the kernel itself (g_tslot -> WaveView::tslot)
      if (!c.tslots.p || c.tslots_used >= kTimeSlots) return;
      open = c.marks.size();
      c.marks.push_back(StageMark{stage, SIZE_MAX, SIZE_MAX, c.tslots_used});
      g_tslot = static_cast<unsigned long long*>(c.tslots.p) + (size_t)kTimeSlotWords * c.tslots_used++;
      launch_timed = true;
      return;
    }
    open = c.marks.size();
    c.marks.push_back(StageMark{stage, next(), SIZE_MAX});
  }
  void end() {
    if (quiet_open) {
      quiet_open = false;
      g_launch_timing = LaunchTiming{};  // (taken by the launch; cleared if there was none)
      return;
    }
    if (open == SIZE_MAX) return;
    if (launch_timed) {
      launch_timed = false;
      if (g_tslot || g_launch_timing.start) {  // nothing was launched: nothing recorded, no mark
        if (g_tslot) --c.tslots_used;
        g_tslot = nullptr;
        g_launch_timing = LaunchTiming{};
        c.marks.erase(c.marks.begin() + (std::ptrdiff_t)open);
      }
      open = SIZE_MAX;
      return;
    }
    c.marks[open].e = next();
    open = SIZE_MAX;
  }
  // The call span of an untimed direct wavefront call: a timing slot whose start the call's first launch
  // (k_frame_dyn) stores and whose end its last (k_accum) takes, like a slot-timed launch's, instead of
  // two event records, each of which idled the GPU for ~5 us (r06, kernel trace of the 8-way C2 shard:
  // 475 us per step with them, 463 without; dispatch events on those two launches left the same gaps).
  uint32_t call_slot = UINT32_MAX;
  bool stop_set = false;
  unsigned long long* slot_ptr(uint32_t i) const {
    return static_cast<unsigned long long*>(c.tslots.p) + (size_t)kTimeSlotWords * i;
  }
  unsigned long long* pre_call(bool wavefront) {  // right before the call's first launch: its t0 word
    if (SPTR_CALL_SPAN != 1 || !wavefront || on || capturing || !c.tslots.p || c.tslots_used >= kTimeSlots)
      return nullptr;
    call_slot = c.tslots_used++;
    return slot_ptr(call_slot);
  }
  void begin_call() {  // (a replayed graph's call span is recorded around its launch: run_call)
    if (capturing || (on && trace_only)) return;  // SPTR_FRAME_TIMING_TRACE: the trace spans only
    if (SPTR_CALL_SPAN == 2 && !on) return;
    call = c.marks.size();
    if (call_slot != UINT32_MAX) c.marks.push_back(StageMark{0, SIZE_MAX, SIZE_MAX, call_slot});
    else c.marks.push_back(StageMark{0, next(), SIZE_MAX});
  }
  void last_launch() {  // right before the call's last launch on s (k_accum)
    if (call_slot == UINT32_MAX || call == SIZE_MAX) return;
    g_tslot = slot_ptr(call_slot);
    stop_set = true;
  }
  void end_call() {
    if (call == SIZE_MAX) return;
    if (call_slot != UINT32_MAX) {  // (a slot whose end was not taken reads as 0 ms)
      if (stop_set) g_tslot = nullptr;
      return;
    }
    c.marks[call].e = next();
  }
};

// The launch intervals [start, end] (device wall-clock ticks) of the context's slot-timed launches in
// this collection window, by slot; {0, 0} for a slot whose launch left no time.
std::vector<std::pair<uint64_t, uint64_t>> read_slots(Context& c) {
  std::vector<std::pair<uint64_t, uint64_t>> iv(c.tslots_used, {0, 0});
  if (c.tslots_used == 0) return iv;
  std::vector<unsigned long long> w((size_t)kTimeSlotWords * c.tslots_used);
  if (hipMemcpy(w.data(), c.tslots.p, w.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return iv;
  for (uint32_t i = 0; i < c.tslots_used; ++i) {
    const unsigned long long* sl = w.data() + (size_t)kTimeSlotWords * i;
    uint64_t t1 = 0;
    for (uint32_t j = 1; j <= kTimeEndLines; ++j) t1 = std::max<uint64_t>(t1, sl[kTimeLineWords * j]);
    const uint64_t t0 = sl[0];
    if (t0 != 0 && t1 >= t0) iv[i] = {t0, t1};
  }
  return iv;
}

// Length of the union of intervals.
template <typename T>
double union_length(std::vector<std::pair<T, T>>& iv) {
  if (iv.empty()) return 0.0;
  std::sort(iv.begin(), iv.end());
  double busy = 0.0;
  T lo = iv[0].first, hi = iv[0].second;
  for (size_t i = 1; i < iv.size(); ++i) {
    if (iv[i].first > hi) {
      busy += (double)(hi - lo);
      lo = iv[i].first;
      hi = iv[i].second;
    } else {
      hi = std::max(hi, iv[i].second);
    }
  }
  return busy + (double)(hi - lo);
}

// Busy time of the trace stage over the pending calls of contexts cs[0..n): the union of the trace
// launches' intervals (stages 1, 5 and 9).  Slot-timed launches are placed on the device's wall clock,
// event-timed ones (the pixel lanes' calls) by their events' offsets from the first such event; both
// clocks are shared by every stream and both lanes, whose trace launches overlap.  (A window holding
// calls of both kinds adds the two unions: such calls run one after the other on the render stream.)
// 0 when a stream fails (collect_pending reports that failure).
double trace_busy_ms(Context* const* cs, int n) {
  std::vector<std::pair<uint64_t, uint64_t>> iv;
  std::vector<std::pair<float, float>> ev;
  double khz = 0.0;
  hipEvent_t ref = nullptr;
  for (int k = 0; k < n; ++k) {
    Context& c = *cs[k];
    if (c.pending == 0) continue;
    if (hipStreamSynchronize(c.pending_stream) != hipSuccess) return 0.0;
    const auto sl = read_slots(c);
    khz = c.wall_khz;
    for (const StageMark& m : c.marks) {
      if (m.stage != 1 && m.stage != 5 && m.stage != 9) continue;
      if (m.slot != UINT32_MAX) {
        if (m.slot < sl.size() && sl[m.slot].second) iv.push_back(sl[m.slot]);
      } else if (m.b < c.events.size() && m.e < c.events.size()) {
        if (!ref) ref = c.events[m.b];
        float b = 0.0f, e = 0.0f;
        if (hipEventElapsedTime(&b, ref, c.events[m.b]) == hipSuccess &&
            hipEventElapsedTime(&e, ref, c.events[m.e]) == hipSuccess)
          ev.emplace_back(b, e);
      }
    }
  }
  return (khz > 0.0 ? union_length(iv) / khz : 0.0) + union_length(ev);
}

// Wait for the pending render calls, fold their device counters and stage events into *stats
// (may be null) and start a new collection window.
int collect_pending(Context& c, sptr_stats* stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (c.pending == 0) return SPTR_OK;
  // (the side streams' work is joined into pending_stream: complete once it is)
  const hipError_t se = hipStreamSynchronize(c.pending_stream);
  Context* self = &c;
  const double busy = se == hipSuccess && stats ? trace_busy_ms(&self, 1) : 0.0;
  double ms[kStages] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t trace_launches = 0, shadow_launches = 0;
  const auto slots = se == hipSuccess ? read_slots(c) : std::vector<std::pair<uint64_t, uint64_t>>();
  for (const StageMark& m : c.marks) {
    float t = 0.0f;
    if (m.slot != UINT32_MAX) {  // timed by the launch itself
      if (m.slot < slots.size()) t = (float)((double)(slots[m.slot].second - slots[m.slot].first) / c.wall_khz);
    } else if (se == hipSuccess && m.b < c.events.size() && m.e < c.events.size()) {
      (void)hipEventElapsedTime(&t, c.events[m.b], c.events[m.e]);
    }
    ms[m.stage] += t;
    if (m.stage == 1 || m.stage == 5 || m.stage == 9) ++trace_launches;
    if (m.stage == 3) ++shadow_launches;
  }
  c.marks.clear();
  c.events_used = 0;
  if (c.tslots_used) {  // the slots this window used, zeroed for the next one (the streams are idle)
    if (se == hipSuccess) (void)hipMemset(c.tslots.p, 0, (size_t)c.tslots_used * kTimeSlotWords * 8);
    c.tslots_used = 0;
  }
  const uint64_t samples = c.pending_samples, waves = c.pending_waves, culls = c.pending_culls;
  c.pending = 0;
  c.pending_samples = c.pending_waves = c.pending_culls = 0;
  if (se != hipSuccess) return fail(c, SPTR_ERR_HIP, std::string("render: ") + hipGetErrorString(se));
  unsigned long long tot[kTotWords];
  API_HIP(hipMemcpy(tot, c.w_tot.p, sizeof(tot), hipMemcpyDeviceToHost));
  if (tot[kTotOverflow]) return fail(c, SPTR_ERR_HIP, "render: segmented stream overflow (internal error)");
  if (tot[kTotStackOverflow]) return fail(c, SPTR_ERR_HIP, "render: BVH traversal stack overflow (internal error)");
  if (!stats) return SPTR_OK;
  stats->ms_total = ms[0];
  stats->ms_raygen = 0.0;  // raygen is fused into the bounce-0 trace (ms_trace0)
  stats->ms_trace = ms[1] + ms[5] + ms[9];
  stats->ms_shade = ms[2] + ms[6];
  stats->ms_trace0 = ms[5];
  stats->ms_shade0 = ms[6];
  stats->ms_shadow = ms[3];
  stats->ms_accum = ms[4];
  stats->trace_launches = trace_launches;
  stats->rays_closest = tot[kTotClosest];
  stats->rays_shadow = tot[kTotShadow];
  stats->rays_tail = tot[kTotTail];
  stats->ms_tail = ms[7];
  stats->samples = samples;
  stats->waves = waves;
  stats->node_visits = tot[kTotNodes];
  stats->tri_tests = tot[kTotTris];
  stats->sphere_tests = tot[kTotSph];
  stats->shadow_node_visits = tot[kTotShNodes];
  stats->shadow_prim_tests = tot[kTotShPrims];
  stats->traced_primary = tot[kTotTracedP];
  stats->traced_bounce = tot[kTotTracedB];
  stats->node_visits_primary = tot[kTotNodesP];
  stats->tri_tests_primary = tot[kTotTrisP];
  stats->sphere_tests_primary = tot[kTotSphP];
  stats->ms_cull = ms[8];
  stats->shadow_launches = shadow_launches;
  for (int d = 0; d < kStatDepths; ++d) {
    stats->traced_by_depth[d] = tot[kTotTracedD + d];
    stats->nodes_by_depth[d] = tot[kTotNodesD + d];
  }
  for (int b = 0; b < kHistBins; ++b) {
    stats->trace_visit_hist[b] = tot[kTotHistT + b];
    stats->shadow_visit_hist[b] = tot[kTotHistS + b];
  }
  stats->hits_primary = tot[kTotHitP];
  stats->hits_bounce = tot[kTotHitB];
  stats->paths_handed_off = tot[kTotStrag];
  for (int i = 0; i < 3; ++i) stats->strag_visits[i] = tot[kTotStragNodes + i];
  stats->cull_launches = culls;
  stats->ms_trace_busy = busy;
  stats->traced_fused = tot[kTotTracedF];
  return SPTR_OK;
}

// Device work of the pending render calls must be complete before a host read of their results.
int sync_pending(Context& c) {
  if (c.pending) API_HIP(hipStreamSynchronize(c.pending_stream));
  return SPTR_OK;
}

// Pixel buffers of a (W, H, shard) configuration.  A pending asynchronous render may still use the
// old buffers, so it is waited for before they are reallocated, and the clears are enqueued on the
// render stream (ordered before this call's kernels).
int ensure_pixels(Context& c, int W, int H, int G, int R, hipStream_t s, bool& resized) {
  resized = false;
  if (c.W == W && c.H == H && c.G == G && c.R == R && c.accum.p) return SPTR_OK;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  const uint32_t local_tiles = shard_tiles(W, H, G, R);
  c.W = W;
  c.H = H;
  c.G = G;
  c.R = R;
  c.local_tiles = local_tiles;
  c.P = local_tiles * (uint32_t)kTilePixels;
  API_HIP(c.accum.ensure((size_t)c.P * 16));
  API_HIP(c.tiles.ensure((size_t)c.P * 4));
  API_HIP(c.image.ensure((size_t)W * H * 3));
  API_HIP(c.cull.ensure((size_t)c.P / 32u * 4u + 4u));
  API_HIP(c.plist.ensure(((size_t)c.P + 2u) * 4u));
  API_HIP(c.entry.ensure((size_t)c.P / 4u * 4u + 4u));
  ++c.epoch;
  API_HIP(hipMemsetAsync(c.accum.p, 0, (size_t)c.P * 16, s));
  API_HIP(hipMemsetAsync(c.tiles.p, 0, (size_t)c.P * 4, s));
  API_HIP(hipMemsetAsync(c.image.p, 0, (size_t)W * H * 3, s));
  c.last_samples = 0;
  resized = true;
  return SPTR_OK;
}

// OptiX-compatible camera and light (OptixBackend::render, src/backends/OptixBackend.cpp:1515-1620):
// cam_u / cam_v scaled from Camera::getRayDirection at the image edges, the first directional light
// as direction FROM the light and colour * intensity.  Host float arithmetic in the reference's order.
void optix_frame_params(const Context& c, const sptr_frame& f, FrameView& v) {
  const sptr_camera& k = f.camera;
  const vec3 fwd = normalize(v3(k.forward[0], k.forward[1], k.forward[2]));
  const vec3 right = normalize(v3(k.right[0], k.right[1], k.right[2]));
  const vec3 up = normalize(v3(k.up[0], k.up[1], k.up[2]));
  const vec3 cf = v3(k.forward[0], k.forward[1], k.forward[2]), cr = v3(k.right[0], k.right[1], k.right[2]),
             cu = v3(k.up[0], k.up[1], k.up[2]);
  auto ray_dir = [&](float u, float vv) {  // Camera::getRayDirection (Camera.cpp:95-106)
    const float nx = (u - 0.5f) * 2.0f, ny = -(vv - 0.5f) * 2.0f;
    return normalize(cf + nx * k.half_width * cr + ny * k.half_height * cu);
  };
  const vec3 dx = ray_dir(1.0f, 0.5f), dy = ray_dir(0.5f, 0.0f);
  const float den_x = dot(dx, fwd), den_y = dot(dy, fwd);
  const float hw = den_x != 0.0f ? dot(dx, right) / den_x : 0.0f;
  const float hh = den_y != 0.0f ? dot(dy, up) / den_y : 0.0f;
  v.ox_u = right * hw;
  v.ox_v = up * hh;
  v.ox_w = fwd;
  v.ox_has_light = 0u;
  v.ox_light_dir = v3(0.0f, -1.0f, 0.0f);
  v.ox_light_rad = v3(0.0f, 0.0f, 0.0f);
  for (const DevLight& l : shading(c).lights_host)
    if (l.type == 0) {  // DevLight keeps the direction TO the light
      v.ox_light_dir = -v3(l.v[0], l.v[1], l.v[2]);
      v.ox_light_rad = v3(l.radiance[0], l.radiance[1], l.radiance[2]);
      v.ox_has_light = 1u;
      break;
    }
}

// Path-per-thread render calls (SPTR_INTEGRATOR_PATHTRACER / _OPTIX): no wavefront streams.
// Frames are launched kPtFramesPerLaunch at a time (bounded launch length); the accumulation order
// is the frame order either way.
constexpr uint32_t kPtFramesPerLaunch = 4;
// Launch sequence of a path-per-thread call on stream s (timer tm on s); returns the launch count.
uint32_t enqueue_path_per_thread(Context& c, const sptr_frame& f, hipStream_t s, StageTimer& tm) {
  const SceneView sv = scene_view(c);
  const ShadeView sh = shade_view(c);
  WaveView w = wave_view(c);
  FrameView fv = frame_view(c, f);
  fv.dyn = static_cast<const uint32_t*>(c.dyn.p);
  const bool optix = f.integrator == SPTR_INTEGRATOR_OPTIX;
  if (optix) optix_frame_params(c, f, fv);
  tm.begin_call();
  uint32_t done = 0, launches = 0;
  while (done < f.spp) {
    fv.k = std::min<uint32_t>(kPtFramesPerLaunch, f.spp - done);
    fv.acc0 = done;                  // offset from the call's frame_begin (frame_dyn)
    fv.reset = done == 0 ? 1u : 0u;  // and the call's reset flag applies to its first batch only
    tm.begin(7);
    if (optix) launch_optix(sv, sh, fv, w, s);
    else launch_pathtracer(sv, sh, fv, w, s);
    tm.end();
    done += fv.k;
    ++launches;
  }
  if (!(f.flags & SPTR_FRAME_NO_RESOLVE)) {
    tm.begin(4);
    launch_resolve(fv, static_cast<const float4*>(c.accum.p), 0u, static_cast<uint32_t*>(c.tiles.p),
                   c.image_out ? c.image_out : static_cast<uint8_t*>(c.image.p), s);
    tm.end();
  }
  tm.end_call();
  return launches;
}


// launches overlapped on the side streams (launch mode 2: everything on one stream)
bool overlap_enabled(const Context& c) {
#ifdef SPTR_EXPERIMENT_KNOBS
  static const bool env = [] {  // SPTR_OVERLAP=0: experiment builds only
    const char* e = getenv("SPTR_OVERLAP");
    return !(e && e[0] == '0');
  }();
  if (!env) return false;
#endif
  return c.launch_mode != 2 && c.side_stream && c.side2_stream;  // (a pixel lane has no side streams)
}

// Launch sequence of a wavefront call (batches of k samples, tail from bounce T) on stream s (the
// caller's stream, or the capture stream inside a graph capture).
//
// Side streams, star-shaped: a launch that overlaps the main sequence is forked from s (an event
// recorded on s, waited on by the side stream) and joined back into s (an event recorded on the side
// stream, waited on by s); a side stream never waits on an event of the other side stream.  Any
// other shape breaks the HIP runtime torch ships (ROCm 7.0): a capture in which one forked stream
// waits on an event recorded by another forked (non-origin) stream — a fork from a fork, or two side
// streams ordered against each other — ends in an endless recursion inside hipStreamEndCapture, which
// overflows the host stack (the r03 libamdhip64+0x2d34a8 crash of the two-lane calls;
// tools/micro/capture_events.hip reproduces it with three streams).  run_call checks every captured
// graph (check_graph) before instantiating it.
// Whether this call's cull is the exact one (k_cull<true>: LDS-staged BVH2 scenes), which also fills the entry
// words.  A cached mask is paid once per camera, so it always is.  A call that recomputes its mask in its own
// sequence (SPTR_FRAME_RECULL) pays the cull every time, at the head of its launch chain, and the exact cull
// costs about three times the box cull (C2: 39 against 16 us; on a shard of one block per CU or less 30
// against 10 us, the time of its longest wave whatever the shard's size), while what it saves in the bounce-0
// trace grows with the call's samples.  Measured on C2 at 64 spp (profiles/r09_cull_entry_ab.txt): the 8-way
// shard, one chain of 16.7 M samples, saves 10 us in k_trace_wp and loses 20 in k_cull (0.438-0.442 -> 0.449-0.451
// ms); the 2-way shard's lanes, 33.4 M samples each, gain (1.262-1.263 -> 1.227-1.234).  Such calls keep the box
// cull below 2^24 samples, the size from which a call is "large" for the pixel lanes too (lanes_for).
constexpr uint64_t kExactRecullMinSamples = 1ull << 24;
bool cull_exact_for(const Context& c, const SceneView& sv, const sptr_frame& f) {
  if (!cull_entries_apply(sv)) return false;
  if (f.flags & SPTR_FRAME_RECULL) return (uint64_t)c.P * f.spp >= kExactRecullMinSamples;
  return true;
}

uint32_t enqueue_wavefront(Context& c, const sptr_frame& f, uint32_t k, int T, hipStream_t s, StageTimer& tm) {
  const SceneView sv = scene_view(c);
  const ShadeView sh = shade_view(c);
  WaveView w = wave_view(c);
  FrameView fv = frame_view(c, f);
  fv.dyn = static_cast<const uint32_t*>(c.dyn.p);
  const bool count = (f.flags & SPTR_FRAME_COUNT_VISITS) != 0;
  const bool fuse = shade_fuses_shadows(sv, sh, count);
#ifdef SPTR_EXPERIMENT_KNOBS
  static const bool no_bounce = getenv("SPTR_NO_BOUNCE") != nullptr;
  // SPTR_FUSE_FROM: first fused bounce of a large batch (A/B; 0 = none)
  static const int fuse_from_env = getenv("SPTR_FUSE_FROM") ? atoi(getenv("SPTR_FUSE_FROM")) : 0;
#else
  constexpr bool no_bounce = false;
  constexpr int fuse_from_env = 0;
#endif
  // bounce-0 pixel-frustum cull mask of this call's camera (every batch of the call shares it): made
  // current by refresh_cull ahead of this launch sequence, or, with SPTR_FRAME_RECULL, computed as the
  // sequence's first launch (inside a captured graph, whose key includes the camera and the flag)
  if (!(f.flags & SPTR_FRAME_NO_CULL)) {
    const bool exact = cull_exact_for(c, sv, f);
    fv.cull_depth = cull_depth_for(f.spp, exact);
    fv.cull = static_cast<const uint32_t*>(c.cull.p);
    fv.unculled = static_cast<const uint32_t*>(c.plist.p) + c.P;
    if (exact) fv.entry = static_cast<const uint32_t*>(c.entry.p);  // computed with the mask
  }
  tm.begin_call();
  if (fv.cull && (f.flags & SPTR_FRAME_RECULL)) {  // the count at plist[P] was zeroed by k_frame_dyn
    tm.begin(8);
    launch_cull(sv, fv, static_cast<uint32_t*>(c.cull.p), static_cast<uint32_t*>(c.plist.p),
                fv.entry ? static_cast<uint32_t*>(c.entry.p) : nullptr, c.sky_split_last != 0u, s);
    tm.end();
  }
  uint32_t done = 0, waves = 0;
  const int D = (int)f.max_depth;
  const bool overlap = overlap_enabled(c);
  const bool cap = tm.capturing;
  const hipStream_t ss = cap ? c.cap_side : c.side_stream;   // k_shadow_dyn(d)
  const hipStream_t ks = cap ? c.cap_side2 : c.side2_stream;  // k_sky (apart from the shadow launches it outlasts)
  const Context::DepEvents& ev = c.dev[cap ? 1 : 0];
  auto check = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && tm.err == hipSuccess) {
      tm.err = e;
      tm.what = what;
    }
  };
  auto fork_to = [&](hipStream_t side) {  // side's next launches start after everything enqueued on s so far
    if (!cap) c.last_forked = true;
    check(hipEventRecord(ev.fork, s), "shadow fork record");
    check(hipStreamWaitEvent(side, ev.fork, 0), "shadow fork wait");
  };
  // pending side-stream work: shadow(d) (ev.join) and k_sky (ev.sky)
  bool join = false, join_sky = false;
  auto join_shadow = [&]() {
    if (join) check(hipStreamWaitEvent(s, ev.join, 0), "shadow join wait");
    join = false;
  };
  // any-hit launches of their own (k_shadow_dyn: scenes traversed from L2/HBM) run on the side stream
  // beside the next bounce's trace: shadow(d) only adds to rad[], which the bounce traces then leave
  // alone (misses deferred to k_shade, WaveView::defer_miss); k_shade(d + 1) overwrites the shadow
  // tasks and updates rad[], so it, the tail and k_accum wait for shadow(d) (ev.join)
  const bool shadow_side = overlap && !fuse && shadow_overlaps(sv, w);
  const bool strag = c.strag_lanes != 0u && !count && w.strag != nullptr && strag_applies(sv);
  w.defer_miss = shadow_side ? 1u : 0u;
  // shadow carry (WaveView::carry_depth): the last wavefront bounce before the tail hands its continuing
  // paths' shadow rays to k_tail, so that the tail need not wait for that bounce's shadow launch (which
  // then traces only the shadow rays of paths ending there, beside the tail, joined before k_accum).
  // Not in the visit-count pass (its k_shadow tallies every query).  Only for scenes resident in an
  // XCD's L2 (r05p/q: C3 3.70 -> 3.57 ms/step; C5, traversed from HBM, 7.38-7.44 -> 7.46-7.52: there the
  // tail, path per thread at 4 waves/SIMD, traces the carried rays slower than the refilling
  // k_shadow_dyn, 816 -> 1318 us, and the launch it shortens was 374 us).
  w.carry_depth = (shadow_side && !count && T < D && w.L == 1u && !trace_queue_applies(sv)) ? (uint32_t)(T - 1) : kNoHit;
  StageTimer tside{c, tm.on, tm.trace_only, ss};
  tside.capturing = tm.capturing;
  while (done < f.spp) {
    const uint32_t kk = std::min<uint32_t>(k, f.spp - done);
    fv.k = kk;
    fv.acc0 = done;                  // offset from the call's frame_begin (frame_dyn)
    fv.reset = done == 0 ? 1u : 0u;  // and the call's reset flag applies to its first batch only
    fv.pixel_major = bounce0_pixel_major(sv, fv);
    // culled pixels summed by k_sky (beside the trace when launches overlap): path-major batches.
    // (r04s: handing them to k_sky beside the thread-per-pixel bounce 0 too: C2 3.09-3.20 -> 3.54-3.57 ms)
    fv.sky_fold = (fv.cull != nullptr && fv.pixel_major == kFoldNone) ? 1u : 0u;
    fv.plist = fv.sky_fold ? static_cast<const uint32_t*>(c.plist.p) : nullptr;
    // the culled bulk of a lane-group bounce 0 summed thread per pixel (k_sky's list mode), the rest as an item list
    // (only where this call's cull listed the culled pixels: decided for the call's first batch, sptr_render; a
    // later batch is never the first to take lane groups)
    const bool listed = (f.flags & SPTR_FRAME_RECULL) ? c.sky_split_last != 0u : c.cull_listed;
    fv.split_threads = listed ? sky_split_threads(c, sv, sh, fv) : 0u;
    if (fv.split_threads) fv.plist = static_cast<const uint32_t*>(c.plist.p);
    // fused bounces (k_shade_trace since r08; the figures here are its predecessors k_bounce01 / k_bounce's), in
    // batches of every size since r06: r02 measured them on C2 only where
    // launches are short (8-way shard 0.627 -> 0.590 ms, 2-way 1.887 -> 1.822, but 1 GPU (133 M paths) 3.39
    // -> 3.46 ms: the traversal at the shading kernel's occupancy); after k_bounce01 they gain on the large
    // batches too (r06s: C4, 535 M-path batches, 122.2-122.6 -> 119.2-119.4 ms/step; C2 unchanged)
    const bool fuse_bounce = fuse && !no_bounce;
    const bool shade_first = shade_first_on((uint64_t)kk * c.P);  // k_shade_trace, or k_bounce01 + k_bounce
    // larger batches could fuse only their late bounces, whose queues are short: no gain measured
    // (r03zx, SPTR_FUSE_FROM 2/3/4 on C2: 3.16-3.25 vs 3.17 ms/step)
    const int fuse_from = fuse_bounce ? 1 : ((fuse && !no_bounce && fuse_from_env > 0) ? fuse_from_env : D + 1);
    // segment-table chain: trace(d) -> shade(d) -> {shadow(d), trace(d+1)}; each launcher returns
    // its grid size = the number of segments its consumers scan
    uint32_t g_shade = 0;
    // k_sky beside the tail instead of beside the bounce-0 trace, for scenes beyond an XCD's L2: there the
    // chain's traces are long and latency-bound, and the sky's VALU-bound grid beside bounce 0 took the
    // wave slots of the trace on the critical path (r05t: C5 7.34-7.37 -> 7.08-7.13 ms/step).  C3's
    // cubemap sky outlasts the whole chain (2.5 of 3.6 ms), so it keeps forking at bounce 0.
    const bool sky_late = fv.sky_fold && overlap && shadow_side && T < D && trace_queue_applies(sv);
    // fused bounces alternate the ray tables: the table holding the current rays, and the other
    SegTable rays_tab = w.segN, spare_tab = w.segH;
    for (int d = 0; d < D; ++d) {
      if (d >= T) {  // the remaining bounces, path per thread
        // (shadow(d - 1) adds to rad[], which the tail reads — unless the tail carries those shadow rays
        // itself (w.carry_depth); k_sky only to the culled pixels' accum, joined before k_accum, so the
        // tail runs beside it: C3's k_sky outlasts the whole bounce chain)
        if (w.carry_depth == kNoHit) join_shadow();
        WaveView wt = w;
        wt.segN = rays_tab;
        if (sky_late) {  // k_sky beside the tail, on the (joined) shadow stream, joined before k_accum
          fork_to(ss);
          launch_sky(sh, fv, true, ss);
          check(hipEventRecord(ev.join, ss), "sky join record");
          join = true;
        }
        tm.begin(7);
        launch_tail(sv, sh, fv, wt, d, g_shade, s);
        tm.end();
        break;
      }
      if (d >= fuse_from) {  // shade(d - 1) (+ shadow) and trace(d) in one launch; the last of them shades bounce d too
        WaveView wf = w;
        wf.segN = rays_tab;
        wf.segH = spare_tab;
        tm.begin(9);  // (a trace launch that also shades: ms_trace, trace_launches)
        g_shade = launch_bounce(sv, sh, fv, wf, d, g_shade, shade_first, d + 1 >= std::min(T, D), s);
        tm.end();
        std::swap(rays_tab, spare_tab);
        continue;
      }
      const bool sky = d == 0 && fv.sky_fold && !sky_late;  // the culled pixels' environment sums: accumulation, not k_trace
      const bool sky_side = sky && overlap;
      if (sky && !sky_side) {
        tm.begin(4);
        launch_sky(sh, fv, false, s);
        tm.end();
      }
      // k_sky forks at the same point as the bounce-0 trace (it writes only the culled pixels' accum
      // words, which nothing reads before this batch's k_accum, the join point): its VALU-bound blocks
      // fill the CUs the latency-bound trace leaves idle, above all in the trace's tail.  Enqueued
      // after the trace, so that the trace's grid is dispatched first.  (sky_late: beside the tail.)
      if (sky_side) {
        if (!cap) c.last_forked = true;
        check(hipEventRecord(ev.fork, s), "sky fork record");
      }
      // straggler hand-off of this bounce's trace (scenes beyond an XCD's L2; not the visit-count pass)
      WaveView wt = w;
      wt.strag_lanes = (strag && (uint32_t)d < kStragHandoffBounces) ? c.strag_lanes : 0u;
      if (d == 0 && fv.split_threads && !sky_split_late()) {  // (A/B: the culled bulk ahead of the lane groups)
        tm.begin(4);
        launch_sky_list(sh, fv, s);
        tm.end();
      }
      tm.begin(d == 0 ? 5 : 1);
      const uint32_t g_trace = launch_trace(sv, sh, fv, wt, d, count, g_shade, s);
      tm.end();
      if (sky_side) {
        check(hipStreamWaitEvent(ks, ev.fork, 0), "sky fork wait");
        launch_sky(sh, fv, true, ks);
        check(hipEventRecord(ev.sky, ks), "sky join record");
        join_sky = true;
      }
      join_shadow();  // shadow(d - 1) before shade(d)
      if (wt.strag_lanes) {
        // k_strag(d) after trace(d) and shadow(d - 1) (both may have updated the handed-off paths'
        // radiance), on the k_sky stream, joined before k_accum with k_sky (ev.sky)
        if (overlap) {
          fork_to(ks);
          launch_strag(sv, sh, fv, w, d, ks);
          check(hipEventRecord(ev.sky, ks), "straggler join record");
          join_sky = true;
        } else {
          launch_strag(sv, sh, fv, w, d, s);
        }
      }
      if (d == 0 && fuse_bounce && T >= 2 && D >= 2 && bounce_chain_on(c, (uint64_t)kk * c.P)) {
        // bounce 0's shading and bounces 1 .. T-1 in one launch (k_bounce_chain) in place of k_bounce01 and the
        // fused bounces' launches: the rays of bounce T (if the tail follows) are in rs[T & 1], counted in w.segN
        const int Tc = std::min(T, D);
        tm.begin(9);
        g_shade = launch_bounce_chain(sv, sh, fv, w, Tc, g_trace, s);
        tm.end();
        rays_tab = w.segN;
        spare_tab = w.segH;
        d = Tc - 1;
        continue;
      }
      if (d == 0 && fuse && !no_bounce && T >= 2 && D >= 2) {
        // bounce 0's shading and bounce 1's trace in one launch (k_shade_trace<first>), in batches of every size:
        // bounce 1's hit-ray records go to w.segN, where the fused launches from 2 on take them (as the closing
        // launch, T or D = 2, it shades bounce 1 too and writes the rays of bounce 2).  k_bounce01's r06 A/B on one
        // box: C2 (two lanes, fused bounces) 2.58-2.60 -> 2.36 ms/step, 8-way shard 0.52 -> 0.49; C4 (batches
        // of 535 M paths, separate stages from bounce 2) 136.6 -> 122.4 ms, C2 as one chain 3.01 -> 2.76
        // (gpurun_out/r06p, r06q)
        tm.begin(9);
        g_shade = launch_bounce01(sv, sh, fv, w, g_trace, shade_first, std::min(T, D) <= 2, s);
        tm.end();
        rays_tab = w.segN;
        spare_tab = w.segH;
        d = 1;
        continue;
      }
      tm.begin(d == 0 ? 6 : 2);
      g_shade = launch_shade(sv, sh, fv, w, d, g_trace, fuse, s);
      tm.end();
      if (!fuse && shadow_side) {
        fork_to(ss);
        tside.begin(3);
        launch_shadow(sv, sh, w, d, count, g_shade, ss);
        tside.end();
        check(hipEventRecord(ev.join, ss), "shadow join record");
        join = true;
      } else if (!fuse) {
        tm.begin(3);
        launch_shadow(sv, sh, w, d, count, g_shade, s);
        tm.end();
      }
    }
    // the call's last batch resolves in the same launch (k_accum<true>: each thread resolves the
    // sum it holds, as k_resolve would next)
    const bool resolve = done + kk >= f.spp && !(f.flags & SPTR_FRAME_NO_RESOLVE);
    join_shadow();
    if (join_sky) check(hipStreamWaitEvent(s, ev.sky, 0), "sky join wait");
    join_sky = false;
    if (fv.split_threads && sky_split_late()) {  // the culled bulk (sky_split.h), in this chain (sky_split_late)
      tm.begin(4);
      launch_sky_list(sh, fv, s);
      tm.end();
    }
    tm.begin(4);
    if (done + kk >= f.spp) tm.last_launch();
    launch_accumulate(fv, w, static_cast<float4*>(c.accum.p), static_cast<uint32_t*>(c.tiles.p),
                      c.image_out ? c.image_out : static_cast<uint8_t*>(c.image.p), resolve, s);
    tm.end();
    done += kk;
    ++waves;
  }
  if (tside.err != hipSuccess && tm.err == hipSuccess) {
    tm.err = tside.err;
    tm.what = tside.what;
  }
  tm.end_call();
  return waves;
}

// The shadow entry table (ShadeView::shadow_entry, shadow_entry.h) of a wavefront call: built on the render
// stream ahead of the call's launch sequence, never inside it, when the call qualifies and no current table is
// cached.  It qualifies when the scene is an LDS-staged BVH2 with a root node, its one light is directional and
// the call's shadow rays are traced in place (shade_fuses_shadows), and, in the automatic mode, when the call is
// large enough.  A cached table serves every call (shade_view), whatever its size.
// The bounds follow kExactRecullMinSamples' reasoning, a fixed cost against a gain that grows with the call's
// samples, with this table's figures: a build is one launch of the cull's descent (41 us on C2's scene) and a
// 64-byte read-back with a stream synchronisation, about 55 us together, and the walks gain 0.41 us per million
// samples (C2: 54 us on 132.7 M).
//   The first build after an upload (kShadowEntryMinSamples, 2^23): a scene that is uploaded and then rendered
//   keeps its table from call to call, so the build is paid once where the in-sequence cull is paid in every
//   call.  A call of 2^23 samples gains 3.4 us; a caller that accumulates with calls of that size has the build
//   back within sixteen of them (the pixel lanes of C2's 4-way shard and its 8-way shard, 16.6 M samples a call,
//   are such callers; a 1-spp frame, 2 M at 1080p, is not).
//   A rebuild (kShadowEntryRebuildMinSamples, 2^27): a table that a refit, a transform update or a turn of the
//   light has ended says the caller animates, and the next change may end the new one after a single call.  That
//   call alone must then pay: 55 us / 0.41 us per million = 134 M samples.  Below it the call walks from the
//   root, as it did before there were tables, and pays neither the launch nor the synchronisation.
// Bounds that give no usable frame are remembered with the scene and light they belong to and not read again.
// A build changes the kernels' arguments, so it ends the validity of a captured launch graph (the epoch).
constexpr uint64_t kShadowEntryMinSamples = 1ull << 23;
constexpr uint64_t kShadowEntryRebuildMinSamples = 1ull << 27;
int refresh_shadow_entries(Context& c, const sptr_frame& f, hipStream_t s) {
  if (c.shadow_mode == 0u) return SPTR_OK;
  const SceneView sv = scene_view(c);
  const ShadeView sh = shade_view(c);
  if (sh.shadow_entry) return SPTR_OK;  // current
  if (!cull_entries_apply(sv) || !shade_fuses_shadows(sv, sh, false) || sh.lights[0].type != 0) return SPTR_OK;
  if (sv.root == kNoHit || (sv.root & kLeafBit) || sv.num_nodes == 0u) return SPTR_OK;
  const DevLight& l = sh.lights[0];
  if (c.se.no_frame && c.se.geom_rev == c.geom_rev && std::memcmp(l.v, c.se.light.v, sizeof(l.v)) == 0) return SPTR_OK;
  if (c.shadow_mode == 1u) {
    const bool first = c.se.upload_rev != c.upload_rev;  // nothing was built for this upload yet
    if ((uint64_t)c.P * f.spp < (first ? kShadowEntryMinSamples : kShadowEntryRebuildMinSamples)) return SPTR_OK;
  }
  BvhNode root;
  API_HIP(hipMemcpyAsync(&root, sv.nodes + sv.root, sizeof(BvhNode), hipMemcpyDeviceToHost, s));
  API_HIP(hipStreamSynchronize(s));
  const vec3 lo = v3(std::min(root.lxy.x, root.rxy.x), std::min(root.lxy.z, root.rxy.z), std::min(root.z.x, root.z.z));
  const vec3 hi = v3(std::max(root.lxy.y, root.rxy.y), std::max(root.lxy.w, root.rxy.w), std::max(root.z.y, root.z.w));
  ShadowFrame fr;
  c.se.valid = false;
  c.se.geom_rev = c.geom_rev;
  c.se.light = l;
  c.se.upload_rev = c.upload_rev;
  c.se.no_frame = !shadow_frame(v3(l.v[0], l.v[1], l.v[2]), lo, hi, kShadowEntryCells, fr);
  if (c.se.no_frame) return SPTR_OK;  // (no usable bounds: root walks)
  API_HIP(c.se.table.ensure((size_t)fr.R * fr.R * 4));
  launch_shadow_entries(sv, fr, static_cast<uint32_t*>(c.se.table.p), s);
  API_HIP(hipGetLastError());
  c.se.valid = true;
  c.se.frame = fr;
  ++c.se.builds;
  ++c.epoch;
  return SPTR_OK;
}

// The bounce-0 pixel-frustum cull mask (and unculled-pixel list) of a wavefront call's camera.  It is
// launched directly on the render stream ahead of the call's launch sequence, never inside it: a
// captured launch graph therefore holds no k_cull, and whichever camera a replayed graph was
// captured for, it runs against the mask of the camera of its own call (a graph key includes the
// camera; the mask is recomputed here whenever the camera, the cull depth or the state epoch differ
// from the cached mask's, and on SPTR_FRAME_RECULL).
int refresh_cull(Context& c, const sptr_frame& f, hipStream_t s, bool timing) {
  if (f.flags & SPTR_FRAME_NO_CULL) return SPTR_OK;
  const SceneView sv = scene_view(c);
  const bool exact = cull_exact_for(c, sv, f);
  const uint32_t depth = cull_depth_for(f.spp, exact);
  if (f.flags & SPTR_FRAME_RECULL) {  // the call's own launch sequence computes the mask (enqueue_wavefront)
    c.cull_epoch = 0;  // the cached key is set once that sequence is enqueued (sptr_render)
    return SPTR_OK;
  }
  const bool want_list = c.sky_split_last != 0u;  // this call's bounce 0 splits (sptr_render): it needs the culled list
  if (!(f.flags & SPTR_FRAME_RECULL) && c.cull_epoch == c.epoch && c.cull_depth == depth && c.cull_exact == exact &&
      (c.cull_listed || !want_list) && std::memcmp(&c.cull_cam, &f.camera, sizeof(sptr_camera)) == 0)
    return SPTR_OK;
  FrameView fv = frame_view(c, f);
  fv.cull_depth = depth;
  StageTimer tm{c, timing, true, s};
  tm.begin(8);
  API_HIP(hipMemsetAsync(static_cast<uint32_t*>(c.plist.p) + c.P, 0, 8, s));
  launch_cull(sv, fv, static_cast<uint32_t*>(c.cull.p), static_cast<uint32_t*>(c.plist.p),
              exact ? static_cast<uint32_t*>(c.entry.p) : nullptr, want_list, s);
  tm.end();
  API_HIP(hipGetLastError());
  if (tm.err != hipSuccess) return fail(c, SPTR_ERR_HIP, std::string("render: cull events: ") + hipGetErrorString(tm.err));
  c.cull_epoch = c.epoch;
  c.cull_cam = f.camera;
  c.cull_depth = depth;
  c.cull_exact = exact;
  c.cull_listed = want_list;
  ++c.pending_culls;
  return SPTR_OK;
}

bool same_key(const GraphKey& a, const GraphKey& b) { return std::memcmp(&a, &b, sizeof(GraphKey)) == 0; }

// A captured launch graph is accepted only if it is a DAG of bounded depth: nodes, dependency
// edges and the number of nodes on its longest path (Kahn's algorithm over hipGraphGetEdges).  The
// fork/join plan of enqueue_wavefront yields ~10-200 nodes whose longest path is the main sequence;
// a cycle, or a path longer than the node count, means a broken plan.
struct GraphShape {
  uint32_t nodes = 0, edges = 0, depth = 0;
};
constexpr size_t kMaxGraphNodes = 4096;
bool check_graph(hipGraph_t g, GraphShape& out, std::string& why) {
  size_t n = 0, ne = 0;
  if (hipGraphGetNodes(g, nullptr, &n) != hipSuccess || hipGraphGetEdges(g, nullptr, nullptr, &ne) != hipSuccess) {
    why = "hipGraphGetNodes/Edges failed";
    return false;
  }
  if (n == 0 || n > kMaxGraphNodes) {
    why = std::to_string(n) + " nodes";
    return false;
  }
  std::vector<hipGraphNode_t> nodes(n), from(ne), to(ne);
  if (hipGraphGetNodes(g, nodes.data(), &n) != hipSuccess ||
      (ne && hipGraphGetEdges(g, from.data(), to.data(), &ne) != hipSuccess)) {
    why = "hipGraphGetNodes/Edges failed";
    return false;
  }
  std::vector<std::pair<hipGraphNode_t, uint32_t>> index(n);
  for (size_t i = 0; i < n; ++i) index[i] = {nodes[i], (uint32_t)i};
  std::sort(index.begin(), index.end());
  auto id_of = [&](hipGraphNode_t x) -> int64_t {
    const auto it = std::lower_bound(index.begin(), index.end(), std::make_pair(x, 0u));
    return (it != index.end() && it->first == x) ? (int64_t)it->second : -1;
  };
  std::vector<uint32_t> indeg(n, 0), level(n, 1);
  std::vector<std::vector<uint32_t>> succ(n);
  for (size_t e = 0; e < ne; ++e) {
    const int64_t a = id_of(from[e]), b = id_of(to[e]);
    if (a < 0 || b < 0) {
      why = "edge to an unknown node";
      return false;
    }
    succ[(size_t)a].push_back((uint32_t)b);
    ++indeg[(size_t)b];
  }
  std::vector<uint32_t> ready;
  for (uint32_t i = 0; i < n; ++i)
    if (indeg[i] == 0) ready.push_back(i);
  size_t seen = 0;
  uint32_t depth = 0;
  while (!ready.empty()) {
    const uint32_t v = ready.back();
    ready.pop_back();
    ++seen;
    depth = std::max(depth, level[v]);
    for (uint32_t w : succ[v]) {
      level[w] = std::max(level[w], level[v] + 1);
      if (--indeg[w] == 0) ready.push_back(w);
    }
  }
  out.nodes = (uint32_t)n;
  out.edges = (uint32_t)ne;
  out.depth = depth;
  if (seen != n) {
    why = "dependency cycle (" + std::to_string(n - seen) + " of " + std::to_string(n) + " nodes)";
    return false;
  }
  return true;
}

// Enqueue one render call's launch sequence on s.  A call shape seen twice in a row is captured
// once into a hipGraph (on the context's capture stream) and replayed from then on: one graph
// launch instead of ~20 kernel launches, with the per-call values (frame_begin, reset, total) passed
// as the arguments of the graph's k_frame_dyn node.  The launch sequence itself is the same code
// either way.  A replay's call span (stage 0) is recorded around its hipGraphLaunch; calls with stage
// timing (SPTR_FRAME_TIMING*) always run as direct launches: a stage span inside a graph would need
// external event-record nodes, which torch's HIP 7.0 runtime (the one bench.py and any process that
// imports torch first binds libsptr_hip to) refuses inside a capture (hipErrorInvalidValue, r04g).
constexpr uint64_t kGraphMinSamples = 1ull << 24;  // launch mode 0 captures calls of at least this many samples
template <class Enqueue>
int run_call(Context& c, const GraphKey& key, uint32_t frame_begin, uint32_t reset, uint32_t total, uint64_t samples, uint32_t* clear,
             bool timing, bool trace_only, hipStream_t s, Enqueue&& enqueue, uint32_t& waves) {
  const bool repeat = c.have_last_key && same_key(key, c.last_key);
  c.last_key = key;
  c.have_last_key = true;
  // mode 0 captures a call whose launches fork nothing to the side streams: the runtime's graph executor
  // does not run a graph's parallel branches concurrently, so a call with side-stream launches replays
  // slower than it launches directly, at every size measured (r04h: C5 8.70 vs 8.18 ms, C3 3.80 vs 3.75;
  // r05i, 1-spp frames, C5 at 256x144 / 512x288 / 960x540 / 1920x1080: 1.87 / 2.21 / 2.52 / 3.11 vs
  // 1.23 / 1.50 / 1.72 / 2.22 ms, C3 0.46 / 0.61 / 0.78 / 0.96 vs 0.44 / 0.57 / 0.73 / 0.92 ms; r05k, the
  // default scene's 1-spp 1080p frame, which forks only k_sky: 0.47 vs 0.41 ms).  C2's 64-spp call forks
  // nothing: 3.07 graph vs 3.10 ms direct.  Mode 3 captures every repeated shape.
  // Nor does mode 0 capture small calls: the default scene's 1-spp frames (r05zh, sptr_cli, 400 frames,
  // two repetitions; mean wall / device ms, graph vs direct) 640x360 0.42/0.18 and 0.31/0.18 vs 0.38/0.19
  // and 0.30/0.20; 800x600 0.33/0.21 vs 0.31/0.22; 1280x720 0.37-0.38/0.22 vs 0.35/0.24; 1920x1080 (whose
  // pixel-major bounce 0 forks nothing) 0.46/0.25 vs 0.41-0.42/0.23 — the replays' device time is at best
  // 10 us shorter and their wall time has spikes.  Calls from kGraphMinSamples on (C2: 2.98 vs 3.02 ms).
  // Nor the halves of a two-lane call (time_by_events marks them): the two lanes' graphs replayed beside
  // each other measured slower than their direct launches (r05i, C2: 2.865 vs 2.528 ms per call).
  const bool graphable = c.launch_mode == 3 ||
                         (c.launch_mode == 0 && !c.last_forked && !c.time_by_events && samples >= kGraphMinSamples);
  const bool bad = c.have_bad_key && same_key(key, c.bad_key);  // this shape failed to capture before
  auto direct = [&]() -> int {
    c.last_forked = false;  // (set by the launch sequence if it forks)
    StageTimer tm{c, timing, trace_only, s};
    // untimed two-lane calls launch their trace and fused-bounce kernels with dispatch events all the same
    // (two events reused by every such launch, never read): r06l, C2 2.512-2.531 vs 2.548-2.565 ms per step
    // with plain launches, on one box
    tm.quiet = !timing && c.time_by_events && c.quiet_ev[1] != nullptr;
    unsigned long long* t0 = tm.pre_call(key.frame.integrator == SPTR_INTEGRATOR_WAVEFRONT);
    launch_frame_dyn(static_cast<uint32_t*>(c.dyn.p), frame_begin, reset, total, clear, t0, s);
    waves = enqueue(s, tm);
    API_HIP(hipGetLastError());
    if (tm.err != hipSuccess) return fail(c, SPTR_ERR_HIP, "render: " + tm.what + ": " + hipGetErrorString(tm.err));
    return SPTR_OK;
  };
  if (!graphable || timing || bad || !(repeat || (c.graph.valid && same_key(key, c.graph.key)))) return direct();
  if (!(c.graph.valid && same_key(key, c.graph.key))) {  // capture this shape
    c.graph.exec.reset();  // (before its graph)
    c.graph = GraphCache{};
    // a pixel lane's capture stream is its own, created on its first capture (only launch mode 3 captures
    // a lane's calls).  r06: with one capture stream shared by the two contexts, a parent's capture after
    // the lane's (a mode-3 two-lane shape, then direct two-lane calls, then a one-chain shape captured in
    // mode 0) was instantiated, and its first hipGraphLaunch faulted inside torch's HIP runtime (a null
    // member read at libamdhip64+0xaee41, gpurun_out/r06e); with a stream per context it does not.
    if (!c.cap_stream && hipStreamCreateWithFlags(c.cap_stream.put(), hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      return direct();
    }
    GraphShape gshape;
    // A shape that cannot be captured (the capture fails, leaves a forked stream capturing, or yields
    // a graph check_graph rejects or the runtime cannot instantiate) is remembered and launched
    // directly, this call and every later one: the direct launches are safe (the runtime faults
    // only while ending a capture), and a failing shape re-captured per call would never render.
    // graph_info / sptr_capture_error report why.
    auto not_capturable = [&](hipError_t status, const std::string& why) -> int {
      c.capture_status = (int32_t)(status != hipSuccess ? status : hipErrorUnknown);
      c.capture_error = why;
      c.bad_key = key;
      c.have_bad_key = true;
      (void)hipGetLastError();
      return direct();
    };
    API_HIP(hipStreamBeginCapture(c.cap_stream, hipStreamCaptureModeThreadLocal));
    StageTimer tm{c, false, false, c.cap_stream};
    tm.capturing = true;
    const uint32_t nw = enqueue(c.cap_stream, tm);
    GraphCache gc;
    DevGraph& g = gc.graph;  // (dropped with gc on every path that does not keep it)
    const hipError_t ec = hipStreamEndCapture(c.cap_stream, g.put());
    // every stream the capture forked must have left capture mode with it (a stream still capturing
    // would fold the next direct launches into a dead graph): end the capture on any that did not
    bool stuck = false;
    for (hipStream_t st : std::initializer_list<hipStream_t>{c.cap_stream, c.cap_side, c.cap_side2}) {
      if (!st) continue;
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        stuck = true;
        DevGraph gs;
        (void)hipStreamEndCapture(st, gs.put());
      }
    }
    if (stuck)
      return not_capturable(hipErrorStreamCaptureUnjoined, "graph capture: a forked stream was still capturing");
    if (ec != hipSuccess || tm.err != hipSuccess || !g)
      return not_capturable(ec != hipSuccess ? ec : tm.err,
                            ec != hipSuccess ? std::string("hipStreamEndCapture: ") + hipGetErrorString(ec)
                                             : tm.what + ": " + hipGetErrorString(tm.err));
    {
      std::string why;
      if (!check_graph(g, gshape, why)) return not_capturable(hipErrorInvalidValue, "captured graph rejected: " + why);
    }
    gc.key = key;
    gc.waves = nw;
    gc.nodes = gshape.nodes + 1;  // + the k_frame_dyn head added below, ahead of every root
    gc.depth = gshape.depth + 1;
    // the k_frame_dyn node heads the graph: every captured root depends on it
    size_t nr = 0;
    API_HIP(hipGraphGetRootNodes(g, nullptr, &nr));
    std::vector<hipGraphNode_t> roots(nr);
    API_HIP(hipGraphGetRootNodes(g, roots.data(), &nr));
    void* dyn_ptr = c.dyn.p;
    uint32_t a0 = frame_begin, a1 = reset, a2 = total;
    uint32_t* a3 = clear;
    unsigned long long* a4 = nullptr;  // (a replay's call span: event records around its launch)
    void* args[6] = {&dyn_ptr, &a0, &a1, &a2, &a3, &a4};
    hipKernelNodeParams kp{};
    kp.func = const_cast<void*>(frame_dyn_kernel());
    kp.gridDim = dim3(1);
    kp.blockDim = dim3(64);
    kp.sharedMemBytes = 0;
    kp.kernelParams = args;
    kp.extra = nullptr;
    API_HIP(hipGraphAddKernelNode(&gc.dyn_node, g, nullptr, 0, &kp));
    for (hipGraphNode_t r : roots) API_HIP(hipGraphAddDependencies(g, &gc.dyn_node, &r, 1));
    gc.edges = gshape.edges + (uint32_t)nr;
    gc.dyn_params = kp;
    const hipError_t ei = hipGraphInstantiate(gc.exec.put(), g, nullptr, nullptr, 0);
    if (ei != hipSuccess) return not_capturable(ei, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
    gc.valid = true;
    c.graph = std::move(gc);
    ++c.captures;
  }
  // replay: the call's values into the k_frame_dyn node, the call span around the launch
  GraphCache& gc = c.graph;
  void* dyn_ptr = c.dyn.p;
  uint32_t a0 = frame_begin, a1 = reset, a2 = total;
  uint32_t* a3 = clear;
  unsigned long long* a4 = nullptr;
  void* args[6] = {&dyn_ptr, &a0, &a1, &a2, &a3, &a4};
  hipKernelNodeParams p = gc.dyn_params;
  p.kernelParams = args;
  p.extra = nullptr;
  API_HIP(hipGraphExecKernelNodeSetParams(gc.exec, gc.dyn_node, &p));
  StageTimer tm{c, false, false, s};
  tm.begin_call();
  API_HIP(hipGraphLaunch(gc.exec, s));
  tm.end_call();
  if (tm.err != hipSuccess) return fail(c, SPTR_ERR_HIP, "render: " + tm.what + ": " + hipGetErrorString(tm.err));
  waves = gc.waves;
  return SPTR_OK;
}

}  // namespace
}  // namespace sptr

namespace sptr {
namespace {
bool create_events(Context& c) {
  for (Context::DepEvents& d : c.dev)
    for (DevEvent* e : {&d.fork, &d.join, &d.sky})
      if (hipEventCreateWithFlags(e->put(), hipEventDisableTiming) != hipSuccess) return false;
  for (DevEvent& e : c.quiet_ev)
    if (hipEventCreate(e.put()) != hipSuccess) return false;
  return true;
}
}  // namespace
}  // namespace sptr

using namespace sptr;

extern "C" {

static void add_stats(sptr_stats& a, const sptr_stats& b);  // (pixel lanes, below)

int sptr_abi_version(void) { return SPTR_ABI_VERSION; }


// SPTR_SEGV_TRACE=1 (diagnostics only): a host SIGSEGV prints, before the default action, the fault
// address, the faulting instruction and stack pointer, each code address among the 512 words above the
// stack pointer as library + offset (a scan that needs no unwinder, so it works on an overflowed stack),
// and then the unwinder's backtrace.  Installed once per process, on the first sptr_create, for the
// thread that creates the context (its alternate signal stack).
static void segv_put(const char* s) { (void)!write(2, s, strlen(s)); }
static void segv_hex(uint64_t v) {
  char b[19] = "0x";
  for (int i = 0; i < 16; ++i) b[2 + i] = "0123456789abcdef"[(v >> (60 - 4 * i)) & 15u];
  b[18] = 0;
  segv_put(b);
}
static void segv_where(uint64_t pc) {
  Dl_info di{};
  segv_hex(pc);
  if (dladdr(reinterpret_cast<void*>(pc), &di) && di.dli_fname) {
    segv_put(" ");
    segv_put(di.dli_fname);
    segv_put("+");
    segv_hex(pc - reinterpret_cast<uint64_t>(di.dli_fbase));
    if (di.dli_sname) {
      segv_put(" ");
      segv_put(di.dli_sname);
    }
  }
  segv_put("\n");
}
static void segv_trace(int sig, siginfo_t* si, void* uc_v) {
  const ucontext_t* uc = static_cast<const ucontext_t*>(uc_v);
  const uint64_t pc = (uint64_t)uc->uc_mcontext.gregs[REG_RIP], sp = (uint64_t)uc->uc_mcontext.gregs[REG_RSP];
  segv_put("sptr SIGSEGV: addr ");
  segv_hex(reinterpret_cast<uint64_t>(si->si_addr));
  segv_put(" sp ");
  segv_hex(sp);
  segv_put("\n  pc ");
  segv_where(pc);
  const uint64_t* st = reinterpret_cast<const uint64_t*>(sp);
  for (int i = 0, shown = 0; i < 512 && shown < 96; ++i) {
    Dl_info di{};
    const uint64_t v = st[i];
    if (v > 4096 && dladdr(reinterpret_cast<void*>(v), &di) && di.dli_fname) {
      ++shown;
      segv_put("  ret? ");
      segv_where(v);
    }
  }
  void* fr[64];
  const int n = backtrace(fr, 64);
  backtrace_symbols_fd(fr, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}

static void install_segv_trace() {
  static std::once_flag once;
  std::call_once(once, [] {
    if (getenv("SPTR_SEGV_TRACE") == nullptr) return;
    void* prime[2];
    (void)backtrace(prime, 2);
    static char alt[1 << 20];
    stack_t ss{};
    ss.ss_sp = alt;
    ss.ss_size = sizeof(alt);
    sigaltstack(&ss, nullptr);
    struct sigaction sa{};
    sa.sa_sigaction = segv_trace;
    sa.sa_flags = SA_ONSTACK | SA_SIGINFO;
    sigaction(SIGSEGV, &sa, nullptr);
  });
}

static int create_one(int device, sptr_ctx** out, const sptr_ctx* parent);
int sptr_create(int device, sptr_ctx** out) {
  const int rc = create_one(device, out, nullptr);
  if (rc != SPTR_OK) return rc;
  sptr_ctx* x = *out;
  // the pixel lane: a context of its own (created now, given a scene and a stream only when the scene
  // is staged into LDS)
  if (create_one(device, &x->lane, x) != SPTR_OK) x->lane = nullptr;
  if (x->lane) {
    x->lane->is_lane = true;
    if (hipEventCreateWithFlags(x->lane_fork.put(), hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(x->lane_join.put(), hipEventDisableTiming) != hipSuccess) {
      (void)sptr_destroy(x);
      *out = nullptr;
      return SPTR_ERR_HIP;
    }
  }
  return SPTR_OK;
}

// parent: a pixel lane's context.  It creates no stream here: it makes its own capture stream on its
// first capture (run_call), gets its render stream when it is given a scene
// (sptr_upload_scene) and has no side streams (it renders only scenes staged into LDS, whose launches
// run on one stream).  r05zw: every stream a context creates is one more for the runtime to place on
// the process's hardware queues, and a lane created with a full set of six slowed the parent's
// overlapped C5 / C3 calls from 7.23 / 3.33 to 8.48 / 3.67 ms with the lane never used.
static int create_one(int device, sptr_ctx** out, const sptr_ctx* parent) {
  if (!out) return SPTR_ERR_INVALID;
  install_segv_trace();
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SPTR_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return SPTR_ERR_INVALID;
  sptr_ctx* x = new sptr_ctx();
  Context& c = x->c;
  c.device = device;
  if (parent) {
    c.parent = &parent->c;
    c.prio_lo = parent->c.prio_lo;
    c.prio_hi = parent->c.prio_hi;
    if (hipSetDevice(device) != hipSuccess || !create_events(c)) {
      delete x;
      return SPTR_ERR_HIP;
    }
  } else if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(c.stream.put(), hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(c.cap_stream.put(), hipStreamNonBlocking) != hipSuccess ||
      // the side streams at the lowest priority: a priority of its own puts a stream on a hardware
      // queue of its own, so that its launches can run beside the main sequence's.  (r05t: the main
      // streams at the highest priority instead of the default changed nothing, C3 and C5.)
      hipDeviceGetStreamPriorityRange(&c.prio_lo, &c.prio_hi) != hipSuccess ||
      hipStreamCreateWithPriority(c.side_stream.put(), hipStreamNonBlocking, c.prio_lo) != hipSuccess ||
      hipStreamCreateWithPriority(c.cap_side.put(), hipStreamNonBlocking, c.prio_lo) != hipSuccess ||
      hipStreamCreateWithPriority(c.side2_stream.put(), hipStreamNonBlocking, c.prio_lo) != hipSuccess ||
      hipStreamCreateWithPriority(c.cap_side2.put(), hipStreamNonBlocking, c.prio_lo) != hipSuccess ||
      !create_events(c)) {
    delete x;
    return SPTR_ERR_HIP;
  }
  int khz = 0;
  if (c.wb.seg.ensure(seg_table_bytes()) != hipSuccess || c.w_tot.ensure(kTotWords * 8) != hipSuccess ||
      c.dyn.ensure(kDynBytes) != hipSuccess || hipMemset(c.wb.seg.p, 0, seg_table_bytes()) != hipSuccess ||
      c.tslots.ensure((size_t)kTimeSlots * kTimeSlotWords * 8) != hipSuccess ||
      hipMemset(c.tslots.p, 0, (size_t)kTimeSlots * kTimeSlotWords * 8) != hipSuccess ||
      hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) {
    delete x;
    return SPTR_ERR_OOM;
  }
  c.wall_khz = khz;
  *out = x;
  return SPTR_OK;
}

int sptr_destroy(sptr_ctx* x) {
  if (!x) return SPTR_ERR_INVALID;
  delete x;  // (~sptr_ctx waits for the context's work first)
  return SPTR_OK;
}

const char* sptr_last_error(const sptr_ctx* x) { return x ? x->c.err.c_str() : "null context"; }

static int set_debug_mode_one(sptr_ctx* x, int mode) {
  if (!x) return SPTR_ERR_INVALID;
  x->c.debug_mode = mode;
  ++x->c.epoch;
  return SPTR_OK;
}

static int set_leaf_size_one(sptr_ctx* x, uint32_t n) {
  if (!x) return SPTR_ERR_INVALID;
  if (n > kMaxLeafSize) return fail(x->c, SPTR_ERR_INVALID, "leaf size must be 0 (automatic) or 1..16");
  x->c.leaf_size = n;
  ++x->c.epoch;
  return SPTR_OK;
}

static int set_tree_order_one(sptr_ctx* x, uint32_t mode) {
  if (!x) return SPTR_ERR_INVALID;
  if (mode > 1u) return fail(x->c, SPTR_ERR_INVALID, "tree order must be 0 (automatic) or 1 (Morton)");
  x->c.tree_order = mode;
  ++x->c.epoch;
  return SPTR_OK;
}

static int set_bvh_width_one(sptr_ctx* x, uint32_t width) {
  if (!x) return SPTR_ERR_INVALID;
  if (width != 0 && width != 2 && width != (uint32_t)kWide)
    return fail(x->c, SPTR_ERR_INVALID, "bvh width must be 0 (auto), 2 or " + std::to_string(kWide));
  x->c.bvh_width = width;
  ++x->c.epoch;
  return build_prim_materials(x->c);  // (the width decides whether the scene is staged: scene_view)
}

static int set_tail_depth_one(sptr_ctx* x, uint32_t depth) {
  if (!x) return SPTR_ERR_INVALID;
  if (depth > (uint32_t)kMaxDepth) return fail(x->c, SPTR_ERR_INVALID, "tail depth must be 0 (automatic) or 1..32");
  x->c.tail_depth = depth;
  ++x->c.epoch;
  return SPTR_OK;
}

static int set_bounce_chain_one(sptr_ctx* x, uint32_t mode) {
  if (!x) return SPTR_ERR_INVALID;
  if (mode > 2u) return fail(x->c, SPTR_ERR_INVALID, "bounce chain must be 0 (automatic), 1 (off) or 2 (on)");
  x->c.bounce_chain = mode;  // (part of the launch-graph key: sptr_render)
  return SPTR_OK;
}

static int set_sky_split_one(sptr_ctx* x, uint32_t mode, uint32_t bulk_threads) {
  if (!x) return SPTR_ERR_INVALID;
  if (mode > 2u) return fail(x->c, SPTR_ERR_INVALID, "sky split must be 0 (automatic), 1 (off) or 2 (on)");
  x->c.sky_split = mode;  // (both are part of the launch-graph key: sptr_render)
  x->c.sky_split_threads = bulk_threads;
  return SPTR_OK;
}

static int set_shadow_entries_one(sptr_ctx* x, uint32_t mode) {
  if (!x) return SPTR_ERR_INVALID;
  if (mode > 2u) return fail(x->c, SPTR_ERR_INVALID, "shadow entries must be 0 (off), 1 (automatic) or 2 (always)");
  if (x->c.shadow_mode != mode) ++x->c.epoch;  // (the table is part of the shading launches' arguments)
  x->c.shadow_mode = mode;
  return SPTR_OK;
}

static int set_split_refs_one(sptr_ctx* x, uint32_t max_pieces) {
  if (!x) return SPTR_ERR_INVALID;
  if (max_pieces == 0u) max_pieces = 1u;
  if (max_pieces > 32u || (max_pieces & (max_pieces - 1u)))
    return fail(x->c, SPTR_ERR_INVALID, "split references: 0 (default: 1, none) or a power of two up to 32");
  x->c.split_pieces = max_pieces;
  ++x->c.epoch;
  return SPTR_OK;
}

static int set_stragglers_one(sptr_ctx* x, uint32_t lanes) {
  if (!x) return SPTR_ERR_INVALID;
  if (lanes > 64u) return fail(x->c, SPTR_ERR_INVALID, "straggler lanes: 0 (no hand-off) to 64");
  x->c.strag_lanes = lanes;
  ++x->c.epoch;  // part of every captured launch sequence's arguments
  return SPTR_OK;
}

static int set_wave_paths_one(sptr_ctx* x, uint64_t max_paths) {
  if (!x) return SPTR_ERR_INVALID;
  if (max_paths > (1ull << 30)) return fail(x->c, SPTR_ERR_INVALID, "wave paths above 2^30");
  x->c.wave_paths = max_paths;
  ++x->c.epoch;
  return SPTR_OK;
}

static int upload_scene_one(sptr_ctx* x, const sptr_scene* s) {
  if (!x || !s) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;  // a pending render may still read the old state
  API_HIP(hipSetDevice(c.device));
  if ((s->num_tris && (!s->indices || !s->positions || !s->tri_geom_first)) || (s->num_spheres && !s->spheres) ||
      ((s->num_tri_geoms + s->num_spheres) && !s->geom_material))
    return fail(c, SPTR_ERR_INVALID, "scene: null array with nonzero count");
  // leaf links keep 32 - 1 - kLeafCountBits bits of range start
  if ((uint64_t)s->num_tris + s->num_spheres >= (1ull << (31 - kLeafCountBits)))
    return fail(c, SPTR_ERR_INVALID, "scene too large (at most 2^26 primitives)");
  if (s->num_tri_geoms && s->tri_geom_first[s->num_tri_geoms] != s->num_tris)
    return fail(c, SPTR_ERR_INVALID, "scene: tri_geom_first must end at num_tris");
  for (uint64_t i = 0; i < (uint64_t)s->num_tris * 3; ++i)
    if (s->indices[i] >= s->num_verts) return fail(c, SPTR_ERR_INVALID, "scene: vertex index out of range");
  std::vector<uint32_t> tg(s->num_tris);
  for (uint32_t g = 0; g < s->num_tri_geoms; ++g) {
    if (s->tri_geom_first[g] > s->tri_geom_first[g + 1]) return fail(c, SPTR_ERR_INVALID, "scene: geom offsets");
    for (uint32_t i = s->tri_geom_first[g]; i < s->tri_geom_first[g + 1]; ++i) tg[i] = g;
  }
  c.have_scene = false;
  c.prim_mat_n = 0u;
  c.num_tri_geoms = s->num_tri_geoms;
  c.geom_first.assign(s->tri_geom_first, s->tri_geom_first + (s->num_tri_geoms ? s->num_tri_geoms + 1 : 0));
  c.geom_material.assign(s->geom_material, s->geom_material + s->num_tri_geoms + s->num_spheres);
  const int rc = build_lbvh(c, s->positions, s->num_verts, s->indices, s->num_tris, s->spheres, s->num_spheres, tg.data(),
                            s->num_tri_geoms);
  if (rc != SPTR_OK) return rc;
  // sptr_set_signed_distance: the pseudonormal tables of this upload (the caller's context only; a scene whose
  // triangles belong to no geometry has none).  Off: nothing is allocated, launched or kept.
  if (c.signed_on && !x->is_lane && !(s->num_tris && !s->num_tri_geoms)) {
    const int rs = signed_build_upload(c, s->positions, s->num_verts, s->indices, s->num_tris, s->spheres, s->num_spheres,
                                       tg.data(), s->num_tri_geoms);
    if (rs != SPTR_OK) return rs;
  } else if (c.sg.valid || c.sg.cpos.p) {
    signed_release(c);
  }
  c.have_scene = true;
  ++c.epoch;
  ++c.geom_rev;
  ++c.upload_rev;
  return resolve_geom_materials(c);
}

int sptr_scene_info(const sptr_ctx* x, uint32_t* num_prims, uint32_t* num_nodes, uint32_t* depth, double* build_ms) {
  if (!x) return SPTR_ERR_INVALID;
  const Context& c = x->c;
  if (num_prims) *num_prims = c.num_tris + c.num_sph;
  if (num_nodes) *num_nodes = c.num_nodes;
  if (depth) *depth = c.bvh_depth;
  if (build_ms) *build_ms = c.build_ms;
  return SPTR_OK;
}

int sptr_scene_layout_info(const sptr_ctx* x, sptr_scene_layout* out) {
  if (!x || !out) return SPTR_ERR_INVALID;
  const Context& c = x->c;
  const SceneView sv = scene_view(c);
  out->num_tris = c.num_tris;
  out->num_spheres = c.num_sph;
  out->num_nodes = c.num_nodes;
  out->leaf_size = c.leaf_used;
  out->bvh_depth = c.bvh_depth;
  out->lds_bytes = sv.lds_bytes;
  out->bvh_width = sv.width;
  out->num_nodes = sv.width == (uint32_t)kWide ? c.num_nodes4 : c.num_nodes;
  out->node_bytes = sv.width == (uint32_t)kWide ? (uint64_t)c.num_nodes4 * sizeof(WideNode) : (uint64_t)c.num_nodes * sizeof(BvhNode);
  out->tri_bytes = (uint64_t)c.num_tri_refs * 48u;
  out->sphere_bytes = (uint64_t)c.num_sph * 16u;
  out->prim_ref_bytes = ((uint64_t)c.num_tri_refs + c.num_sph) * 4u;
  out->num_prim_refs = c.num_tri_refs + c.num_sph;
  return SPTR_OK;
}

static int set_materials_one(sptr_ctx* x, const sptr_material* m, uint32_t n) {
  if (!x || (n && !m)) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;  // a pending render may still read the old state
  if (n == 0) return fail(c, SPTR_ERR_INVALID, "at least one material is required");
  API_HIP(hipSetDevice(c.device));
  c.mats_host.resize(n);
  std::memcpy(c.mats_host.data(), m, sizeof(DevMaterial) * n);
  API_HIP(c.mats.ensure(sizeof(DevMaterial) * n));
  API_HIP(hipMemcpy(c.mats.p, c.mats_host.data(), sizeof(DevMaterial) * n, hipMemcpyHostToDevice));
  ++c.epoch;
  return resolve_geom_materials(c);
}

static int set_lights_one(sptr_ctx* x, const sptr_light* l, uint32_t n) {
  if (!x || (n && !l)) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (n > (uint32_t)kMaxLights) return fail(c, SPTR_ERR_INVALID, "too many lights");
  c.lights_host.resize(n);
  ++c.epoch;
  for (uint32_t i = 0; i < n; ++i) {
    DevLight& d = c.lights_host[i];
    d.type = l[i].type;
    if (l[i].type == 0) {  // DirectionalLight stores normalize(-direction) (Light.cpp:43-46)
      const vec3 v = normalize(-v3(l[i].v[0], l[i].v[1], l[i].v[2]));
      d.v[0] = v.x; d.v[1] = v.y; d.v[2] = v.z;
    } else if (l[i].type == 1) {
      d.v[0] = l[i].v[0]; d.v[1] = l[i].v[1]; d.v[2] = l[i].v[2];
    } else {
      return fail(c, SPTR_ERR_INVALID, "unknown light type");
    }
    const vec3 r = v3(l[i].color[0], l[i].color[1], l[i].color[2]) * l[i].intensity;
    d.radiance[0] = r.x; d.radiance[1] = r.y; d.radiance[2] = r.z;
    d.pad = 0.0f;
  }
  return SPTR_OK;
}

static int set_environment_one(sptr_ctx* x, const sptr_environment* e) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;  // a pending render may still read the old state
  API_HIP(hipSetDevice(c.device));
  if (!e || !e->faces) {
    c.env.release();
    ++c.epoch;
    c.env_size = 0;
    if (e) {
      c.env_intensity = e->intensity;
      c.env_clamp = e->max_clamp;
    }
    return SPTR_OK;
  }
  if (e->size < 2) return fail(c, SPTR_ERR_INVALID, "environment face size must be >= 2");
  // env_color indexes texels in 32 bits (24-bit row multiplies): 6 * S * S must stay below 2^32
  if (e->size > kMaxEnvSize) return fail(c, SPTR_ERR_INVALID, "environment face size must be <= 26754");
  const size_t texels = (size_t)6 * e->size * e->size;
  std::vector<float> tmp(texels * 4);
  for (size_t i = 0; i < texels; ++i) {
    tmp[i * 4 + 0] = e->faces[i * 3 + 0];
    tmp[i * 4 + 1] = e->faces[i * 3 + 1];
    tmp[i * 4 + 2] = e->faces[i * 3 + 2];
    tmp[i * 4 + 3] = 0.0f;
  }
  API_HIP(c.env.ensure(texels * 16));
  API_HIP(hipMemcpy(c.env.p, tmp.data(), texels * 16, hipMemcpyHostToDevice));
  c.env_size = e->size;
  ++c.epoch;
  c.env_intensity = e->intensity;
  c.env_clamp = e->max_clamp;
  return SPTR_OK;
}

static int render_one(sptr_ctx* x, const sptr_frame* f, void* stream, sptr_stats* stats) {
  if (!x || !f) return SPTR_ERR_INVALID;
  Context& c = x->c;
  API_HIP(hipSetDevice(c.device));
  if (!c.have_scene) return fail(c, SPTR_ERR_NO_SCENE, "render: no scene uploaded");
  if (shading(c).mats_host.empty()) return fail(c, SPTR_ERR_NO_SCENE, "render: no materials set");
  if (f->width <= 0 || f->height <= 0 || f->spp == 0 || f->max_depth == 0 || f->max_depth > (uint32_t)kMaxDepth ||
      f->frame_begin == 0)
    return fail(c, SPTR_ERR_INVALID, "render: bad frame parameters");
  if (f->integrator > SPTR_INTEGRATOR_OPTIX) return fail(c, SPTR_ERR_INVALID, "render: unknown integrator");
  if (f->integrator == SPTR_INTEGRATOR_PATHTRACER && f->samples_per_frame > 4096)
    return fail(c, SPTR_ERR_INVALID, "render: samples_per_frame above 4096");
  const int G = f->shard_count > 0 ? f->shard_count : 1, R = f->shard_count > 0 ? f->shard_rank : 0;
  if (R < 0 || R >= G) return fail(c, SPTR_ERR_INVALID, "render: shard_rank out of range");
  const int ntiles = ((f->width + kTile - 1) / kTile) * ((f->height + kTile - 1) / kTile);
  if (R >= ntiles) return fail(c, SPTR_ERR_INVALID, "render: more shards than tiles");
  if ((uint64_t)f->width * f->height > (1ull << 28)) return fail(c, SPTR_ERR_INVALID, "render: image too large");
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c.stream;
  if (c.pending && s != c.pending_stream)
    return fail(c, SPTR_ERR_INVALID, "render: asynchronous renders must stay on one stream until sptr_collect_stats");
  bool resized = false;
  int rc = ensure_pixels(c, f->width, f->height, G, R, s, resized);
  if (rc != SPTR_OK) return rc;
  const bool reset = f->frame_begin == 1;
  if (!reset && f->frame_begin != c.last_samples + 1)
    return fail(c, SPTR_ERR_INVALID, "render: frame_begin must continue the accumulation (last + 1) or be 1");
  const bool timing = (f->flags & SPTR_FRAME_TIMING) != 0;
  const bool trace_timing = (f->flags & SPTR_FRAME_TIMING_TRACE) != 0;
  const uint32_t total = f->frame_begin + f->spp - 1;
  if (c.seed_offset != 0u) {  // sptr_set_seed_offset
    if (f->integrator != SPTR_INTEGRATOR_WAVEFRONT)
      return fail(c, SPTR_ERR_INVALID, "render: a seed offset applies to SPTR_INTEGRATOR_WAVEFRONT only (sptr_set_seed_offset)");
    if ((uint64_t)c.seed_offset + f->frame_begin + f->spp - 1 > 0xFFFFFFFFull)
      return fail(c, SPTR_ERR_INVALID, "render: seed offset + frame_begin + spp - 1 overflows 32 bits");
  }
  GraphKey key{};
  key.epoch = c.epoch;
  key.frame = *f;
  key.frame.frame_begin = 0;
  key.frame.flags &= (SPTR_FRAME_TIMING | SPTR_FRAME_TIMING_TRACE | SPTR_FRAME_COUNT_VISITS | SPTR_FRAME_NO_RESOLVE |
                      SPTR_FRAME_NO_CULL | SPTR_FRAME_RECULL);
  uint32_t waves = 0;
  uint64_t samples = 0;
  if (f->integrator != SPTR_INTEGRATOR_WAVEFRONT) {
    if (c.pending == 0) API_HIP(hipMemsetAsync(c.w_tot.p, 0, kTotWords * 8, s));
    const uint32_t spf = f->integrator == SPTR_INTEGRATOR_PATHTRACER ? (f->samples_per_frame ? f->samples_per_frame : 4u) : 1u;
    rc = run_call(c, key, f->frame_begin, reset ? 1u : 0u, total, (uint64_t)frame_view(c, *f).valid * f->spp, nullptr,
                  timing || trace_timing, false, s,
                  [&](hipStream_t cs, StageTimer& tm) { return enqueue_path_per_thread(c, *f, cs, tm); }, waves);
    if (rc != SPTR_OK) return rc;
    samples = (uint64_t)frame_view(c, *f).valid * f->spp * spf;
  } else {
    uint64_t wave_paths = c.wave_paths;
    if (!wave_paths) {  // default: 2^29 paths, or what half of the free HBM holds (at least 2^24)
      wave_paths = kDefaultWavePaths;
      if (c.wb.cap < std::min<uint64_t>(wave_paths, (uint64_t)f->spp * c.P)) {  // would (re)allocate
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b) {
          const uint32_t hm = hrec_mult(scene_view(c));
          const uint64_t held = c.wb.cap ? c.wb.cap * wave_path_bytes(c.wb.L, c.wb.ts, hm) : 0ull;
          const uint32_t L = std::max<uint32_t>(1u, (uint32_t)shading(c).lights_host.size());
          // budget net of the streams' segment slack (worst case: pixel-major hit records, k <= spp)
          const double budget = ((double)free_b + (double)held) * kWaveMemFraction -
                                (double)wave_slack_bytes(L, task_stride(c), std::min<uint32_t>(f->spp, 1024u), hm);
          const uint64_t fit = budget > 0.0 ? (uint64_t)budget / wave_path_bytes(L, task_stride(c), hm) : 0ull;
          wave_paths = std::max<uint64_t>(1ull << 24, std::min<uint64_t>(wave_paths, fit));
        }
      }
    }
    uint32_t k = (uint32_t)std::max<uint64_t>(1, wave_paths / c.P);
    k = std::min<uint32_t>(k, f->spp);
    {
      // hit-record slack: k records per pixel slot only when some batch runs bounce 0 pixel-major
      FrameView probe = frame_view(c, *f);
      probe.k = k;
      bool pm = bounce0_pixel_major(scene_view(c), probe) != 0u;
      if (f->spp % k) {  // the call's last, partial batch
        probe.k = f->spp % k;
        pm = pm || bounce0_pixel_major(scene_view(c), probe) != 0u;
      }
      // hit-record segments hold twice the static shares when k_trace_dyn takes its rays from the per-XCD queues
      rc = ensure_wave(c, (uint64_t)k * c.P, (uint32_t)shading(c).lights_host.size(), task_stride(c), pm ? k : 1u,
                       hrec_mult(scene_view(c)));
      if (rc != SPTR_OK) return rc;
    }
    const int T = std::max(1, (int)(c.tail_depth ? c.tail_depth : auto_tail_depth((uint64_t)k * c.P, scene_view(c))));
    rc = refresh_shadow_entries(c, *f, s);  // (ahead of the key: a build bumps the epoch)
    if (rc != SPTR_OK) return rc;
    key.epoch = c.epoch;  // ensure_wave may have reallocated
    key.k = k;
    key.tail = (uint32_t)T;
    key.chain = c.bounce_chain;
    key.sky_split = c.sky_split;
    key.sky_split_threads = c.sky_split_threads;
    {  // what enqueue_wavefront decides for the call's first batch (sptr_sky_split_info)
      FrameView probe = frame_view(c, *f);
      probe.k = k;
      probe.pixel_major = bounce0_pixel_major(scene_view(c), probe);
      if (!(f->flags & SPTR_FRAME_NO_CULL)) probe.cull = static_cast<const uint32_t*>(c.cull.p);
      c.sky_split_last = sky_split_threads(c, scene_view(c), shade_view(c), probe);
    }
    if (c.pending == 0) API_HIP(hipMemsetAsync(c.w_tot.p, 0, kTotWords * 8, s));
    rc = refresh_cull(c, *f, s, timing || trace_timing);
    if (rc != SPTR_OK) return rc;
    // an in-sequence cull (SPTR_FRAME_RECULL) counts its unculled pixels from zero: k_frame_dyn clears it
    uint32_t* clear = ((f->flags & SPTR_FRAME_RECULL) && !(f->flags & SPTR_FRAME_NO_CULL))
                          ? static_cast<uint32_t*>(c.plist.p) + c.P : nullptr;
    // (the seeds' accumulation index: frame_begin + the seed offset, the k_frame_dyn word they read)
    rc = run_call(c, key, f->frame_begin + c.seed_offset, reset ? 1u : 0u, total, (uint64_t)frame_view(c, *f).valid * f->spp, clear,
                  timing || trace_timing, !timing, s,
                  [&](hipStream_t cs, StageTimer& tm) { return enqueue_wavefront(c, *f, k, T, cs, tm); }, waves);
    if (rc != SPTR_OK) return rc;
    if (clear) {  // the sequence just enqueued computes this camera's mask (keyed only once enqueued)
      c.cull_epoch = c.epoch;
      c.cull_cam = f->camera;
      c.cull_exact = cull_exact_for(c, scene_view(c), *f);
      c.cull_listed = c.sky_split_last != 0u;
      c.cull_depth = cull_depth_for(f->spp, c.cull_exact);
      ++c.pending_culls;
    }
    samples = (uint64_t)frame_view(c, *f).valid * f->spp;
  }
  c.last_samples = total;
  ++c.pending;
  c.pending_stream = s;
  c.pending_samples += samples;
  c.pending_waves += waves;
  if (f->flags & SPTR_FRAME_ASYNC) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return SPTR_OK;
  }
  return collect_pending(c, stats);
}

const char* sptr_capture_error(const sptr_ctx* x) { return x ? x->c.capture_error.c_str() : "null context"; }

int sptr_graph_info(const sptr_ctx* x, uint32_t* valid, uint32_t* nodes, uint32_t* edges, uint32_t* depth,
                    uint32_t* captures, int32_t* capture_status) {
  if (!x) return SPTR_ERR_INVALID;
  const GraphCache& g = x->c.graph;
  if (captures) *captures = x->c.captures;
  if (capture_status) *capture_status = x->c.capture_status;
  if (valid) *valid = g.valid ? 1u : 0u;
  if (nodes) *nodes = g.valid ? g.nodes : 0u;
  if (edges) *edges = g.valid ? g.edges : 0u;
  if (depth) *depth = g.valid ? g.depth : 0u;
  return SPTR_OK;
}

int sptr_overlap_probe(sptr_ctx* x, double* ms) {
  if (!x || !ms) return SPTR_ERR_INVALID;
  Context& c = x->c;
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  int rate_khz = 0;
  API_HIP(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c.device));
  if (rate_khz <= 0) return fail(c, SPTR_ERR_HIP, "overlap probe: no wall clock rate");
  const uint64_t ticks = (uint64_t)rate_khz / 5u;  // 200 us per spin
  DevEvent e0, e1, fk, jn;
  hipError_t err = hipSuccess;
  auto ck = [&](hipError_t e) {
    if (e != hipSuccess && err == hipSuccess) err = e;
  };
  ck(hipEventCreate(e0.put()));
  ck(hipEventCreate(e1.put()));
  ck(hipEventCreateWithFlags(fk.put(), hipEventDisableTiming));
  ck(hipEventCreateWithFlags(jn.put(), hipEventDisableTiming));
  if (err != hipSuccess) return fail(c, SPTR_ERR_HIP, std::string("overlap probe: ") + hipGetErrorString(err));
  const hipStream_t s = c.stream;
  launch_spin(ticks / 8u, s);  // warm the kernel
  ck(hipStreamSynchronize(s));
  const hipStream_t sides[3] = {nullptr, c.side_stream, c.side2_stream};
  for (int i = 0; i < 3; ++i) {
    const hipStream_t side = sides[i] ? sides[i] : s;
    ck(hipEventRecord(e0, s));
    if (side != s) {
      ck(hipEventRecord(fk, s));
      ck(hipStreamWaitEvent(side, fk, 0));
    }
    launch_spin(ticks, s);
    launch_spin(ticks, side);
    if (side != s) {
      ck(hipEventRecord(jn, side));
      ck(hipStreamWaitEvent(s, jn, 0));
    }
    ck(hipEventRecord(e1, s));
    ck(hipStreamSynchronize(s));
    float t = 0.0f;
    ck(hipEventElapsedTime(&t, e0, e1));
    ms[i] = t;
  }
  if (err != hipSuccess) return fail(c, SPTR_ERR_HIP, std::string("overlap probe: ") + hipGetErrorString(err));
  return SPTR_OK;
}

static int set_launch_mode_one(sptr_ctx* x, uint32_t mode) {
  if (!x) return SPTR_ERR_INVALID;
  if (mode > 3)
    return fail(x->c, SPTR_ERR_INVALID,
                "launch mode must be 0 (graphs where they pay), 1 (direct), 2 (direct, one stream) or 3 (graphs)");
  x->c.launch_mode = mode;
  return SPTR_OK;
}

int sptr_collect_stats(sptr_ctx* x, sptr_stats* stats) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  API_HIP(hipSetDevice(c.device));
  if (!x->lane || x->lane->c.pending == 0) return collect_pending(c, stats);
  Context* both[2] = {&c, &x->lane->c};
  const double busy = stats ? trace_busy_ms(both, 2) : 0.0;
  sptr_stats a{}, b{};
  int rc = collect_pending(c, &a);
  if (rc != SPTR_OK) return rc;
  rc = collect_pending(x->lane->c, &b);
  if (rc != SPTR_OK) return fail(c, rc, std::string("pixel lane: ") + x->lane->c.err);
  add_stats(a, b);
  a.ms_trace_busy = busy;
  if (stats) *stats = a;
  return SPTR_OK;
}

int sptr_read_rgb8(sptr_ctx* x, uint8_t* rgb) {
  if (!x || !rgb) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  if (x->split && sync_pending(x->lane->c) != SPTR_OK) return SPTR_ERR_HIP;  // (it resolves into this image)
  if (!c.image.p) return fail(c, SPTR_ERR_NO_SCENE, "read_rgb8: nothing rendered");
  API_HIP(hipSetDevice(c.device));
  // (the denoised image when the last call ran the denoise pass, sptr_set_denoise)
  API_HIP(hipMemcpy(rgb, x->dn.ran ? x->dn.image.p : c.image.p, (size_t)c.W * c.H * 3, hipMemcpyDeviceToHost));
  return SPTR_OK;
}

int sptr_read_rgb8_lagged(sptr_ctx* x, uint8_t* rgb, uint32_t* got) {
  if (!x || !rgb || !got) return SPTR_ERR_INVALID;
  Context& c = x->c;
  *got = 0;
  if (!c.image.p || c.pending == 0)
    return fail(c, SPTR_ERR_INVALID, "read_rgb8_lagged: call after an asynchronous render (SPTR_FRAME_ASYNC)");
  API_HIP(hipSetDevice(c.device));
  if (!x->copy_stream) {
    // a priority of its own (the lowest): its own hardware queue, apart from the render stream's
    API_HIP(hipStreamCreateWithPriority(x->copy_stream.put(), hipStreamNonBlocking, c.prio_lo));
    API_HIP(hipEventCreateWithFlags(x->copy_done.put(), hipEventDisableTiming));
    for (auto& sn : x->snap) API_HIP(hipEventCreateWithFlags(sn.ready.put(), hipEventDisableTiming));
  }
  const size_t bytes = (size_t)c.W * c.H * 3;
  auto& cur = x->snap[x->snap_cur];
  auto& prev = x->snap[x->snap_cur ^ 1u];
  // this call's image, snapshotted on its stream after it (with two lanes, the lane's resolve into this
  // image is joined into that stream before the call's last launch).  The slot's last reader was the copy
  // two calls back, which that call waited for.
  API_HIP(cur.buf.ensure(bytes));
  API_HIP(hipMemcpyAsync(cur.buf.p, x->dn.ran ? x->dn.image.p : c.image.p, bytes, hipMemcpyDeviceToDevice, c.pending_stream));
  API_HIP(hipEventRecord(cur.ready, c.pending_stream));
  if (prev.valid && prev.W == c.W && prev.H == c.H) {
    if (x->reg_ptr != rgb || x->reg_bytes != bytes) {  // page-lock the destination: the copy becomes a DMA
      if (x->reg_ptr) (void)hipHostUnregister(x->reg_ptr);
      x->reg_ptr = nullptr;
      x->reg_bytes = 0;
      if (hipHostRegister(rgb, bytes, hipHostRegisterDefault) == hipSuccess) {
        x->reg_ptr = rgb;
        x->reg_bytes = bytes;
      } else {
        (void)hipGetLastError();  // (a pageable destination works too, through staging)
      }
    }
    API_HIP(hipStreamWaitEvent(x->copy_stream, prev.ready, 0));
    API_HIP(hipMemcpyAsync(rgb, prev.buf.p, bytes, hipMemcpyDeviceToHost, x->copy_stream));
    API_HIP(hipEventRecord(x->copy_done, x->copy_stream));
    API_HIP(hipEventSynchronize(x->copy_done));
    *got = 1;
  }
  cur.valid = true;
  cur.W = c.W;
  cur.H = c.H;
  x->snap_cur ^= 1u;
  return SPTR_OK;
}

int sptr_read_accum(sptr_ctx* x, float* out) {
  if (!x || !out) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  if (!c.accum.p) return fail(c, SPTR_ERR_NO_SCENE, "read_accum: nothing rendered");
  API_HIP(hipSetDevice(c.device));
  std::vector<float> a((size_t)c.P * 4);
  API_HIP(hipMemcpy(a.data(), c.accum.p, a.size() * 4, hipMemcpyDeviceToHost));
  std::memset(out, 0, (size_t)c.W * c.H * 3 * 4);
  auto scatter = [&](const Context& cc, const std::vector<float>& acc) {
    for (uint32_t l = 0; l < cc.P; ++l) {
      int px, py;
      if (!host_local_pixel(cc, l, px, py)) continue;
      float* o = out + ((size_t)py * cc.W + px) * 3;
      o[0] = acc[(size_t)l * 4 + 0];
      o[1] = acc[(size_t)l * 4 + 1];
      o[2] = acc[(size_t)l * 4 + 2];
    }
  };
  scatter(c, a);
  if (x->split) {  // the odd half of the tiles, from the lane
    Context& cy = x->lane->c;
    if (sync_pending(cy) != SPTR_OK) return SPTR_ERR_HIP;
    std::vector<float> b((size_t)cy.P * 4);
    API_HIP(hipMemcpy(b.data(), cy.accum.p, b.size() * 4, hipMemcpyDeviceToHost));
    scatter(cy, b);
  }
  return SPTR_OK;
}

int sptr_tiles_device(sptr_ctx* x, void** dptr, size_t* bytes) {
  if (!x || !dptr || !bytes) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (!c.tiles.p) return fail(c, SPTR_ERR_NO_SCENE, "tiles_device: nothing rendered");
  if (x->split) {  // the two lanes' tiles, interleaved into this context's shard order by sptr_render
    *dptr = x->tiles_full.p;
    *bytes = (size_t)x->full_tiles * kTilePixels * 4;
    return SPTR_OK;
  }
  *dptr = c.tiles.p;
  *bytes = (size_t)c.P * 4;
  return SPTR_OK;
}

int sptr_unpack_tiles(sptr_ctx* x, const void* gathered, int32_t G, uint32_t tpr, int32_t W, int32_t H, void* out,
                      void* stream) {
  if (!x || !gathered || !out || G <= 0 || W <= 0 || H <= 0) return SPTR_ERR_INVALID;
  Context& c = x->c;
  API_HIP(hipSetDevice(c.device));
  const int ntiles = ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
  if ((uint64_t)tpr * (uint64_t)G < (uint64_t)ntiles) return fail(c, SPTR_ERR_INVALID, "unpack: tiles_per_rank too small");
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c.stream;
  launch_unpack(static_cast<const uint32_t*>(gathered), G, tpr, W, H, static_cast<uint8_t*>(out), s);
  API_HIP(hipGetLastError());
  if (!stream) API_HIP(hipStreamSynchronize(s));  // on a caller's stream the call only enqueues
  return SPTR_OK;
}

static int run_query(sptr_ctx* x, const float* rays, uint32_t n, bool anyhit, uint32_t* geom, uint32_t* prim, float* t,
                     float* ng, uint8_t* occ) {
  if (!x || (n && !rays)) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (!c.have_scene) return fail(c, SPTR_ERR_NO_SCENE, "query: no scene");
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  if (n == 0) return SPTR_OK;
  API_HIP(hipSetDevice(c.device));
  const size_t rb = (size_t)n * 32, refb = (size_t)n * 4, tb = (size_t)n * 4, nb = (size_t)n * 12, ob = (size_t)n;
  API_HIP(c.qbuf.ensure(rb + refb + tb + nb + ob + 64));
  char* base = static_cast<char*>(c.qbuf.p);
  uint32_t* d_sflag = reinterpret_cast<uint32_t*>(base + (rb + refb + tb + nb + ob + 15) / 16 * 16);
  float* d_rays = reinterpret_cast<float*>(base);
  uint32_t* d_ref = reinterpret_cast<uint32_t*>(base + rb);
  float* d_t = reinterpret_cast<float*>(base + rb + refb);
  float* d_ng = reinterpret_cast<float*>(base + rb + refb + tb);
  uint8_t* d_occ = reinterpret_cast<uint8_t*>(base + rb + refb + tb + nb);
  API_HIP(hipMemcpy(d_rays, rays, rb, hipMemcpyHostToDevice));
  API_HIP(hipMemset(d_sflag, 0, 4));
  launch_query(scene_view(c), static_cast<const uint32_t*>(c.tri_orig.p), static_cast<const uint32_t*>(c.sph_orig.p),
               d_rays, n, anyhit, d_ref, d_t, d_ng, d_occ, d_sflag, c.stream);
  API_HIP(hipGetLastError());
  API_HIP(hipStreamSynchronize(c.stream));
  uint32_t sflag = 0;
  API_HIP(hipMemcpy(&sflag, d_sflag, 4, hipMemcpyDeviceToHost));
  if (sflag) return fail(c, SPTR_ERR_HIP, "query: BVH traversal stack overflow (internal error)");
  if (anyhit) {
    API_HIP(hipMemcpy(occ, d_occ, ob, hipMemcpyDeviceToHost));
    return SPTR_OK;
  }
  std::vector<uint32_t> ref(n);
  API_HIP(hipMemcpy(ref.data(), d_ref, refb, hipMemcpyDeviceToHost));
  API_HIP(hipMemcpy(t, d_t, tb, hipMemcpyDeviceToHost));
  API_HIP(hipMemcpy(ng, d_ng, nb, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = ref[i];
    if (r == kNoHit) {
      geom[i] = prim[i] = 0xFFFFFFFFu;
    } else if (r & kSphereBit) {
      geom[i] = c.num_tri_geoms + (r & kIndexMask);
      prim[i] = 0;
    } else {
      const uint32_t tri = r & kIndexMask;
      const auto it = std::upper_bound(c.geom_first.begin(), c.geom_first.end(), tri);
      const uint32_t g = (uint32_t)(it - c.geom_first.begin()) - 1u;
      geom[i] = g;
      prim[i] = tri - c.geom_first[g];
    }
  }
  return SPTR_OK;
}

int sptr_intersect(sptr_ctx* x, const float* rays, uint32_t n, uint32_t* geom, uint32_t* prim, float* t, float* ng) {
  if (!geom || !prim || !t || !ng) return SPTR_ERR_INVALID;
  return run_query(x, rays, n, false, geom, prim, t, ng, nullptr);
}

int sptr_occluded(sptr_ctx* x, const float* rays, uint32_t n, uint8_t* occ) {
  if (!occ) return SPTR_ERR_INVALID;
  return run_query(x, rays, n, true, nullptr, nullptr, nullptr, nullptr, occ);
}

// ---- ray queries on caller buffers -----------------------------------------------------------------
constexpr uint32_t kQueryMaxRays = 1u << 28;
constexpr uint32_t kQueryFlags = SPTR_QUERY_ANY_HIT | SPTR_QUERY_DEVICE_PTRS | SPTR_QUERY_SORT | SPTR_QUERY_NO_SORT;
// Order of a query that sets neither sort flag.  The rule: sort scenes that are not staged
// into LDS from the smallest batch at which keys + sort + sorted trace beat the unsorted trace by more than
// the measured spread.  No such batch size has been measured, so the default never sorts.
static bool query_sorts_by_default(const SceneView&, uint32_t) { return false; }

// the triangle list's geomID offsets on the device (k_aov and k_rayquery derive primIDs from them)
static int ensure_geom_first(sptr_ctx* x) {
  Context& c = x->c;
  if (x->geom_first_valid) return SPTR_OK;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  API_HIP(x->geom_first.ensure((c.geom_first.size() + 1) * 4));
  if (!c.geom_first.empty())
    API_HIP(hipMemcpy(x->geom_first.p, c.geom_first.data(), c.geom_first.size() * 4, hipMemcpyHostToDevice));
  x->geom_first_valid = true;
  return SPTR_OK;
}

// the last query of every kind, on whichever stream it was enqueued
static int query_wait(sptr_ctx* x) {
  Context& c = x->c;
  API_HIP(x->wait_queries());
  return SPTR_OK;
}

// after the last query completed: its traversal-stack-overflow flag (sticky on the device; cleared once reported)
static int query_check_flag(sptr_ctx* x) {
  Context& c = x->c;
  if (!x->rq.flag.p) return SPTR_OK;
  uint32_t sflag = 0;
  API_HIP(hipMemcpy(&sflag, x->rq.flag.p, 4, hipMemcpyDeviceToHost));
  if (!sflag) return SPTR_OK;
  API_HIP(hipMemset(x->rq.flag.p, 0, 4));
  return fail(c, SPTR_ERR_HIP, "query: BVH traversal stack overflow (internal error)");
}

// What every enqueued batch needs first: the overflow flag, the geomID offsets, and, for a sorted batch of n rays or
// points, scratch for the keys, the indices and the radix sort (shared by every kind).
static int query_scratch(sptr_ctx* x, uint32_t n, bool sort, hipStream_t s) {
  Context& c = x->c;
  auto& rq = x->rq;
  if (!rq.flag.p) {
    API_HIP(rq.flag.ensure(16));
    API_HIP(hipMemset(rq.flag.p, 0, 16));
  }
  const int rg = ensure_geom_first(x);
  if (rg != SPTR_OK) return rg;
  if (sort) {
    size_t temp_bytes = 0;
    API_HIP(radix_sort_pairs_u64(nullptr, temp_bytes, nullptr, nullptr, nullptr, nullptr, n, s));
    const size_t kb = (size_t)n * 8, ib = (size_t)n * 4;
    if (rq.keys.bytes < kb || rq.keys_sorted.bytes < kb || rq.index.bytes < ib || rq.order.bytes < ib ||
        rq.temp.bytes < temp_bytes) {
      const int rw = query_wait(x);  // an enqueued query may still use the old scratch
      if (rw != SPTR_OK) return rw;
      API_HIP(rq.keys.ensure(kb));
      API_HIP(rq.keys_sorted.ensure(kb));
      API_HIP(rq.index.ensure(ib));
      API_HIP(rq.order.ensure(ib));
      API_HIP(rq.temp.ensure(temp_bytes));
    }
  }
  return SPTR_OK;
}

// launch_ray_keys / launch_point_keys
using KeyLauncher = void (*)(const SceneView&, const float4*, uint32_t, uint64_t*, uint32_t*, hipStream_t);

// The sort phase on s: the kind's keys, radix sort; the kind's launch then reads rq.order.
static int query_sort(sptr_ctx* x, const SceneView& sv, KeyLauncher keys, const float4* in, uint32_t n, hipStream_t s) {
  Context& c = x->c;
  auto& rq = x->rq;
  keys(sv, in, n, static_cast<uint64_t*>(rq.keys.p), static_cast<uint32_t*>(rq.index.p), s);
  API_HIP(hipGetLastError());
  size_t tb = rq.temp.bytes;
  API_HIP(radix_sort_pairs_u64(rq.temp.p, tb, static_cast<const uint64_t*>(rq.keys.p),
                               static_cast<uint64_t*>(rq.keys_sorted.p), static_cast<const uint32_t*>(rq.index.p),
                               static_cast<uint32_t*>(rq.order.p), n, s));
  return SPTR_OK;
}

// The head of every enqueued batch (in: its n rays or points) on s: the run's events, created on first use; the order
// (sort_default: the kind's choice for a query that sets neither sort flag); the shared scratch; the begin event;
// and, for a sorted batch, the sort phase and its event.  *order is what the kind's view takes: null when unsorted.
static int query_begin(sptr_ctx* x, sptr_ctx::QueryRun& run, const SceneView& sv, uint32_t flags, bool sort_default,
                       KeyLauncher keys, const float4* in, uint32_t n, hipStream_t s, const uint32_t** order) {
  Context& c = x->c;
  const bool sort = (flags & SPTR_QUERY_SORT) != 0u ||
                    ((flags & SPTR_QUERY_NO_SORT) == 0u && sv.lds_bytes == 0u && sort_default);
  for (DevEvent& e : run.ev)
    if (!e) API_HIP(hipEventCreate(e.put()));
  const int rs = query_scratch(x, n, sort, s);
  if (rs != SPTR_OK) return rs;
  API_HIP(hipEventRecord(run.ev[0], s));
  *order = nullptr;
  if (sort) {
    const int rk = query_sort(x, sv, keys, in, n, s);
    if (rk != SPTR_OK) return rk;
    API_HIP(hipEventRecord(run.ev[1], s));
    *order = static_cast<const uint32_t*>(x->rq.order.p);
  }
  return SPTR_OK;
}

// The tail, right after the kind's launch: the run counts as issued only once its end event is recorded.
static int query_end(sptr_ctx* x, sptr_ctx::QueryRun& run, bool sorted, hipStream_t s) {
  Context& c = x->c;
  API_HIP(hipGetLastError());
  API_HIP(hipEventRecord(run.ev[2], s));
  run.issued = true;
  run.sorted = sorted;
  ++run.count;
  return SPTR_OK;
}

// The checks every kind makes, in three parts: a kind's own checks come between them, and the order is behaviour (a
// call with several defects reports the first).  who: the function's name in the messages; noun: "rays" / "points".
static int query_refuse(sptr_ctx* x, int code, const char* who, const std::string& what) {
  return fail(x->c, code, std::string(who) + ": " + what);
}

static int check_query_flags(sptr_ctx* x, const char* who, uint32_t flags, uint32_t allowed, const char* unknown) {
  if (x->is_lane) return query_refuse(x, SPTR_ERR_INVALID, who, "not on a lane context");
  if (flags & ~allowed) return query_refuse(x, SPTR_ERR_INVALID, who, unknown);
  if ((flags & SPTR_QUERY_SORT) && (flags & SPTR_QUERY_NO_SORT))
    return query_refuse(x, SPTR_ERR_INVALID, who, "SPTR_QUERY_SORT and SPTR_QUERY_NO_SORT exclude each other");
  return SPTR_OK;
}

static int check_query_batch(sptr_ctx* x, const char* who, const char* noun, uint32_t n, const void* in) {
  if (n > kQueryMaxRays) return query_refuse(x, SPTR_ERR_INVALID, who, std::string("more than 2^28 ") + noun);
  if (n && !in) return query_refuse(x, SPTR_ERR_INVALID, who, std::string("no ") + noun);
  return SPTR_OK;
}

// misaligned: of the device pointers the kind checks; alignment: its rule, as the message states it
static int check_query_placement(sptr_ctx* x, const char* who, bool dev, const void* stream, bool misaligned,
                                 const char* alignment) {
  if (!dev && stream) return query_refuse(x, SPTR_ERR_INVALID, who, "host pointers cannot be enqueued on a stream");
  if (dev && misaligned) return query_refuse(x, SPTR_ERR_INVALID, who, alignment);
  if (!x->c.have_scene) return query_refuse(x, SPTR_ERR_NO_SCENE, who, "no scene");
  return SPTR_OK;
}

// One output of a host-pointer query: the caller's array, the pointer member of the device-side copy of the query
// struct that takes the staged address, the array's bytes, and whether it is staged though the caller passes NULL.
struct StageField {
  void* host;
  void* member;
  size_t bytes;
  bool always = false;
};
constexpr int kStageMaxFields = 10;

// Host pointers: the input goes to rq.stage_in and every output that is taken gets its place in rq.stage_out
// (query_stage.h); the members of the device-side copy point there afterwards, those of the other outputs stay NULL.
static int stage_query(sptr_ctx* x, const void* in, void* in_member, size_t in_bytes, const StageField* f, int k) {
  Context& c = x->c;
  auto& rq = x->rq;
  if (k > kStageMaxFields) return fail(c, SPTR_ERR_INVALID, "query: more staged fields than kStageMaxFields (internal error)");
  size_t bytes[kStageMaxFields], offset[kStageMaxFields];
  for (int i = 0; i < k; ++i) bytes[i] = f[i].host || f[i].always ? f[i].bytes : 0;
  const size_t total = stage_layout(bytes, k, offset);
  API_HIP(rq.stage_in.ensure(in_bytes));
  API_HIP(rq.stage_out.ensure(total));
  API_HIP(hipMemcpy(rq.stage_in.p, in, in_bytes, hipMemcpyHostToDevice));
  std::memcpy(in_member, &rq.stage_in.p, sizeof(void*));
  for (int i = 0; i < k; ++i) {
    void* p = f[i].host || f[i].always ? static_cast<char*>(rq.stage_out.p) + offset[i] : nullptr;
    std::memcpy(f[i].member, &p, sizeof p);
  }
  return SPTR_OK;
}

// ... and back, once the query completed: the outputs the caller takes
static int stage_copy_back(sptr_ctx* x, const StageField* f, int k) {
  Context& c = x->c;
  for (int i = 0; i < k; ++i) {
    if (!f[i].host) continue;
    void* p = nullptr;
    std::memcpy(&p, f[i].member, sizeof p);
    API_HIP(hipMemcpy(f[i].host, p, f[i].bytes, hipMemcpyDeviceToHost));
  }
  return SPTR_OK;
}

// The synchronous call of every kind, after its checks: waits for the pending render and the last queries, stages
// host pointers (in_member, f: into the copy of the query struct that `enqueue` passes on), enqueues on the
// context's stream, waits, reports a traversal-stack overflow and copies the staged outputs back.
extern "C++" {  // (a template, within this file's extern "C")
template <class Enqueue>
static int query_sync(sptr_ctx* x, bool dev, const void* in, void* in_member, size_t in_bytes, const StageField* f,
                      int k, Enqueue enqueue) {
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  const int rw = query_wait(x);
  if (rw != SPTR_OK) return rw;
  if (!dev) {
    const int rs = stage_query(x, in, in_member, in_bytes, f, k);
    if (rs != SPTR_OK) return rs;
  }
  const int rc = enqueue();
  if (rc != SPTR_OK) return rc;
  API_HIP(hipStreamSynchronize(c.stream));
  const int rf = query_check_flag(x);
  if (rf != SPTR_OK) return rf;
  return dev ? SPTR_OK : stage_copy_back(x, f, k);
}
}  // extern "C++"

// What the info call of every kind reports of its last run, into the caller's outputs (each may be NULL): waits for
// the run's end event; device ms of the sort phase (0 when unsorted) and of what followed it, sorted (0 / 1), runs.
static int query_run_info(sptr_ctx* x, const sptr_ctx::QueryRun& run, double* ms_sort, double* ms_main,
                          uint32_t* sorted, uint32_t* queries) {
  Context& c = x->c;
  double ms_s = 0.0, ms_m = 0.0;
  if (run.issued) {
    API_HIP(hipSetDevice(c.device));
    API_HIP(hipEventSynchronize(run.ev[2]));
    float ms = 0.0f;
    if (run.sorted) {
      API_HIP(hipEventElapsedTime(&ms, run.ev[0], run.ev[1]));
      ms_s = ms;
    }
    API_HIP(hipEventElapsedTime(&ms, run.sorted ? run.ev[1] : run.ev[0], run.ev[2]));
    ms_m = ms;
  }
  if (ms_sort) *ms_sort = ms_s;
  if (ms_main) *ms_main = ms_m;
  if (sorted) *sorted = run.issued && run.sorted ? 1u : 0u;
  if (queries) *queries = run.count;
  return SPTR_OK;
}

// One validated batch with device pointers, enqueued on s: [keys, radix sort,] trace.
static int enqueue_query(sptr_ctx* x, const sptr_ray_query& q, hipStream_t s) {
  Context& c = x->c;
  const SceneView sv = scene_view(c);
  const bool any = (q.flags & SPTR_QUERY_ANY_HIT) != 0u;
  RayQueryView v{};
  v.rays = reinterpret_cast<const float4*>(q.rays);
  v.n = q.n;
  const int rb = query_begin(x, x->rq.run, sv, q.flags, query_sorts_by_default(sv, q.n), launch_ray_keys, v.rays, q.n,
                             s, &v.order);
  if (rb != SPTR_OK) return rb;
  if (any) {
    v.occ = q.occluded;
  } else {
    v.geom = q.geom;
    v.prim = q.prim;
    v.t = q.t;
    v.ng = q.ng;
    v.uv = q.uv;
  }
  v.tri_orig = static_cast<const uint32_t*>(c.tri_orig.p);
  v.geom_first = static_cast<const uint32_t*>(x->geom_first.p);
  v.stack_overflow = static_cast<uint32_t*>(x->rq.flag.p);
  launch_rayquery(sv, v, any, s);
  return query_end(x, x->rq.run, v.order != nullptr, s);
}

int sptr_query_rays(sptr_ctx* x, const sptr_ray_query* q, void* stream) {
  if (!x || !q) return SPTR_ERR_INVALID;
  Context& c = x->c;
  const char* who = "query_rays";
  const bool any = (q->flags & SPTR_QUERY_ANY_HIT) != 0u, dev = (q->flags & SPTR_QUERY_DEVICE_PTRS) != 0u;
  int rc = check_query_flags(x, who, q->flags, kQueryFlags, "unknown flags");
  if (rc == SPTR_OK) rc = check_query_batch(x, who, "rays", q->n, q->rays);
  if (rc != SPTR_OK) return rc;
  if (any && !q->occluded) return fail(c, SPTR_ERR_INVALID, "query_rays: SPTR_QUERY_ANY_HIT needs the occluded output");
  rc = check_query_placement(x, who, dev, stream, (reinterpret_cast<uintptr_t>(q->rays) & 15u) != 0u,
                             "the device ray buffer must be 16-byte aligned");
  if (rc != SPTR_OK) return rc;
  if (q->n == 0u) return SPTR_OK;
  API_HIP(hipSetDevice(c.device));
  if (stream) return enqueue_query(x, *q, static_cast<hipStream_t>(stream));  // on a caller's stream the call only enqueues
  sptr_ray_query d = *q;
  const size_t n = q->n;
  const StageField out[] = {{q->geom, &d.geom, n * 4}, {q->prim, &d.prim, n * 4},
                            {q->t, &d.t, n * 4},       {q->ng, &d.ng, n * 12},
                            {q->uv, &d.uv, n * 8},     {q->occluded, &d.occluded, n}};
  return query_sync(x, dev, q->rays, &d.rays, n * 32, any ? out + 5 : out, any ? 1 : 5,
                    [&] { return enqueue_query(x, d, c.stream); });
}

int sptr_query_info(sptr_ctx* x, double* ms_sort, double* ms_trace, uint32_t* sorted, uint32_t* queries) {
  if (!x) return SPTR_ERR_INVALID;
  const int ri = query_run_info(x, x->rq.run, ms_sort, ms_trace, sorted, queries);
  if (ri != SPTR_OK) return ri;
  return x->rq.run.issued ? query_check_flag(x) : SPTR_OK;
}

// ---- multi-hit ray queries ----------------------------------------------------------------------------
constexpr uint32_t kMultiHitFlags = SPTR_QUERY_DEVICE_PTRS | SPTR_QUERY_SORT | SPTR_QUERY_NO_SORT;

// One validated batch with device pointers, enqueued on s: [keys, radix sort,] trace.
static int enqueue_multi_hit(sptr_ctx* x, const sptr_multi_hit_query& q, hipStream_t s) {
  Context& c = x->c;
  auto& mh = x->mh;
  const SceneView sv = scene_view(c);
  RayMultiView v{};
  v.rays = reinterpret_cast<const float4*>(q.rays);
  v.n = q.n;
  const int rb = query_begin(x, mh.run, sv, q.flags, query_sorts_by_default(sv, q.n), launch_ray_keys, v.rays, q.n, s,
                             &v.order);
  if (rb != SPTR_OK) return rb;
  v.k = q.max_hits;
  v.count = q.count;
  v.geom = q.geom;
  v.prim = q.prim;
  v.t = q.t;
  v.ng = q.ng;
  v.uv = q.uv;
  v.tri_orig = static_cast<const uint32_t*>(c.tri_orig.p);
  v.geom_first = static_cast<const uint32_t*>(x->geom_first.p);
  v.stack_overflow = static_cast<uint32_t*>(x->rq.flag.p);
  launch_rayquery_multi(sv, v, s, &mh.list_capacity, &mh.lds_bytes);
  return query_end(x, mh.run, v.order != nullptr, s);
}

int sptr_query_multi_hit(sptr_ctx* x, const sptr_multi_hit_query* q, void* stream) {
  if (!x || !q) return SPTR_ERR_INVALID;
  Context& c = x->c;
  const char* who = "query_multi_hit";
  const bool dev = (q->flags & SPTR_QUERY_DEVICE_PTRS) != 0u;
  int rc = check_query_flags(x, who, q->flags, kMultiHitFlags, "SPTR_QUERY_ANY_HIT or unknown flags");
  if (rc != SPTR_OK) return rc;
  if (q->max_hits < 1u || q->max_hits > (uint32_t)SPTR_MULTI_HIT_MAX)
    return fail(c, SPTR_ERR_INVALID, "query_multi_hit: max_hits must be 1 .. SPTR_MULTI_HIT_MAX");
  if (q->n > kQueryMaxRays || (uint64_t)q->n * q->max_hits > kQueryMaxRays)
    return fail(c, SPTR_ERR_INVALID, "query_multi_hit: more than 2^28 rays or hit slots");
  rc = check_query_batch(x, who, "rays", q->n, q->rays);
  if (rc != SPTR_OK) return rc;
  if (q->n && !q->count) return fail(c, SPTR_ERR_INVALID, "query_multi_hit: the count output is required");
  if (q->pad || q->reserved[0] || q->reserved[1] || q->reserved[2] || q->reserved[3])
    return fail(c, SPTR_ERR_INVALID, "query_multi_hit: pad and reserved must be 0");
  rc = check_query_placement(x, who, dev, stream, (reinterpret_cast<uintptr_t>(q->rays) & 15u) != 0u,
                             "the device ray buffer must be 16-byte aligned");
  if (rc != SPTR_OK) return rc;
  if (q->n == 0u) return SPTR_OK;
  API_HIP(hipSetDevice(c.device));
  if (stream) return enqueue_multi_hit(x, *q, static_cast<hipStream_t>(stream));  // only enqueues
  sptr_multi_hit_query d = *q;
  const size_t n = q->n, m = n * q->max_hits;
  const StageField out[] = {{q->count, &d.count, n * 4}, {q->geom, &d.geom, m * 4},
                            {q->prim, &d.prim, m * 4},   {q->t, &d.t, m * 4},
                            {q->ng, &d.ng, m * 12},      {q->uv, &d.uv, m * 8}};
  return query_sync(x, dev, q->rays, &d.rays, n * 32, out, 6, [&] { return enqueue_multi_hit(x, d, c.stream); });
}

int sptr_multi_hit_info(sptr_ctx* x, double* ms_sort, double* ms_trace, uint32_t* sorted, uint32_t* queries,
                        uint32_t* list_capacity, uint32_t* lds_bytes) {
  if (!x) return SPTR_ERR_INVALID;
  auto& mh = x->mh;
  const int ri = query_run_info(x, mh.run, ms_sort, ms_trace, sorted, queries);
  if (ri != SPTR_OK) return ri;
  if (list_capacity) *list_capacity = mh.list_capacity;
  if (lds_bytes) *lds_bytes = mh.lds_bytes;
  return mh.run.issued ? query_check_flag(x) : SPTR_OK;
}

// ---- closest-point queries ----------------------------------------------------------------------------
constexpr uint32_t kPointFlags = SPTR_QUERY_DEVICE_PTRS | SPTR_QUERY_SORT | SPTR_QUERY_NO_SORT | SPTR_POINT_COUNT;
// Order of a point query that sets neither sort flag: §6d's rule.  No batch size at which keys + sort + sorted walk
// beat the unsorted walk by more than the spread has been measured, so the default never sorts.
static bool points_sort_by_default(const SceneView&, uint32_t) { return false; }

// One validated batch with device pointers, enqueued on s: [keys, radix sort,] walk.
static int enqueue_points(sptr_ctx* x, const sptr_point_query& q, hipStream_t s) {
  Context& c = x->c;
  auto& pq = x->pq;
  const SceneView sv = scene_view(c);
  const bool count = (q.flags & SPTR_POINT_COUNT) != 0u;
  if (count) {
    if (!pq.counters.p) {
      const int rw = query_wait(x);
      if (rw != SPTR_OK) return rw;
      API_HIP(pq.counters.ensure(16));
    }
    API_HIP(hipMemsetAsync(pq.counters.p, 0, 16, s));
  }
  PointQueryView v{};
  v.points = reinterpret_cast<const float4*>(q.points);
  v.n = q.n;
  const int rb = query_begin(x, pq.run, sv, q.flags, points_sort_by_default(sv, q.n), launch_point_keys, v.points, q.n,
                             s, &v.order);
  if (rb != SPTR_OK) return rb;
  v.geom = q.geom;
  v.prim = q.prim;
  v.dist2 = q.dist2;
  v.dist = q.dist;
  v.point = q.point;
  v.uv = q.uv;
  v.ng = q.ng;
  v.tri_orig = static_cast<const uint32_t*>(c.tri_orig.p);
  v.geom_first = static_cast<const uint32_t*>(x->geom_first.p);
  v.stack_overflow = static_cast<uint32_t*>(x->rq.flag.p);
  v.counters = count ? static_cast<unsigned long long*>(pq.counters.p) : nullptr;
  launch_pointquery(sv, v, s, &pq.lds_bytes);
  const int re = query_end(x, pq.run, v.order != nullptr, s);
  if (re == SPTR_OK) pq.counted = count;
  return re;
}

// a device point query's input must be 16-byte aligned, its outputs 4-byte aligned
static bool point_query_misaligned(const sptr_point_query& q) {
  uintptr_t outs = 0;
  for (const void* p : std::initializer_list<const void*>{q.geom, q.prim, q.dist2, q.dist, q.point, q.uv, q.ng})
    outs |= reinterpret_cast<uintptr_t>(p);
  return (reinterpret_cast<uintptr_t>(q.points) & 15u) != 0u || (outs & 3u) != 0u;
}
constexpr const char* kPointAlignment = "the device point buffer must be 16-byte aligned, the outputs 4-byte aligned";

// the seven outputs of a point query (q: the caller's, d: the device-side copy); ids: staged whether or not taken
static void point_stage_fields(const sptr_point_query& q, sptr_point_query& d, bool ids, StageField* f) {
  const size_t n = q.n;
  f[0] = {q.geom, &d.geom, n * 4, ids};
  f[1] = {q.prim, &d.prim, n * 4, ids};
  f[2] = {q.dist2, &d.dist2, n * 4};
  f[3] = {q.dist, &d.dist, n * 4};
  f[4] = {q.point, &d.point, n * 12};
  f[5] = {q.uv, &d.uv, n * 8};
  f[6] = {q.ng, &d.ng, n * 12};
}

int sptr_query_points(sptr_ctx* x, const sptr_point_query* q, void* stream) {
  if (!x || !q) return SPTR_ERR_INVALID;
  Context& c = x->c;
  const char* who = "query_points";
  const bool dev = (q->flags & SPTR_QUERY_DEVICE_PTRS) != 0u;
  int rc = check_query_flags(x, who, q->flags, kPointFlags, "SPTR_QUERY_ANY_HIT or unknown flags");
  if (rc == SPTR_OK) rc = check_query_batch(x, who, "points", q->n, q->points);
  if (rc != SPTR_OK) return rc;
  if (q->reserved[0] || q->reserved[1] || q->reserved[2] || q->reserved[3])
    return fail(c, SPTR_ERR_INVALID, "query_points: reserved must be 0");
  rc = check_query_placement(x, who, dev, stream, point_query_misaligned(*q), kPointAlignment);
  if (rc != SPTR_OK) return rc;
  if (q->n == 0u) return SPTR_OK;
  API_HIP(hipSetDevice(c.device));
  if (stream) return enqueue_points(x, *q, static_cast<hipStream_t>(stream));  // only enqueues
  sptr_point_query d = *q;
  StageField out[7];
  point_stage_fields(*q, d, false, out);
  return query_sync(x, dev, q->points, &d.points, (size_t)q->n * 16, out, 7,
                    [&] { return enqueue_points(x, d, c.stream); });
}

int sptr_point_query_info(sptr_ctx* x, double* ms_sort, double* ms_walk, uint32_t* sorted, uint32_t* queries,
                          uint64_t* node_visits, uint64_t* prim_tests) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  auto& pq = x->pq;
  const int ri = query_run_info(x, pq.run, ms_sort, ms_walk, sorted, queries);
  if (ri != SPTR_OK) return ri;
  uint64_t cnt[2] = {0, 0};
  if (pq.run.issued && pq.counted) API_HIP(hipMemcpy(cnt, pq.counters.p, 16, hipMemcpyDeviceToHost));
  if (node_visits) *node_visits = cnt[0];
  if (prim_tests) *prim_tests = cnt[1];
  return pq.run.issued ? query_check_flag(x) : SPTR_OK;
}

// ---- signed distance queries ----------------------------------------------------------------------------
int sptr_set_signed_distance(sptr_ctx* x, uint32_t on) {
  if (!x) return SPTR_ERR_INVALID;
  if (x->is_lane) return fail(x->c, SPTR_ERR_INVALID, "set_signed_distance: not on a lane context");
  x->c.signed_on = on != 0u;  // read by the next upload
  return SPTR_OK;
}

// One validated batch with device pointers, enqueued on s: the point query as it is, then the sign pass.
static int enqueue_signed(sptr_ctx* x, const sptr_signed_query& q, hipStream_t s) {
  Context& c = x->c;
  auto& sq = x->sq;
  const SignedState& g = c.sg;
  sptr_point_query d = q.q;
  d.flags &= ~(uint32_t)SPTR_SIGNED_FLIP_TRIANGLES;
  for (DevEvent& e : sq.run.ev)
    if (!e) API_HIP(hipEventCreate(e.put()));
  if (!d.geom || !d.prim) {  // the ids go into scratch
    const size_t nb = (size_t)d.n * 4;
    if (sq.geom.bytes < nb || sq.prim.bytes < nb) {
      const int rw = query_wait(x);  // an enqueued query may still use the old scratch
      if (rw != SPTR_OK) return rw;
      API_HIP(sq.geom.ensure(nb));
      API_HIP(sq.prim.ensure(nb));
    }
    if (!d.geom) d.geom = static_cast<uint32_t*>(sq.geom.p);
    if (!d.prim) d.prim = static_cast<uint32_t*>(sq.prim.p);
  }
  const int rc = enqueue_points(x, d, s);
  if (rc != SPTR_OK) return rc;
  PointSignView v{};
  v.points = reinterpret_cast<const float4*>(d.points);
  v.n = d.n;
  v.geom = d.geom;
  v.prim = d.prim;
  v.signed_dist = q.signed_dist;
  v.normal = q.normal;
  v.feature = q.feature;
  v.flip = (q.q.flags & SPTR_SIGNED_FLIP_TRIANGLES) ? 1u : 0u;
  v.geom_first = static_cast<const uint32_t*>(x->geom_first.p);
  v.cpos = static_cast<const float*>(g.cpos.p);
  v.nv = static_cast<const float*>(g.nv.p);
  v.ne = static_cast<const float*>(g.ne.p);
  v.sph = static_cast<const float4*>(g.sph.p);
  v.num_tris = g.num_tris;
  v.num_sph = g.num_sph;
  v.num_tri_geoms = g.num_tri_geoms;
  API_HIP(hipEventRecord(sq.run.ev[0], s));
  launch_point_sign(v, s);
  return query_end(x, sq.run, false, s);
}

int sptr_query_signed_distance(sptr_ctx* x, const sptr_signed_query* sq_in, void* stream) {
  if (!x || !sq_in) return SPTR_ERR_INVALID;
  Context& c = x->c;
  const sptr_point_query* q = &sq_in->q;
  const char* who = "query_signed_distance";
  const bool dev = (q->flags & SPTR_QUERY_DEVICE_PTRS) != 0u;
  int rc = check_query_flags(x, who, q->flags, kPointFlags | (uint32_t)SPTR_SIGNED_FLIP_TRIANGLES,
                             "SPTR_QUERY_ANY_HIT or unknown flags");
  if (rc == SPTR_OK) rc = check_query_batch(x, who, "points", q->n, q->points);
  if (rc != SPTR_OK) return rc;
  if (q->reserved[0] || q->reserved[1] || q->reserved[2] || q->reserved[3] || sq_in->reserved[0] || sq_in->reserved[1] ||
      sq_in->reserved[2] || sq_in->reserved[3])
    return fail(c, SPTR_ERR_INVALID, "query_signed_distance: reserved must be 0");
  const uintptr_t outs = reinterpret_cast<uintptr_t>(sq_in->signed_dist) | reinterpret_cast<uintptr_t>(sq_in->normal) |
                         reinterpret_cast<uintptr_t>(sq_in->feature);
  rc = check_query_placement(x, who, dev, stream, point_query_misaligned(*q) || (outs & 3u) != 0u, kPointAlignment);
  if (rc != SPTR_OK) return rc;
  if (!c.sg.valid)
    return fail(c, SPTR_ERR_INVALID, "query_signed_distance: the scene was not uploaded with sptr_set_signed_distance(1)");
  if (q->n == 0u) return SPTR_OK;
  API_HIP(hipSetDevice(c.device));
  if (stream) return enqueue_signed(x, *sq_in, static_cast<hipStream_t>(stream));  // only enqueues
  sptr_signed_query d = *sq_in;
  const size_t n = q->n;
  StageField out[10];
  point_stage_fields(*q, d.q, true, out);  // (the sign pass reads the ids whether or not the caller takes them)
  out[7] = {sq_in->signed_dist, &d.signed_dist, n * 4};
  out[8] = {sq_in->normal, &d.normal, n * 12};
  out[9] = {sq_in->feature, &d.feature, n * 4};
  return query_sync(x, dev, q->points, &d.q.points, n * 16, out, 10, [&] { return enqueue_signed(x, d, c.stream); });
}

int sptr_signed_info(sptr_ctx* x, sptr_signed_info_t* out) {
  if (!x) return SPTR_ERR_INVALID;
  const SignedState& g = x->c.sg;
  double ms_sign = 0.0;
  const int ri = query_run_info(x, x->sq.run, nullptr, &ms_sign, nullptr, nullptr);
  if (ri != SPTR_OK) return ri;
  if (out) {
    out->welded_vertices = g.valid ? g.counts_h[0] : 0u;
    out->edges = g.valid ? g.counts_h[1] : 0u;
    out->open_edges = g.valid ? g.counts_h[2] : 0u;
    out->irregular_edges = g.valid ? g.counts_h[3] : 0u;
    out->table_bytes = g.valid ? (uint64_t)g.num_tris * (72u + 36u) : 0u;
    out->builds = g.builds;
    out->valid = g.valid ? 1u : 0u;
    out->num_tris = g.valid ? g.num_tris : 0u;
    out->pad = 0u;
    out->ms_build = g.ms_build;
    out->ms_sign = ms_sign;
  }
  return SPTR_OK;
}

int sptr_read_pseudonormals(sptr_ctx* x, float* nv, float* ne) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (!c.have_scene) return fail(c, SPTR_ERR_NO_SCENE, "read_pseudonormals: no scene");
  if (!c.sg.valid)
    return fail(c, SPTR_ERR_INVALID, "read_pseudonormals: the scene was not uploaded with sptr_set_signed_distance(1)");
  API_HIP(hipSetDevice(c.device));
  const size_t nb = (size_t)c.sg.num_tris * 36;
  if (nb == 0) return SPTR_OK;
  if (nv) API_HIP(hipMemcpy(nv, c.sg.nv.p, nb, hipMemcpyDeviceToHost));
  if (ne) API_HIP(hipMemcpy(ne, c.sg.ne.p, nb, hipMemcpyDeviceToHost));
  return SPTR_OK;
}

// ---- path-traced radiance for caller-supplied rays ---------------------------------------------------
constexpr uint32_t kRaysMaxRays = 1u << 28;
constexpr uint64_t kRaysMaxPaths = 1ull << 29;
constexpr uint32_t kRaysFlags = SPTR_RAYS_DEVICE_PTRS | SPTR_RAYS_ACCUMULATE | SPTR_RAYS_NORMALIZE;
// wave capacity the ray path allocates when the context has none yet (about 0.8 GB with one light; a context
// that has rendered has its own, and the ray path takes that)
constexpr uint64_t kRaysOwnPaths = 1ull << 22;

// Paths per chunk that the wave buffers the context already has can hold on the current scene and lights,
// 0 if they cannot serve the ray path as they are.  A chunk of np paths needs np records in every stream, the
// segment slack ensure_wave adds, and hit records for the trace's segments (twice the static shares where the
// trace takes its rays from the per-XCD queues).
static uint64_t rays_wave_capacity(Context& c) {
  const WaveBufs& b = c.wb;
  const uint32_t L = std::max<uint32_t>(1u, (uint32_t)shading(c).lights_host.size()), ts = task_stride(c);
  if (!b.seg.p || !b.rad.p || b.cap == 0 || (uint64_t)b.L * b.ts < (uint64_t)L * ts) return 0;
  const uint64_t slack = (uint64_t)kMaxSegs * kBlock;
  const uint64_t hrecs = b.hrec.bytes / (kHitBytes * hrec_mult(scene_view(c)));
  if (hrecs <= slack) return 0;
  return std::min<uint64_t>(b.cap, hrecs - slack);
}

// after the last call completed: the flags its launches may have set in the call's totals block
static int ray_render_check(sptr_ctx* x, unsigned long long* tot_out) {
  Context& c = x->c;
  unsigned long long tot[kTotWords];
  API_HIP(hipMemcpy(tot, x->rr.tot.p, sizeof(tot), hipMemcpyDeviceToHost));
  if (tot_out) std::memcpy(tot_out, tot, sizeof(tot));
  if (tot[kTotOverflow]) return fail(c, SPTR_ERR_HIP, "render_rays: segmented stream overflow (internal error)");
  if (tot[kTotStackOverflow]) return fail(c, SPTR_ERR_HIP, "render_rays: BVH traversal stack overflow (internal error)");
  return SPTR_OK;
}

// One validated batch with device pointers, enqueued on the context's stream in chunks of at most cap paths.
// Per chunk: k_rays_inject, then the serial separate-stage chain from depth 0 — trace(d), shade(d) with its
// shadow ray in place where shade_fuses_shadows says so, else shadow(d) — with k_tail from the tail depth the
// batch-size rule gives a batch of the chunk's paths, then k_rays_gather.  No cull, no k_sky, no side streams,
// no captured graph, no straggler hand-off, no fused bounce launches, no deferred misses, no shadow carry.
static int enqueue_ray_render(sptr_ctx* x, const sptr_ray_render& q, uint64_t cap) {
  Context& c = x->c;
  auto& rr = x->rr;
  const hipStream_t s = c.stream;
  const SceneView sv = scene_view(c);
  const ShadeView sh = shade_view(c);
  WaveView w = wave_view(c);
  w.tot = static_cast<unsigned long long*>(rr.tot.p);
  sptr_frame f{};
  f.width = f.height = 1;
  f.frame_begin = q.frame_index;
  f.spp = 1;
  f.max_depth = q.max_depth;
  const FrameView fv = frame_view(c, f);  // (dyn null: absolute values; the stages of bounces >= 1 read max_depth only)
  const bool fuse = shade_fuses_shadows(sv, sh, false);
  RayBatchView b{};
  b.rays = reinterpret_cast<const float4*>(q.rays);
  b.seeds = q.seeds;
  b.samples = q.samples;
  b.frame_index = q.frame_index;
  b.normalize = (q.flags & SPTR_RAYS_NORMALIZE) ? 1u : 0u;
  b.accumulate = (q.flags & SPTR_RAYS_ACCUMULATE) ? 1u : 0u;
  b.radiance = q.radiance;
  b.carry = static_cast<float4*>(rr.carry.p);
  const int D = (int)q.max_depth;
  const uint64_t chunks = ray_chunk_count(q.n, q.samples, cap);
  for (uint64_t ci = 0; ci < chunks; ++ci) {
    const RayChunk ck = ray_chunk_at(q.n, q.samples, cap, ci);
    const uint64_t np = (uint64_t)ck.nrays * ck.ns;
    const int T = std::max(1, (int)(c.tail_depth ? c.tail_depth : auto_tail_depth(np, sv)));
    uint32_t g_shade = launch_rays_inject(b, ck, w, s);
    for (int d = 0; d < D; ++d) {
      if (d >= T) {
        launch_tail(sv, sh, fv, w, d, g_shade, s);
        break;
      }
      const uint32_t g_trace = launch_trace(sv, sh, fv, w, d, false, g_shade, s, true);
      g_shade = launch_shade(sv, sh, fv, w, d, g_trace, fuse, s, true);
      if (!fuse) launch_shadow(sv, sh, w, d, false, g_shade, s);
    }
    launch_rays_gather(b, ck, w, s);
    API_HIP(hipGetLastError());
  }
  rr.chunks = (uint32_t)chunks;
  return SPTR_OK;
}

int sptr_render_rays(sptr_ctx* x, const sptr_ray_render* q, void* stream) {
  if (!x || !q) return SPTR_ERR_INVALID;
  Context& c = x->c;
  auto& rr = x->rr;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "render_rays: not on a lane context");
  const bool dev = (q->flags & SPTR_RAYS_DEVICE_PTRS) != 0u;
  if (q->flags & ~kRaysFlags) return fail(c, SPTR_ERR_INVALID, "render_rays: unknown flags");
  for (uint32_t r : q->reserved)
    if (r) return fail(c, SPTR_ERR_INVALID, "render_rays: reserved words must be 0");
  if (q->n > kRaysMaxRays) return fail(c, SPTR_ERR_INVALID, "render_rays: more than 2^28 rays");
  if (q->samples == 0u || q->max_depth == 0u || q->max_depth > (uint32_t)kMaxDepth || q->frame_index == 0u)
    return fail(c, SPTR_ERR_INVALID, "render_rays: bad batch parameters");
  if ((uint64_t)q->frame_index + q->samples - 1u > 0xFFFFFFFFull)
    return fail(c, SPTR_ERR_INVALID, "render_rays: frame_index + samples - 1 overflows 32 bits");
  if ((uint64_t)q->n * q->samples > kRaysMaxPaths) return fail(c, SPTR_ERR_INVALID, "render_rays: more than 2^29 paths");
  if (q->n && (!q->rays || !q->radiance)) return fail(c, SPTR_ERR_INVALID, "render_rays: no rays or no radiance buffer");
  if (!dev && stream) return fail(c, SPTR_ERR_INVALID, "render_rays: host pointers cannot be enqueued on a stream");
  if (dev && (reinterpret_cast<uintptr_t>(q->rays) & 15u))
    return fail(c, SPTR_ERR_INVALID, "render_rays: the device ray buffer must be 16-byte aligned");
  if (!c.have_scene) return fail(c, SPTR_ERR_NO_SCENE, "render_rays: no scene");
  if (shading(c).mats_host.empty()) return fail(c, SPTR_ERR_NO_SCENE, "render_rays: no materials set");
  if (q->n == 0u) return SPTR_OK;
  API_HIP(hipSetDevice(c.device));
  const hipStream_t cs = stream ? static_cast<hipStream_t>(stream) : nullptr;
  for (DevEvent& e : rr.ev)
    if (!e) API_HIP(hipEventCreate(e.put()));
  // pending renders on another stream than the context's: waited for on the host (stream == NULL), or followed
  // through an event (a caller's stream; renders pending on that stream itself are followed through its fork)
  if (c.pending && c.pending_stream != c.stream && c.pending_stream != cs) {
    if (!cs) {
      if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
    } else {
      API_HIP(hipEventRecord(rr.ev[2], c.pending_stream));
      API_HIP(hipStreamWaitEvent(c.stream, rr.ev[2], 0));
    }
  }
  // The wave buffers the context has are taken as they are: the ray path never grows or reallocates them while
  // they can serve it.  A context without any (or whose buffers do not fit the current lights or scene) gets a
  // capacity through ensure_wave, which waits for pending renders and bumps the state epoch, as any growth does.
  uint64_t cap = rays_wave_capacity(c);
  if (cap == 0) {
    const uint64_t want = c.wb.cap ? c.wb.cap : std::min<uint64_t>(kRaysOwnPaths, (uint64_t)q->n * q->samples);
    const int rc = ensure_wave(c, want, (uint32_t)shading(c).lights_host.size(), task_stride(c), 1u, hrec_mult(scene_view(c)));
    if (rc != SPTR_OK) return rc;
    cap = rays_wave_capacity(c);
    if (cap == 0) return fail(c, SPTR_ERR_HIP, "render_rays: no wave capacity (internal error)");
  }
  if (c.wave_paths) cap = std::min<uint64_t>(cap, c.wave_paths);
  if (!rr.tot.p) API_HIP(rr.tot.ensure(kTotWords * 8));
  if (!rr.carry.p) API_HIP(rr.carry.ensure(256));
  sptr_ray_render d = *q;
  const size_t n = q->n;
  if (!dev) {  // host pointers: rays, seeds and (to accumulate) the radiance in, the radiance out
    API_HIP(rr.stage_rays.ensure(n * 32));
    API_HIP(rr.stage_out.ensure(n * 12));
    API_HIP(hipMemcpyAsync(rr.stage_rays.p, q->rays, n * 32, hipMemcpyHostToDevice, c.stream));
    if (q->seeds) {
      API_HIP(rr.stage_seeds.ensure(n * 4));
      API_HIP(hipMemcpyAsync(rr.stage_seeds.p, q->seeds, n * 4, hipMemcpyHostToDevice, c.stream));
      d.seeds = static_cast<const uint32_t*>(rr.stage_seeds.p);
    }
    if (q->flags & SPTR_RAYS_ACCUMULATE)
      API_HIP(hipMemcpyAsync(rr.stage_out.p, q->radiance, n * 12, hipMemcpyHostToDevice, c.stream));
    d.rays = static_cast<const float*>(rr.stage_rays.p);
    d.radiance = static_cast<float*>(rr.stage_out.p);
  }
  if (cs) {  // the rays' producer on the caller's stream
    API_HIP(hipEventRecord(rr.ev[2], cs));
    API_HIP(hipStreamWaitEvent(c.stream, rr.ev[2], 0));
  }
  API_HIP(hipMemsetAsync(rr.tot.p, 0, kTotWords * 8, c.stream));
  API_HIP(hipEventRecord(rr.ev[0], c.stream));
  const int rc = enqueue_ray_render(x, d, cap);
  // (the end event also after a failed launch: what was enqueued may still run)
  const hipError_t ee = hipEventRecord(rr.ev[1], c.stream);
  rr.issued = ee == hipSuccess;
  if (rc != SPTR_OK) return rc;
  API_HIP(ee);
  if (cs) {
    API_HIP(hipStreamWaitEvent(cs, rr.ev[1], 0));
    return SPTR_OK;
  }
  API_HIP(hipStreamSynchronize(c.stream));
  const int rf = ray_render_check(x, nullptr);
  if (rf != SPTR_OK) return rf;
  if (!dev) API_HIP(hipMemcpy(q->radiance, d.radiance, n * 12, hipMemcpyDeviceToHost));
  return SPTR_OK;
}

int sptr_ray_render_info(sptr_ctx* x, double* ms, uint64_t* closest, uint64_t* shadow, uint32_t* chunks) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  auto& rr = x->rr;
  double ms_v = 0.0;
  unsigned long long tot[kTotWords] = {};
  int rc = SPTR_OK;
  if (rr.issued) {
    API_HIP(hipSetDevice(c.device));
    API_HIP(hipEventSynchronize(rr.ev[1]));
    float t = 0.0f;
    API_HIP(hipEventElapsedTime(&t, rr.ev[0], rr.ev[1]));
    ms_v = t;
    rc = ray_render_check(x, tot);
  }
  if (ms) *ms = ms_v;
  if (closest) *closest = tot[kTotClosest];
  if (shadow) *shadow = tot[kTotShadow];
  if (chunks) *chunks = rr.issued ? rr.chunks : 0u;
  return rc;
}

// ---- adaptive sampling ------------------------------------------------------------------
// Context::last_samples after an adaptive call: no frame_begin continues it (frame_begin + 0 == 0 is rejected)
constexpr uint32_t kAdaptiveMark = 0xFFFFFFFFu;
constexpr uint32_t kAdaptiveMaxSamples = 65536u;

// the state block for P local pixels: guard | E | guard | n | guard | list | guard | block words | result
static int ensure_adaptive(sptr_ctx* x, uint32_t P) {
  Context& c = x->c;
  auto& ad = x->ad;
  if (ad.state.p && ad.P == P) return SPTR_OK;
  const size_t g = kAdaptiveGuardWords;
  size_t off[4], w = 0;
  off[0] = w, w += g;
  const size_t wE = w;
  w += (size_t)P * 4;
  off[1] = w, w += g;
  const size_t wn = w;
  w += P;
  off[2] = w, w += g;
  const size_t wl = w;
  w += P;
  off[3] = w, w += g;
  const size_t wb = w;
  w += (size_t)kMaxSegs * kAdaptiveStatWords;
  const size_t wr = w;
  w += kAdaptiveResWords;
  ad.valid = false;
  API_HIP(ad.state.ensure(w * 4));
  uint32_t* base = static_cast<uint32_t*>(ad.state.p);
  API_HIP(hipMemset(base, 0, w * 4));
  const std::vector<uint32_t> guard(g, kAdaptiveGuardValue);
  for (int k = 0; k < 4; ++k) {
    API_HIP(hipMemcpy(base + off[k], guard.data(), g * 4, hipMemcpyHostToDevice));
    ad.bufs.guard_off[k] = (uint32_t)off[k];
  }
  ad.bufs.base = base;
  ad.bufs.E = reinterpret_cast<float4*>(base + wE);  // (16-byte aligned: the guard run is 64 B)
  ad.bufs.n = base + wn;
  ad.bufs.list = base + wl;
  ad.bufs.bstat = base + wb;
  ad.bufs.result = base + wr;
  ad.P = P;
  return SPTR_OK;
}

// One group of a pass: the first `count` list entries take `take` samples each, in chunks of at most cap paths.
// Per chunk: k_adapt_inject, the chain of enqueue_ray_render, k_adapt_gather.
static int enqueue_adaptive_group(sptr_ctx* x, const FrameView& fv, const FrameView& fchain, uint32_t count, uint32_t take,
                                  uint64_t cap, uint32_t& chunks_out) {
  Context& c = x->c;
  const hipStream_t s = c.stream;
  const SceneView sv = scene_view(c);
  const ShadeView sh = shade_view(c);
  WaveView w = wave_view(c);
  w.tot = static_cast<unsigned long long*>(x->ad.tot.p);
  const bool fuse = shade_fuses_shadows(sv, sh, false);
  const int D = (int)fv.max_depth;
  const uint64_t chunks = ray_chunk_count(count, take, cap);
  for (uint64_t ci = 0; ci < chunks; ++ci) {
    const RayChunk ck = ray_chunk_at(count, take, cap, ci);
    const uint64_t np = (uint64_t)ck.nrays * ck.ns;
    const int T = std::max(1, (int)(c.tail_depth ? c.tail_depth : auto_tail_depth(np, sv)));
    uint32_t g_shade = launch_adapt_inject(x->ad.bufs, ck, c.seed_offset, fv, w, s);
    for (int d = 0; d < D; ++d) {
      if (d >= T) {
        launch_tail(sv, sh, fchain, w, d, g_shade, s);
        break;
      }
      const uint32_t g_trace = launch_trace(sv, sh, fchain, w, d, false, g_shade, s, true);
      g_shade = launch_shade(sv, sh, fchain, w, d, g_trace, fuse, s, true);
      if (!fuse) launch_shadow(sv, sh, w, d, false, g_shade, s);
    }
    launch_adapt_gather(x->ad.bufs, ck, fv, w, s);
    API_HIP(hipGetLastError());
  }
  chunks_out += (uint32_t)chunks;
  return SPTR_OK;
}

int sptr_render_adaptive(sptr_ctx* x, const sptr_frame* f, const sptr_adaptive_params* p, sptr_adaptive_info* info) {
  if (!x || !f || !p) return SPTR_ERR_INVALID;
  Context& c = x->c;
  auto& ad = x->ad;
  if (info) std::memset(info, 0, sizeof(*info));
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "render_adaptive: not on a lane context");
  API_HIP(hipSetDevice(c.device));
  if (!c.have_scene) return fail(c, SPTR_ERR_NO_SCENE, "render_adaptive: no scene uploaded");
  if (shading(c).mats_host.empty()) return fail(c, SPTR_ERR_NO_SCENE, "render_adaptive: no materials set");
  if (x->dn.p.iterations != 0u) return fail(c, SPTR_ERR_INVALID, "render_adaptive: the denoiser is on (sptr_set_denoise)");
  if (p->flags & ~(uint32_t)SPTR_ADAPTIVE_CONTINUE) return fail(c, SPTR_ERR_INVALID, "render_adaptive: unknown flags");
  for (uint32_t r : p->reserved)
    if (r) return fail(c, SPTR_ERR_INVALID, "render_adaptive: reserved words must be 0");
  if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold) || p->min_samples < 2u || p->max_samples < p->min_samples ||
      p->max_samples > kAdaptiveMaxSamples || p->step < 1u)
    return fail(c, SPTR_ERR_INVALID, "render_adaptive: parameters out of bounds");
  if (f->width <= 0 || f->height <= 0 || f->max_depth == 0 || f->max_depth > (uint32_t)kMaxDepth || f->frame_begin != 1u)
    return fail(c, SPTR_ERR_INVALID, "render_adaptive: bad frame parameters (frame_begin must be 1)");
  if (f->integrator != SPTR_INTEGRATOR_WAVEFRONT)
    return fail(c, SPTR_ERR_INVALID, "render_adaptive: SPTR_INTEGRATOR_WAVEFRONT only");
  if (f->flags & ~(uint32_t)SPTR_FRAME_NO_RESOLVE)
    return fail(c, SPTR_ERR_INVALID, "render_adaptive: the only frame flag accepted is SPTR_FRAME_NO_RESOLVE");
  const int G = f->shard_count > 0 ? f->shard_count : 1, R = f->shard_count > 0 ? f->shard_rank : 0;
  if (R < 0 || R >= G) return fail(c, SPTR_ERR_INVALID, "render_adaptive: shard_rank out of range");
  const int ntiles = ((f->width + kTile - 1) / kTile) * ((f->height + kTile - 1) / kTile);
  if (R >= ntiles) return fail(c, SPTR_ERR_INVALID, "render_adaptive: more shards than tiles");
  if ((uint64_t)f->width * f->height > (1ull << 28)) return fail(c, SPTR_ERR_INVALID, "render_adaptive: image too large");
  if ((uint64_t)c.seed_offset + p->max_samples > 0xFFFFFFFFull)
    return fail(c, SPTR_ERR_INVALID, "render_adaptive: seed offset + max_samples overflows 32 bits");
  const bool cont = (p->flags & SPTR_ADAPTIVE_CONTINUE) != 0u;
  if (cont) {
    const bool same = ad.valid && !x->split && c.last_samples == kAdaptiveMark && ad.W == f->width && ad.H == f->height &&
                      ad.G == G && ad.R == R && c.W == f->width && c.H == f->height && c.G == G && c.R == R &&
                      ad.max_depth == f->max_depth && ad.epoch == c.epoch && std::memcmp(&ad.cam, &f->camera, sizeof(sptr_camera)) == 0;
    if (!same)
      return fail(c, SPTR_ERR_INVALID, "render_adaptive: SPTR_ADAPTIVE_CONTINUE needs the last adaptive call's size, camera, depth, shard and state");
  }
  // synchronous: everything pending on the context ends first
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  if (x->split) {  // leaving a two-lane accumulation, as a one-lane render call does
    if (sync_pending(x->lane->c) != SPTR_OK) return SPTR_ERR_HIP;
    x->split = false;
    c.W = 0;
  }
  const hipStream_t s = c.stream;
  bool resized = false;
  int rc = ensure_pixels(c, f->width, f->height, G, R, s, resized);
  if (rc != SPTR_OK) return rc;
  // wave capacity as sptr_render_rays takes it: the buffers the context has, or a capacity of the ray path's own
  uint64_t cap = rays_wave_capacity(c);
  if (cap == 0) {
    const uint64_t want = c.wb.cap ? c.wb.cap : std::min<uint64_t>(kRaysOwnPaths, (uint64_t)c.P * p->min_samples);
    rc = ensure_wave(c, want, (uint32_t)shading(c).lights_host.size(), task_stride(c), 1u, hrec_mult(scene_view(c)));
    if (rc != SPTR_OK) return rc;
    cap = rays_wave_capacity(c);
    if (cap == 0) return fail(c, SPTR_ERR_HIP, "render_adaptive: no wave capacity (internal error)");
  }
  if (c.wave_paths) cap = std::min<uint64_t>(cap, c.wave_paths);
  if (cont && ad.epoch != c.epoch) return fail(c, SPTR_ERR_INVALID, "render_adaptive: the state changed since the last adaptive call");
  rc = ensure_adaptive(x, c.P);
  if (rc != SPTR_OK) return rc;
  if (!ad.tot.p) API_HIP(ad.tot.ensure(kTotWords * 8));
  for (DevEvent& e : ad.ev)
    if (!e) API_HIP(hipEventCreate(e.put()));
  ad.valid = false;
  c.last_samples = kAdaptiveMark;
  x->dn.ran = false;
  x->dn.last_cam = f->camera;
  x->dn.last_W = f->width;
  x->dn.last_H = f->height;

  const FrameView fv = frame_view(c, *f);
  sptr_frame fc{};  // the chain's frame, as enqueue_ray_render builds it (its stages read max_depth only)
  fc.width = fc.height = 1;
  fc.frame_begin = 1;
  fc.spp = 1;
  fc.max_depth = f->max_depth;
  const FrameView fchain = frame_view(c, fc);
  const AdaptiveRule rule{p->threshold, p->min_samples, p->max_samples, p->step};

  API_HIP(hipMemsetAsync(ad.tot.p, 0, kTotWords * 8, s));
  API_HIP(hipEventRecord(ad.ev[0], s));
  if (!cont) {
    API_HIP(hipMemsetAsync(c.accum.p, 0, (size_t)c.P * 16, s));
    API_HIP(hipMemsetAsync(ad.bufs.E, 0, (size_t)c.P * 16, s));
    API_HIP(hipMemsetAsync(ad.bufs.n, 0, (size_t)c.P * 4, s));
  }
  sptr_adaptive_info out{};
  uint32_t res[kAdaptiveResWords] = {};
  auto select = [&](uint32_t key) -> int {
    launch_adapt_select(ad.bufs, rule, key, fv, s);
    API_HIP(hipGetLastError());
    API_HIP(hipStreamSynchronize(s));
    API_HIP(hipMemcpy(res, ad.bufs.result, sizeof(res), hipMemcpyDeviceToHost));
    if (res[kAdaptiveResGuardBad]) return fail(c, SPTR_ERR_HIP, "render_adaptive: a guard word of the state was overwritten (internal error)");
    return SPTR_OK;
  };
  // the key most pixels of the next pass will have: a new accumulation's first pass is all fresh pixels, and
  // after it every active pixel of a call that is no continuation holds the same n
  uint32_t guess = cont ? std::min<uint32_t>(p->step, p->max_samples) : kAdaptiveKeyFresh;
  uint32_t n_uniform = 0;  // (calls that are no continuation: the n of every active pixel)
  for (;;) {
    rc = select(guess);
    if (rc != SPTR_OK) return rc;
    if (res[kAdaptiveResActive] == 0u) break;
    uint32_t key = guess;
    if (res[kAdaptiveResKeyBelow] != 0xFFFFFFFFu || res[kAdaptiveResGroup] == 0u) {  // a smaller key comes first
      key = std::min(res[kAdaptiveResKeyBelow], res[kAdaptiveResKeyAbove]);
      const uint32_t active = res[kAdaptiveResActive];
      rc = select(key);
      if (rc != SPTR_OK) return rc;
      if (res[kAdaptiveResActive] != active || res[kAdaptiveResGroup] == 0u || res[kAdaptiveResKeyBelow] != 0xFFFFFFFFu)
        return fail(c, SPTR_ERR_HIP, "render_adaptive: selection not reproducible (internal error)");
    }
    ++out.passes;
    out.active_last = res[kAdaptiveResActive];
    if (out.passes == 1u) out.active_first = out.active_last;
    for (;;) {  // the pass's groups in ascending key
      const uint32_t count = res[kAdaptiveResGroup];
      const uint32_t take = key == kAdaptiveKeyFresh ? p->min_samples : key;
      rc = enqueue_adaptive_group(x, fv, fchain, count, take, cap, out.chunks);
      if (rc != SPTR_OK) return rc;
      out.samples += (uint64_t)count * take;
      const uint32_t next = res[kAdaptiveResKeyAbove];
      if (next == 0xFFFFFFFFu) break;
      key = next;
      rc = select(key);
      if (rc != SPTR_OK) return rc;
      if (res[kAdaptiveResGroup] == 0u) return fail(c, SPTR_ERR_HIP, "render_adaptive: empty group (internal error)");
    }
    n_uniform = n_uniform == 0u ? p->min_samples : n_uniform + std::min(p->step, p->max_samples - n_uniform);
    guess = cont ? std::min<uint32_t>(p->step, p->max_samples)
                 : std::max<uint32_t>(1u, std::min(p->step, p->max_samples - std::min(n_uniform, p->max_samples)));
  }
  out.min_count = res[kAdaptiveResMinN] == 0xFFFFFFFFu ? 0u : res[kAdaptiveResMinN];
  out.max_count = res[kAdaptiveResMaxN];
  if (!(f->flags & SPTR_FRAME_NO_RESOLVE)) {
    launch_adapt_resolve(ad.bufs, fv, static_cast<uint32_t*>(c.tiles.p), static_cast<uint8_t*>(c.image.p), s);
    API_HIP(hipGetLastError());
  }
  API_HIP(hipEventRecord(ad.ev[1], s));
  API_HIP(hipStreamSynchronize(s));
  unsigned long long tot[kTotWords];
  API_HIP(hipMemcpy(tot, ad.tot.p, sizeof(tot), hipMemcpyDeviceToHost));
  if (tot[kTotOverflow]) return fail(c, SPTR_ERR_HIP, "render_adaptive: segmented stream overflow (internal error)");
  if (tot[kTotStackOverflow]) return fail(c, SPTR_ERR_HIP, "render_adaptive: BVH traversal stack overflow (internal error)");
  float ms = 0.0f;
  API_HIP(hipEventElapsedTime(&ms, ad.ev[0], ad.ev[1]));
  out.ms = ms;
  out.rays_closest = tot[kTotClosest];
  out.rays_shadow = tot[kTotShadow];
  ad.valid = true;
  ad.cam = f->camera;
  ad.W = f->width;
  ad.H = f->height;
  ad.G = G;
  ad.R = R;
  ad.max_depth = f->max_depth;
  ad.epoch = c.epoch;
  if (info) *info = out;
  return SPTR_OK;
}

int sptr_read_sample_counts(sptr_ctx* x, uint32_t* counts) {
  if (!x || !counts) return SPTR_ERR_INVALID;
  Context& c = x->c;
  auto& ad = x->ad;
  if (!ad.valid || c.last_samples != kAdaptiveMark || ad.P != c.P)
    return fail(c, SPTR_ERR_INVALID, "read_sample_counts: the context holds no adaptive state");
  API_HIP(hipSetDevice(c.device));
  std::vector<uint32_t> n(c.P);
  API_HIP(hipMemcpy(n.data(), ad.bufs.n, (size_t)c.P * 4, hipMemcpyDeviceToHost));
  std::memset(counts, 0, (size_t)c.W * c.H * 4);
  for (uint32_t l = 0; l < c.P; ++l) {
    int px, py;
    if (host_local_pixel(c, l, px, py)) counts[(size_t)py * c.W + px] = n[l];
  }
  return SPTR_OK;
}

int sptr_primary_rays(sptr_ctx* x, const sptr_camera* cam, int32_t W, int32_t H, uint32_t acc, float* dirs,
                      uint32_t* rng) {
  if (!x || !cam || W <= 0 || H <= 0 || !dirs || !rng) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  API_HIP(hipSetDevice(c.device));
  sptr_frame f{};
  f.width = W;
  f.height = H;
  f.camera = *cam;
  f.frame_begin = acc;
  f.max_depth = 1;
  FrameView fv = frame_view(c, f);
  const size_t n = (size_t)W * H;
  API_HIP(c.qbuf.ensure(n * 16 + 64));
  float* d_dirs = static_cast<float*>(c.qbuf.p);
  uint32_t* d_rng = reinterpret_cast<uint32_t*>(static_cast<char*>(c.qbuf.p) + n * 12);
  launch_primary(fv, d_dirs, d_rng, c.stream);
  API_HIP(hipGetLastError());
  API_HIP(hipStreamSynchronize(c.stream));
  API_HIP(hipMemcpy(dirs, d_dirs, n * 12, hipMemcpyDeviceToHost));
  API_HIP(hipMemcpy(rng, d_rng, n * 4, hipMemcpyDeviceToHost));
  return SPTR_OK;
}

int sptr_sort_pairs_u64(sptr_ctx* x, const uint64_t* keys, const uint32_t* vals, uint32_t n, uint64_t* keys_out,
                        uint32_t* vals_out) {
  if (!x || (n && (!keys || !vals || !keys_out || !vals_out))) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  API_HIP(hipSetDevice(c.device));
  DevTemps d;
  uint64_t *ki = nullptr, *ko = nullptr;
  uint32_t *vi = nullptr, *vo = nullptr;
  char* tmp = nullptr;
  size_t tb = 0;
  API_HIP(radix_sort_pairs_u64(nullptr, tb, nullptr, nullptr, nullptr, nullptr, n, c.stream));
  API_HIP(d.alloc(&ki, n));
  API_HIP(d.alloc(&ko, n));
  API_HIP(d.alloc(&vi, n));
  API_HIP(d.alloc(&vo, n));
  API_HIP(d.alloc(&tmp, tb));
  if (n) {
    API_HIP(hipMemcpy(ki, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    API_HIP(hipMemcpy(vi, vals, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  API_HIP(radix_sort_pairs_u64(tmp, tb, ki, ko, vi, vo, n, c.stream));
  API_HIP(hipStreamSynchronize(c.stream));
  if (n) {
    API_HIP(hipMemcpy(keys_out, ko, (size_t)n * 8, hipMemcpyDeviceToHost));
    API_HIP(hipMemcpy(vals_out, vo, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  return SPTR_OK;
}

int sptr_eval_math(sptr_ctx* x, int fn, const float* in, uint32_t n, float* out) {
  if (!x || !out || (fn != SPTR_MATH_COSINE_SINCOS && fn != SPTR_MATH_GAMMA) || (fn == SPTR_MATH_GAMMA && n && !in))
    return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  API_HIP(hipSetDevice(c.device));
  const uint32_t m = fn == SPTR_MATH_COSINE_SINCOS ? (1u << 24) : n;
  const size_t out_n = fn == SPTR_MATH_COSINE_SINCOS ? 2u * (size_t)m : (size_t)m;
  DevTemps d;
  float *di = nullptr, *dout = nullptr;
  API_HIP(d.alloc(&di, fn == SPTR_MATH_GAMMA ? (size_t)n : 4));
  API_HIP(d.alloc(&dout, out_n));
  if (fn == SPTR_MATH_GAMMA && n) API_HIP(hipMemcpy(di, in, (size_t)n * 4, hipMemcpyHostToDevice));
  if (m) launch_eval_math(fn, di, m, dout, c.stream);
  API_HIP(hipGetLastError());
  API_HIP(hipStreamSynchronize(c.stream));
  if (out_n) API_HIP(hipMemcpy(out, dout, out_n * 4, hipMemcpyDeviceToHost));
  return SPTR_OK;
}

int sptr_scan_u32(sptr_ctx* x, const uint32_t* in, uint32_t n, uint32_t* out) {
  if (!x || (n && (!in || !out))) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  API_HIP(hipSetDevice(c.device));
  DevTemps d;
  uint32_t *di = nullptr, *dout = nullptr;
  char* tmp = nullptr;
  size_t tb = 0;
  API_HIP(scan_u32(nullptr, tb, nullptr, nullptr, n, c.stream));
  API_HIP(d.alloc(&di, n));
  API_HIP(d.alloc(&dout, n));
  API_HIP(d.alloc(&tmp, tb));
  if (n) API_HIP(hipMemcpy(di, in, (size_t)n * 4, hipMemcpyHostToDevice));
  API_HIP(scan_u32(tmp, tb, di, dout, n, c.stream));
  API_HIP(hipStreamSynchronize(c.stream));
  if (n) API_HIP(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
  return SPTR_OK;
}


// ---- pixel lanes -------------------------------------------------------------------------------
// A setter applied to the lane context too: its failure is reported through this context's error text.
static int lane_forward(sptr_ctx* x, int rc_lane) {
  if (!x || !x->lane || rc_lane == SPTR_OK) return SPTR_OK;
  return fail(x->c, rc_lane, std::string("pixel lane: ") + x->lane->c.err);
}

int sptr_upload_scene(sptr_ctx* x, const sptr_scene* s) {
  const int rc = upload_scene_one(x, s);
  if (rc != SPTR_OK) return rc;
  x->geom_first_valid = false;
  x->dn.snap_valid = false;  // (the snapshot's slots were the old scene's)
  if (x->split) x->c.W = 0;  // the pixel buffers describe the even lane: re-laid out for the next call
  x->split = false;
  x->lane_scene = false;
  // the lane gets a copy only of scenes staged into LDS (small by construction): the two chains of a
  // larger scene traversed from L2/HBM compete for the same memory latency (r05zs: C5 8.0 -> 7.6-7.7 ms,
  // but a second copy of a 10M-triangle scene), and C3's VALU-bound sky gains nothing (3.55-3.63 -> 3.65)
  if (x->lane && scene_view(x->c).lds_bytes != 0) {
    Context& cy = x->lane->c;
    // (a priority of its own puts the lane's stream on a hardware queue apart from the render stream's:
    // created at the default priority it shared that queue and the two chains ran one after the other,
    // r05zx, C2 3.24 ms; at the lowest priority, the side streams', 2.56-2.58; at the highest 2.67-2.69)
    if (!cy.stream && hipStreamCreateWithPriority(cy.stream.put(), hipStreamNonBlocking, x->c.prio_lo) != hipSuccess)
      return fail(x->c, SPTR_ERR_HIP, "pixel lane: stream creation failed");
    const int r1 = upload_scene_one(x->lane, s);
    if (r1 != SPTR_OK) return lane_forward(x, r1);
    x->lane_scene = true;
    const int r2 = build_prim_materials(cy);  // (its slots, this context's geom_mat)
    if (r2 != SPTR_OK) return lane_forward(x, r2);
  }
  return SPTR_OK;
}

// ---- dynamic scenes ----------------------------------------------------------------------------
int sptr_set_dynamic(sptr_ctx* x, uint32_t on) {
  if (!x) return SPTR_ERR_INVALID;
  x->c.dynamic = on != 0u;  // read by the next upload (build_lbvh)
  x->c.dynamic_xf = (on & SPTR_DYNAMIC_TRANSFORMS) != 0u;
  // (the lane's copy of the scene is refitted from this context's rest pose and matrices: it keeps neither)
  if (x->lane) x->lane->c.dynamic = x->c.dynamic;
  return SPTR_OK;
}

// c's scene refitted from device coordinates (either may be null); d_xf: refit_lbvh
static int refit_one(Context& c, const float* d_pos, const float* d_sph, const float* d_xf) {
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;  // a pending render may still read the old boxes
  const int rc = refit_lbvh(c, d_pos, reinterpret_cast<const float4*>(d_sph), d_xf);
  ++c.epoch;  // cull mask, AOV planes and captured graphs were computed for the old coordinates
  ++c.geom_rev;  // ... and the shadow entry table
  return rc;
}

// The body sptr_update_geometry and sptr_update_transforms share, after their arguments are checked and their
// host arrays staged on c.stream: the history's snapshot, the refit, the epoch, the pixel lane's copy.
static int refit_scene(sptr_ctx* x, const char* who, const float* d_pos, const float* d_sph, const float* d_xf,
                       std::chrono::steady_clock::time_point t0) {
  Context& c = x->c;
  // sptr_set_history_motion: the records the last history pass saw, kept before the refit overwrites them.
  // Only when that pass ran on this generation: after two refits between passes the snapshot still holds
  // the geometry of the pass a later call takes as its carry.
  auto& d = x->dn;
  if (d.motion_on && d.last.valid && d.last.gen == d.geom_gen) {
    const int rs = refit_snapshot(c);
    if (rs != SPTR_OK) return rs;
    d.snap_gen = d.geom_gen;
    d.snap_valid = true;
  }
  const uint64_t epoch_before = c.epoch;
  const int rc = refit_one(c, d_pos, d_sph, d_xf);  // (returns after c.stream drained: the staging is stable)
  ++d.geom_gen;
  if (rc != SPTR_OK) return rc;
  if (c.sg.valid) {  // sptr_set_signed_distance: the tables of the moved corners, welding included
    const int rs = signed_rebuild(c, d_pos, d_xf, reinterpret_cast<const float4*>(d_sph));
    if (rs != SPTR_OK) return rs;
  }
  if (d.motion_on)  // the history outlives the refit: its passes follow the epoch, and differ by generation
    for (sptr_ctx::Denoise::Pass* p : {&d.last, &d.carry})
      if (p->valid && p->epoch == epoch_before) p->epoch = c.epoch;
  if (x->lane && x->lane_scene) {  // the lane's copy of the scene, on the lane's stream
    Context& cy = x->lane->c;
    if (!cy.rf.valid) return fail(c, SPTR_ERR_INVALID, std::string(who) + ": the pixel lane's scene is not dynamic");
    const int r1 = refit_one(cy, d_pos, d_sph, d_xf);
    if (r1 != SPTR_OK) return lane_forward(x, r1);
  }
  c.rf.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SPTR_OK;
}

int sptr_update_geometry(sptr_ctx* x, const float* positions, uint32_t num_verts, const float* spheres,
                         uint32_t num_spheres, uint32_t flags) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "update_geometry: not on a lane context");
  if (!c.have_scene) return fail(c, SPTR_ERR_NO_SCENE, "update_geometry: no scene uploaded");
  if (c.rf.split)
    return fail(c, SPTR_ERR_INVALID, "update_geometry: the scene was built with split references (sptr_set_split_refs)");
  if (!c.rf.valid) return fail(c, SPTR_ERR_INVALID, "update_geometry: the scene was not uploaded with sptr_set_dynamic(1)");
  if (!positions && !spheres) return fail(c, SPTR_ERR_INVALID, "update_geometry: no coordinates given");
  if ((positions && num_verts != c.rf.num_verts) || (spheres && num_spheres != c.num_sph))
    return fail(c, SPTR_ERR_INVALID, "update_geometry: counts differ from the uploaded scene's");
  if (flags & ~(uint32_t)SPTR_UPDATE_DEVICE_PTRS) return fail(c, SPTR_ERR_INVALID, "update_geometry: unknown flags");
  const auto t0 = std::chrono::steady_clock::now();
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  const float *d_pos = positions, *d_sph = spheres;
  if (!(flags & SPTR_UPDATE_DEVICE_PTRS)) {
    if (positions) {
      API_HIP(c.rf.in_pos.ensure((size_t)num_verts * 12));
      API_HIP(hipMemcpyAsync(c.rf.in_pos.p, positions, (size_t)num_verts * 12, hipMemcpyHostToDevice, c.stream));
      d_pos = static_cast<const float*>(c.rf.in_pos.p);
    }
    if (spheres) {
      API_HIP(c.rf.in_sph.ensure((size_t)num_spheres * 16));
      API_HIP(hipMemcpyAsync(c.rf.in_sph.p, spheres, (size_t)num_spheres * 16, hipMemcpyHostToDevice, c.stream));
      d_sph = static_cast<const float*>(c.rf.in_sph.p);
    }
  }
  return refit_scene(x, "update_geometry", d_pos, d_sph, nullptr, t0);
}

// The checks sptr_set_rest_positions and sptr_update_transforms share.
static int transforms_ready(sptr_ctx* x, const char* who) {
  Context& c = x->c;
  const std::string w(who);
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, w + ": not on a lane context");
  if (!c.have_scene) return fail(c, SPTR_ERR_NO_SCENE, w + ": no scene uploaded");
  if (c.rf.split) return fail(c, SPTR_ERR_INVALID, w + ": the scene was built with split references (sptr_set_split_refs)");
  if (!c.rf.valid || !c.rf.xf_valid)
    return fail(c, SPTR_ERR_INVALID, w + ": the scene was not uploaded with sptr_set_dynamic(SPTR_DYNAMIC_TRANSFORMS)");
  return SPTR_OK;
}

int sptr_set_rest_positions(sptr_ctx* x, const float* positions, uint32_t num_verts, uint32_t flags) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  const int ready = transforms_ready(x, "set_rest_positions");
  if (ready != SPTR_OK) return ready;
  if (num_verts != c.rf.num_verts || (num_verts && !positions))
    return fail(c, SPTR_ERR_INVALID, "set_rest_positions: the vertex count differs from the uploaded scene's");
  if (flags & ~(uint32_t)SPTR_UPDATE_DEVICE_PTRS) return fail(c, SPTR_ERR_INVALID, "set_rest_positions: unknown flags");
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  if (num_verts) {
    API_HIP(hipMemcpyAsync(c.rf.rest.p, positions, (size_t)num_verts * 12,
                           (flags & SPTR_UPDATE_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream));
    API_HIP(hipStreamSynchronize(c.stream));
  }
  return SPTR_OK;
}

int sptr_update_transforms(sptr_ctx* x, const float* xforms, uint32_t num_tri_geoms, const float* spheres,
                           uint32_t num_spheres, uint32_t flags) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  const int ready = transforms_ready(x, "update_transforms");
  if (ready != SPTR_OK) return ready;
  if (!xforms && !spheres) return fail(c, SPTR_ERR_INVALID, "update_transforms: neither matrices nor spheres given");
  // (a scene whose triangles belong to no geometry has no matrix to take: num_tri_geoms 0 is refused with xforms)
  if ((xforms && (num_tri_geoms != c.num_tri_geoms || num_tri_geoms == 0u)) || (spheres && num_spheres != c.num_sph))
    return fail(c, SPTR_ERR_INVALID, "update_transforms: counts differ from the uploaded scene's");
  if (flags & ~(uint32_t)SPTR_UPDATE_DEVICE_PTRS) return fail(c, SPTR_ERR_INVALID, "update_transforms: unknown flags");
  const bool device = (flags & SPTR_UPDATE_DEVICE_PTRS) != 0u;
  if (xforms && !device)
    for (size_t i = 0; i < (size_t)num_tri_geoms * 16; ++i)
      if (!std::isfinite(xforms[i])) return fail(c, SPTR_ERR_INVALID, "update_transforms: a matrix entry is not finite");
  const auto t0 = std::chrono::steady_clock::now();
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  const float *d_xf = xforms, *d_sph = spheres;
  if (!device) {
    if (xforms) {
      API_HIP(c.rf.in_xf.ensure((size_t)num_tri_geoms * 64));
      API_HIP(hipMemcpyAsync(c.rf.in_xf.p, xforms, (size_t)num_tri_geoms * 64, hipMemcpyHostToDevice, c.stream));
      d_xf = static_cast<const float*>(c.rf.in_xf.p);
    }
    if (spheres) {
      API_HIP(c.rf.in_sph.ensure((size_t)num_spheres * 16));
      API_HIP(hipMemcpyAsync(c.rf.in_sph.p, spheres, (size_t)num_spheres * 16, hipMemcpyHostToDevice, c.stream));
      d_sph = static_cast<const float*>(c.rf.in_sph.p);
    }
  }
  return refit_scene(x, "update_transforms", d_xf ? static_cast<const float*>(c.rf.rest.p) : nullptr, d_sph, d_xf, t0);
}

int sptr_tree_cost(sptr_ctx* x, double* cost, double* root_area, double* cost_at_upload, double* root_area_at_upload) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (!c.have_scene) return fail(c, SPTR_ERR_NO_SCENE, "tree_cost: no scene uploaded");
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  double cur = 0.0, area = 0.0;
  if (cost || root_area) {
    const int rc = refit_tree_cost(c, &cur, &area);
    if (rc != SPTR_OK) return rc;
  }
  if (cost) *cost = cur;
  if (root_area) *root_area = area;
  if (cost_at_upload) *cost_at_upload = c.rf.cost_upload;
  if (root_area_at_upload) *root_area_at_upload = c.rf.area_upload;
  return SPTR_OK;
}

int sptr_refit_info(const sptr_ctx* x, uint32_t* refits, double* ms_wall, double* ms_device, uint32_t* excluded_prims) {
  if (!x) return SPTR_ERR_INVALID;
  const Context& c = x->c;
  if (refits) *refits = c.rf.refits;
  if (ms_wall) *ms_wall = c.rf.ms_wall;
  if (ms_device) *ms_device = c.rf.ms_device;
  if (excluded_prims) *excluded_prims = c.excluded_prims;
  return SPTR_OK;
}

int sptr_set_pixel_lanes(sptr_ctx* x, uint32_t lanes) {
  if (!x) return SPTR_ERR_INVALID;
  if (lanes > 2u) return fail(x->c, SPTR_ERR_INVALID, "pixel lanes: 0 (automatic), 1 or 2");
  if (x->is_lane) return fail(x->c, SPTR_ERR_INVALID, "pixel lanes: not on a lane context");
  if (lanes == 2u && !x->lane) return fail(x->c, SPTR_ERR_INVALID, "pixel lanes: no lane context");
  if (sync_pending(x->c) != SPTR_OK) return SPTR_ERR_HIP;
  if (x->lane && sync_pending(x->lane->c) != SPTR_OK) return SPTR_ERR_HIP;
  x->lanes_req = lanes;
  if (x->split) x->c.W = 0;  // (as in sptr_upload_scene)
  x->split = false;  // the next call starts an accumulation of its own (frame_begin 1)
  x->c.last_samples = 0;
  return SPTR_OK;
}

int sptr_pixel_lanes_info(const sptr_ctx* x, uint32_t* requested, uint32_t* active) {
  if (!x) return SPTR_ERR_INVALID;
  if (requested) *requested = x->lanes_req;
  if (active) *active = x->split ? 1u : 0u;
  return SPTR_OK;
}

// Two lanes for this call: an accumulation continues in the mode it started in; a new one (frame_begin 1)
// runs in two lanes when the scene is staged into LDS, the integrator is the wavefront one and the call
// is large (>= 2^24 samples: r05zs, two contexts on one GPU, C2 3.0 -> 2.47 ms, C4 158.5 -> 137.5 ms, the
// 8-way C2 shard 0.49-0.51 -> 0.46 ms; 1-spp frames keep one chain), or when asked for (lanes_req 2).
static bool lanes_for(const sptr_ctx* x, const sptr_frame* f) {
  if (!x->lane || !x->lane_scene || x->lanes_req == 1u || f->integrator != SPTR_INTEGRATOR_WAVEFRONT) return false;
  const int G = f->shard_count > 0 ? f->shard_count : 1, R = f->shard_count > 0 ? f->shard_rank : 0;
  const int ntiles = ((f->width + kTile - 1) / kTile) * ((f->height + kTile - 1) / kTile);
  if (R < 0 || R >= G || R + G >= ntiles) return false;  // the second lane would hold no tile
  if (f->frame_begin != 1) return x->split;
  if (x->lanes_req == 2u) return true;
  const uint64_t px = (uint64_t)shard_tiles(f->width, f->height, G, R) * kTilePixels;
  return px * f->spp >= (1ull << 24);
}

static void add_stats(sptr_stats& a, const sptr_stats& b) {
  // the counters add, and so do the stage times (sums of launch durations); the call spans overlap
  const double total = std::max(a.ms_total, b.ms_total);
  a.rays_closest += b.rays_closest;
  a.rays_shadow += b.rays_shadow;
  a.samples += b.samples;
  a.waves += b.waves;
  a.ms_raygen += b.ms_raygen;
  a.ms_trace += b.ms_trace;
  a.ms_shade += b.ms_shade;
  a.ms_shadow += b.ms_shadow;
  a.ms_accum += b.ms_accum;
  a.trace_launches += b.trace_launches;
  a.node_visits += b.node_visits;
  a.tri_tests += b.tri_tests;
  a.sphere_tests += b.sphere_tests;
  a.shadow_node_visits += b.shadow_node_visits;
  a.shadow_prim_tests += b.shadow_prim_tests;
  a.ms_trace0 += b.ms_trace0;
  a.ms_shade0 += b.ms_shade0;
  a.rays_tail += b.rays_tail;
  a.ms_tail += b.ms_tail;
  a.traced_primary += b.traced_primary;
  a.traced_bounce += b.traced_bounce;
  a.node_visits_primary += b.node_visits_primary;
  a.tri_tests_primary += b.tri_tests_primary;
  a.sphere_tests_primary += b.sphere_tests_primary;
  a.ms_cull += b.ms_cull;
  a.cull_launches += b.cull_launches;
  a.shadow_launches += b.shadow_launches;
  for (int i = 0; i < 8; ++i) {
    a.traced_by_depth[i] += b.traced_by_depth[i];
    a.nodes_by_depth[i] += b.nodes_by_depth[i];
  }
  for (int i = 0; i < 16; ++i) {
    a.trace_visit_hist[i] += b.trace_visit_hist[i];
    a.shadow_visit_hist[i] += b.shadow_visit_hist[i];
  }
  a.hits_primary += b.hits_primary;
  a.hits_bounce += b.hits_bounce;
  a.paths_handed_off += b.paths_handed_off;
  for (int i = 0; i < 3; ++i) a.strag_visits[i] += b.strag_visits[i];
  a.traced_fused += b.traced_fused;
  a.ms_total = total;
  a.ms_trace_busy = std::max(a.ms_trace_busy, b.ms_trace_busy);  // (the callers set the union)
}

// One render call without the denoise pass (sptr_render, below, appends it).
static int render_call(sptr_ctx* x, const sptr_frame* f, void* stream, sptr_stats* stats) {
  Context& c = x->c;
  if (!lanes_for(x, f)) {
    if (x->split) {  // leaving a two-lane accumulation: this call must start a new one
      if (f->frame_begin != 1) return fail(c, SPTR_ERR_INVALID, "render: frame_begin must be 1 after a two-lane accumulation");
      if (sync_pending(x->lane->c) != SPTR_OK) return SPTR_ERR_HIP;
      x->split = false;
      c.W = 0;  // the pixel buffers describe the even lane: re-laid out for the whole shard
    }
    c.time_by_events = false;
    return render_one(x, f, stream, stats);
  }
  // two lanes: this context renders shard (R, 2G) — the even half of shard (R, G)'s tiles — and the
  // lane shard (R + G, 2G), the odd half, on its own stream, forked after everything enqueued on s so far
  // and joined back into s
  API_HIP(hipSetDevice(c.device));
  sptr_ctx* y = x->lane;
  Context& cy = y->c;
  const int G = f->shard_count > 0 ? f->shard_count : 1, R = f->shard_count > 0 ? f->shard_rank : 0;
  sptr_frame f0 = *f, f1 = *f;
  f0.shard_count = f1.shard_count = 2 * G;
  f0.shard_rank = R;
  f1.shard_rank = R + G;
  f0.flags |= SPTR_FRAME_ASYNC;
  f1.flags |= SPTR_FRAME_ASYNC;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c.stream;
  const bool serial = c.launch_mode == 2u;  // one stream: the lanes one after the other
  hipStream_t sy = serial ? s : cy.stream;
  // both halves checked before either is enqueued (a change into or out of launch mode 2 between two
  // asynchronous calls moves the lane's half between its own stream and s: ADVICE r05)
  if ((c.pending && s != c.pending_stream) || (cy.pending && sy != cy.pending_stream))
    return fail(c, SPTR_ERR_INVALID, "render: asynchronous renders must stay on one stream until sptr_collect_stats");
  if (!x->split || c.W != f->width || c.H != f->height || x->full_G != G || x->full_R != R) {
    if (f->frame_begin != 1) return fail(c, SPTR_ERR_INVALID, "render: frame_begin must continue the accumulation (last + 1) or be 1");
    if (sync_pending(c) != SPTR_OK || sync_pending(cy) != SPTR_OK) return SPTR_ERR_HIP;
    x->full_G = G;
    x->full_R = R;
    x->full_tiles = shard_tiles(f->width, f->height, G, R);
    API_HIP(x->tiles_full.ensure((size_t)x->full_tiles * kTilePixels * 4));
    API_HIP(hipMemsetAsync(x->tiles_full.p, 0, (size_t)x->full_tiles * kTilePixels * 4, s));
  }
  x->split = true;
  c.time_by_events = cy.time_by_events = true;  // (LaunchTiming, sptr_internal.h)
  // this context's pixel buffers first (the image both lanes resolve into is cleared on s before the fork)
  bool resized = false;
  int rc = ensure_pixels(c, f->width, f->height, 2 * G, R, s, resized);
  if (rc != SPTR_OK) return rc;
  cy.image_out = static_cast<uint8_t*>(c.image.p);
  if (!serial) {
    API_HIP(hipEventRecord(x->lane_fork, s));
    API_HIP(hipStreamWaitEvent(sy, x->lane_fork, 0));
  }
  rc = render_one(x, &f0, s, nullptr);
  if (rc != SPTR_OK) return rc;
  rc = render_one(y, &f1, sy, nullptr);
  if (rc != SPTR_OK) return fail(c, rc, std::string("pixel lane: ") + cy.err);
  if (!serial) {
    API_HIP(hipEventRecord(x->lane_join, sy));
    API_HIP(hipStreamWaitEvent(s, x->lane_join, 0));
  }
  // this context's tiles (the multi-GPU gather's send buffer): the lanes' tiles interleaved
  launch_interleave_tiles(static_cast<const uint32_t*>(c.tiles.p), c.local_tiles, static_cast<const uint32_t*>(cy.tiles.p),
                          cy.local_tiles, static_cast<uint32_t*>(x->tiles_full.p), x->full_tiles, s);
  API_HIP(hipGetLastError());
  if (f->flags & SPTR_FRAME_ASYNC) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return SPTR_OK;
  }
  Context* both[2] = {&c, &cy};
  const double busy = stats ? trace_busy_ms(both, 2) : 0.0;
  sptr_stats a{}, b{};
  rc = collect_pending(c, &a);
  if (rc != SPTR_OK) return rc;
  rc = collect_pending(cy, &b);
  if (rc != SPTR_OK) return fail(c, rc, std::string("pixel lane: ") + cy.err);
  add_stats(a, b);
  a.ms_trace_busy = busy;
  if (stats) *stats = a;
  return SPTR_OK;
}

// ---- first-hit AOVs and the denoiser --------------------------------------------------------------
// Half a standard deviation: the tightest of the clips tried on the CPU (tests/test_temporal_cpu.py)
static constexpr float kHistoryClip = 0.5f;
int sptr_set_denoise(sptr_ctx* x, const sptr_denoise_params* p) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "denoise: not on a lane context");
  sptr_denoise_params q{};
  if (p) q = *p;
  if (q.iterations > 5u) return fail(c, SPTR_ERR_INVALID, "denoise: at most 5 iterations");
  if (q.normal_log2_power > 16u) return fail(c, SPTR_ERR_INVALID, "denoise: normal_log2_power above 16");
  for (float v : {q.sigma_color, q.sigma_depth, q.sigma_albedo})
    if (!(v >= 0.0f) || !std::isfinite(v)) return fail(c, SPTR_ERR_INVALID, "denoise: a sigma is negative or not finite");
  if (q.sigma_color == 0.0f) q.sigma_color = 0.5f;
  if (q.sigma_depth == 0.0f) q.sigma_depth = 0.05f;
  if (q.sigma_albedo == 0.0f) q.sigma_albedo = 0.2f;
  if (q.normal_log2_power == 0u) q.normal_log2_power = 6u;
  x->dn.p = q;  // (by value in the pass's launch arguments: a pending pass keeps the values it was enqueued with)
  return SPTR_OK;
}

// The AOV planes of (cam, W, H) on stream s, unless the cached ones were computed for them and for this
// scene state.  *ran: whether k_aov was launched.  uv: the reference / barycentric plane is wanted too
// (SPTR_AOV_UV, sptr_set_history_motion): cached planes computed without it are computed again, in place.
static int ensure_aov(sptr_ctx* x, const sptr_camera& cam, int W, int H, hipStream_t s, bool timed, bool* ran, bool uv = false) {
  Context& c = x->c;
  auto& d = x->dn;
  *ran = false;
  const bool same = d.aov_epoch == c.epoch && d.aov_W == W && d.aov_H == H && std::memcmp(&d.aov_cam, &cam, sizeof(cam)) == 0;
  if (same && (!uv || d.aov_uv)) return SPTR_OK;
  const size_t n = (size_t)W * H;
  // the side written: never the one that holds the carry's planes (history off: always side 0); the same
  // planes again (for the plane they lack): the side they are in, which gets the values it holds
  const int side = same ? d.aov_side : d.carry.valid ? d.carry.side ^ 1 : d.aov_side;
  sptr::DevBuf& nzb = side ? d.nz1 : d.nz;
  sptr::DevBuf& idb = side ? d.ids1 : d.ids;
  if (nzb.bytes < n * 16 || d.albedo.bytes < n * 16 || idb.bytes < n * 8 || (uv && d.ruv.bytes < n * 16)) {
    if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;  // a pending pass may still read the old planes
    API_HIP(nzb.ensure(n * 16));
    API_HIP(d.albedo.ensure(n * 16));
    API_HIP(idb.ensure(n * 8));
    if (uv) API_HIP(d.ruv.ensure(n * 16));
  }
  if (!same && d.last.valid && d.last.side == side) d.last.valid = false;  // its planes are overwritten below
  if (!d.flag.p) {
    API_HIP(d.flag.ensure(16));
    API_HIP(hipMemset(d.flag.p, 0, 16));
  }
  const int rg = ensure_geom_first(x);
  if (rg != SPTR_OK) return rg;
  sptr_frame fr{};
  fr.width = W;
  fr.height = H;
  fr.camera = cam;
  fr.frame_begin = 1;
  fr.max_depth = 1;
  const FrameView fv = frame_view(c, fr);
  AovView a{};
  a.nz = static_cast<float4*>(nzb.p);
  a.albedo = static_cast<float4*>(d.albedo.p);
  a.ids = static_cast<uint2*>(idb.p);
  a.ruv = uv ? static_cast<float4*>(d.ruv.p) : nullptr;
  a.tri_orig = static_cast<const uint32_t*>(c.tri_orig.p);
  a.geom_first = static_cast<const uint32_t*>(x->geom_first.p);
  a.mats = static_cast<const DevMaterial*>(c.mats.p);
  a.geom_mat = static_cast<const uint32_t*>(c.geom_mat.p);
  a.stack_overflow = static_cast<uint32_t*>(d.flag.p);
  if (timed) API_HIP(hipEventRecord(d.ev[0], s));
  launch_aov(scene_view(c), fv, a, s);
  API_HIP(hipGetLastError());
  if (timed) API_HIP(hipEventRecord(d.ev[1], s));
  d.aov_epoch = c.epoch;
  d.aov_cam = cam;
  d.aov_W = W;
  d.aov_H = H;
  d.aov_side = side;
  d.aov_uv = uv;
  ++d.aov_passes;
  *ran = true;
  return SPTR_OK;
}

// The denoise pass of the render call just enqueued on s: AOVs (if not cached), c_0, the a-trous
// iterations, the resolve into the second RGB8 image.  Direct launches, outside any captured graph.
static int enqueue_denoise(sptr_ctx* x, const sptr_frame* f, hipStream_t s) {
  Context& c = x->c;
  auto& d = x->dn;
  for (DevEvent& e : d.ev)
    if (!e) API_HIP(hipEventCreate(e.put()));
  const int W = f->width, H = f->height;
  const size_t n = (size_t)W * H;
  if (d.col[0].bytes < n * 16 || d.col[1].bytes < n * 16 || d.image.bytes < n * 3) {
    if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
    API_HIP(d.col[0].ensure(n * 16));
    API_HIP(d.col[1].ensure(n * 16));
    API_HIP(d.image.ensure(n * 3));
  }
  const bool history = d.hp.max_history != 0u;
  d.hist_ran = false;
  bool use_motion = false;
  if (history) {
    // the carry rules: a pass of another size or scene state is no history; a call that starts an
    // accumulation takes the last pass as its carry, one that continues it keeps the carry it has
    auto stale = [&](const sptr_ctx::Denoise::Pass& p) { return !p.valid || p.W != W || p.H != H || p.epoch != c.epoch; };
    if (stale(d.last)) d.last.valid = false;
    if (stale(d.carry)) d.carry.valid = false;
    if (f->frame_begin == 1) d.carry = d.last;
    // a carry of an earlier geometry (sptr_update_geometry since; it is here only with motion on, which kept
    // its epoch current) is read through the snapshot of that geometry, or not at all
    use_motion = d.carry.valid && d.carry.gen != d.geom_gen;
    if (use_motion && !(d.motion_on && d.snap_valid && d.snap_gen == d.carry.gen &&
                        c.rf.snap.bytes >= (size_t)c.num_tri_refs * 48 + (size_t)c.num_sph * 16))
      d.carry.valid = use_motion = false;
    if (d.motion_on && d.motion.bytes < n * 8) {
      if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
      API_HIP(d.motion.ensure(n * 8));
    }
    if (d.hist[0].bytes < n * 16 || d.hist[1].bytes < n * 16 || d.nz1.bytes < n * 16 || d.ids1.bytes < n * 8 ||
        d.nz.bytes < n * 16 || d.ids.bytes < n * 8 || !d.hcount.p) {
      if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
      d.last.valid = d.carry.valid = false;  // (a size none of them was made for)
      d.aov_epoch = 0;
      d.aov_side = 0;
      for (sptr::DevBuf* b : {&d.hist[0], &d.hist[1], &d.nz, &d.nz1}) API_HIP(b->ensure(n * 16));
      for (sptr::DevBuf* b : {&d.ids, &d.ids1}) API_HIP(b->ensure(n * 8));
      API_HIP(d.hcount.ensure(16));
      use_motion = false;
    }
    for (DevEvent& e : d.hev)
      if (!e) API_HIP(hipEventCreate(e.put()));
  }
  bool aov_ran = false;
  const int rc = ensure_aov(x, f->camera, W, H, s, true, &aov_ran, history && d.motion_on);
  if (rc != SPTR_OK) return rc;
  d.aov_timed = aov_ran;
  DenoiseView v{};
  v.W = W;
  v.H = H;
  v.n = f->frame_begin + f->spp - 1;
  v.nz = static_cast<const float4*>(d.aov_side ? d.nz1.p : d.nz.p);
  v.albedo = static_cast<const float4*>(d.albedo.p);
  v.sigma_z = d.p.sigma_depth;
  v.sigma_a2 = d.p.sigma_albedo * d.p.sigma_albedo;
  v.normal_log2 = d.p.normal_log2_power;
  float4* col[2] = {static_cast<float4*>(d.col[0].p), static_cast<float4*>(d.col[1].p)};
  API_HIP(hipEventRecord(d.ev[2], s));
  // two pixel lanes: this context holds the even tiles (shard 0 of 2), the lane the odd ones
  launch_dn_mean(v, static_cast<const float4*>(c.accum.p), x->split ? static_cast<const float4*>(x->lane->c.accum.p) : nullptr,
                 x->split ? 2 : 1, col[0], s);
  uint32_t cur = 0;
  if (!history) {
    for (uint32_t i = 0; i < d.p.iterations; ++i) {
      const float S = d.p.sigma_color * (1.0f / float(1u << i)) / float(v.n);  // sigma_c 2^-i / n
      launch_atrous(v, col[cur], col[cur ^ 1u], 1 << i, S * S, s);
      cur ^= 1u;
    }
  } else {
    // c_0 and the carry integrated into the history slot the carry is not in; iteration 0 reads that slot
    // directly, and the iterations divide sigma_c 2^-i by the pixel's n_eff (the slot's w)
    const uint32_t slot = d.carry.valid ? (uint32_t)(d.carry.slot ^ 1) : (d.last.valid ? (uint32_t)d.last.slot : 0u);
    ReprojView r{};
    r.c0 = col[0];
    r.ids = static_cast<const uint2*>(d.aov_side ? d.ids1.p : d.ids.p);
    if (d.carry.valid) {
      r.hist_prev = static_cast<const float4*>(d.hist[d.carry.slot].p);
      r.nz_prev = static_cast<const float4*>(d.carry.side ? d.nz1.p : d.nz.p);
      r.ids_prev = static_cast<const uint2*>(d.carry.side ? d.ids1.p : d.ids.p);
      const sptr_camera& k = d.carry.cam;
      r.pos = v3(k.pos[0], k.pos[1], k.pos[2]);
      r.fw = v3(k.forward[0], k.forward[1], k.forward[2]);
      r.rt = v3(k.right[0], k.right[1], k.right[2]);
      r.up = v3(k.up[0], k.up[1], k.up[2]);
      r.hw = k.half_width;
      r.hh = k.half_height;
      // a history seen from elsewhere is clipped to the current neighbourhood's colours; a
      // standing camera's estimates the same integrand and is taken whole
      r.clip = std::memcmp(&k, &f->camera, sizeof(k)) != 0 ? kHistoryClip : 0.0f;
      if (use_motion) {
        // shadows and reflections belong to the scene state as they belong to the view: always clipped
        r.clip = kHistoryClip;
        r.ruv = static_cast<const float4*>(d.ruv.p);
        r.tris_prev = static_cast<const float4*>(c.rf.snap.p);
        r.sph_prev = r.tris_prev + (size_t)c.num_tri_refs * 3;
        r.sph = static_cast<const float4*>(c.sph.p);
        r.num_tris = c.num_tri_refs;
        r.num_sph = c.num_sph;
        r.motion = static_cast<float2*>(d.motion.p);
      }
    }
    r.hist = static_cast<float4*>(d.hist[slot].p);
    r.max_history = float(d.hp.max_history);
    r.count = static_cast<uint32_t*>(d.hcount.p);
    sptr_frame fr{};
    fr.width = W;
    fr.height = H;
    fr.camera = f->camera;
    fr.frame_begin = 1;
    fr.max_depth = 1;
    API_HIP(hipMemsetAsync(d.hcount.p, 0, 4, s));
    API_HIP(hipEventRecord(d.hev[0], s));
    if (use_motion) launch_dn_reproject_motion(v, frame_view(c, fr), r, s);
    else launch_dn_reproject(v, frame_view(c, fr), r, s);
    API_HIP(hipEventRecord(d.hev[1], s));
    const float4* in = r.hist;
    for (uint32_t i = 0; i < d.p.iterations; ++i) {
      launch_atrous_history(v, in, col[cur], 1 << i, d.p.sigma_color * (1.0f / float(1u << i)), s);
      in = col[cur];
      cur ^= 1u;
    }
    cur ^= 1u;  // (the image the last iteration wrote)
    d.hist_ran = true;
    d.hist_carried = d.carry.valid;
    d.hist_slot = slot;
    d.motion_used = use_motion;
    d.last.gen = d.geom_gen;
    d.last.valid = true;
    d.last.slot = (int)slot;
    d.last.side = d.aov_side;
    d.last.cam = f->camera;
    d.last.W = W;
    d.last.H = H;
    d.last.epoch = c.epoch;
  }
  launch_dn_resolve(v, col[cur], static_cast<uint8_t*>(d.image.p), s);
  API_HIP(hipGetLastError());
  API_HIP(hipEventRecord(d.ev[3], s));
  d.filter_timed = true;
  d.final_col = cur;
  d.ran = true;
  return SPTR_OK;
}

int sptr_render(sptr_ctx* x, const sptr_frame* f, void* stream, sptr_stats* stats) {
  if (!x || !f) return SPTR_ERR_INVALID;
  Context& c = x->c;
  const bool dn = x->dn.p.iterations != 0u && !x->is_lane;
  if (!dn) {
    const int rc = render_call(x, f, stream, stats);
    if (rc == SPTR_OK) {
      x->dn.ran = false;
      x->dn.last_cam = f->camera;
      x->dn.last_W = f->width;
      x->dn.last_H = f->height;
    }
    return rc;
  }
  if (f->integrator != SPTR_INTEGRATOR_WAVEFRONT)
    return fail(c, SPTR_ERR_INVALID, "render: the denoiser runs with SPTR_INTEGRATOR_WAVEFRONT only (sptr_set_denoise)");
  if (f->shard_count > 1)
    return fail(c, SPTR_ERR_INVALID, "render: the denoiser needs the whole image (shard_count 1): a shard's tiles have no neighbours");
  // the call is enqueued without waiting, the pass after it on the same stream; a synchronous call is
  // then collected as sptr_collect_stats collects asynchronous ones
  sptr_frame fa = *f;
  fa.flags |= SPTR_FRAME_ASYNC;
  int rc = render_call(x, &fa, stream, nullptr);
  if (rc != SPTR_OK) return rc;
  x->dn.last_cam = f->camera;
  x->dn.last_W = f->width;
  x->dn.last_H = f->height;
  x->dn.ran = false;
  if (!(f->flags & SPTR_FRAME_NO_RESOLVE)) {
    rc = enqueue_denoise(x, f, c.pending_stream);
    if (rc != SPTR_OK) return rc;
  }
  if (f->flags & SPTR_FRAME_ASYNC) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return SPTR_OK;
  }
  return sptr_collect_stats(x, stats);
}

int sptr_read_aov(sptr_ctx* x, int kind, void* out) {
  if (!x || !out) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (kind < SPTR_AOV_ALBEDO || kind > SPTR_AOV_UV) return fail(c, SPTR_ERR_INVALID, "read_aov: unknown kind");
  if (!c.have_scene || x->dn.last_W <= 0) return fail(c, SPTR_ERR_NO_SCENE, "read_aov: nothing rendered");
  if (shading(c).mats_host.empty()) return fail(c, SPTR_ERR_NO_SCENE, "read_aov: no materials set");
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  auto& d = x->dn;
  bool ran = false;
  // (cached planes that hold the reference plane serve every kind; new ones get it as the passes ask for it)
  const int rc = ensure_aov(x, d.last_cam, d.last_W, d.last_H, c.stream, false, &ran,
                            kind == SPTR_AOV_UV || (d.motion_on && d.hp.max_history != 0u));
  if (rc != SPTR_OK) return rc;
  API_HIP(hipStreamSynchronize(c.stream));
  uint32_t flag = 0;
  API_HIP(hipMemcpy(&flag, d.flag.p, 4, hipMemcpyDeviceToHost));
  if (flag) return fail(c, SPTR_ERR_HIP, "read_aov: BVH traversal stack overflow (internal error)");
  const size_t n = (size_t)d.last_W * d.last_H;
  if (kind == SPTR_AOV_ID) {
    API_HIP(hipMemcpy(out, d.aov_side ? d.ids1.p : d.ids.p, n * 8, hipMemcpyDeviceToHost));
    return SPTR_OK;
  }
  std::vector<float> tmp(n * 4);
  API_HIP(hipMemcpy(tmp.data(), kind == SPTR_AOV_ALBEDO ? d.albedo.p : kind == SPTR_AOV_UV ? d.ruv.p : (d.aov_side ? d.nz1.p : d.nz.p),
                    n * 16, hipMemcpyDeviceToHost));
  float* o = static_cast<float*>(out);
  for (size_t i = 0; i < n; ++i) {
    if (kind == SPTR_AOV_UV) {
      o[i * 2 + 0] = tmp[i * 4 + 1];
      o[i * 2 + 1] = tmp[i * 4 + 2];
    } else if (kind == SPTR_AOV_DEPTH) {
      o[i] = tmp[i * 4 + 3];
    } else {
      o[i * 3 + 0] = tmp[i * 4 + 0];
      o[i * 3 + 1] = tmp[i * 4 + 1];
      o[i * 3 + 2] = tmp[i * 4 + 2];
    }
  }
  return SPTR_OK;
}

int sptr_read_denoised(sptr_ctx* x, float* rgb) {
  if (!x || !rgb) return SPTR_ERR_INVALID;
  Context& c = x->c;
  auto& d = x->dn;
  if (!d.ran) return fail(c, SPTR_ERR_INVALID, "read_denoised: the last render call ran no denoise pass (sptr_set_denoise)");
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  const size_t n = (size_t)d.last_W * d.last_H;
  std::vector<float> tmp(n * 4);
  API_HIP(hipMemcpy(tmp.data(), d.col[d.final_col].p, n * 16, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    rgb[i * 3 + 0] = tmp[i * 4 + 0];
    rgb[i * 3 + 1] = tmp[i * 4 + 1];
    rgb[i * 3 + 2] = tmp[i * 4 + 2];
  }
  return SPTR_OK;
}

int sptr_denoise_info(const sptr_ctx* x, double* ms_aov, double* ms_filter, uint32_t* aov_passes) {
  if (!x) return SPTR_ERR_INVALID;
  const auto& d = x->dn;
  float a = 0.0f, fl = 0.0f;
  if (d.ran && d.filter_timed) {
    if (hipEventSynchronize(d.ev[3]) != hipSuccess) return SPTR_ERR_HIP;
    if (d.aov_timed) (void)hipEventElapsedTime(&a, d.ev[0], d.ev[1]);
    (void)hipEventElapsedTime(&fl, d.ev[2], d.ev[3]);
  }
  if (ms_aov) *ms_aov = a;
  if (ms_filter) *ms_filter = fl;
  if (aov_passes) *aov_passes = d.aov_passes;
  return SPTR_OK;
}

// ---- temporal reprojection ------------------------------------------------------------------------
static int set_seed_offset_one(sptr_ctx* x, uint32_t offset) {
  if (!x) return SPTR_ERR_INVALID;
  x->c.seed_offset = offset;  // (a k_frame_dyn argument: no captured graph depends on it)
  return SPTR_OK;
}
int sptr_set_seed_offset(sptr_ctx* x, uint32_t offset) {
  const int rc = set_seed_offset_one(x, offset);
  return rc == SPTR_OK ? lane_forward(x, set_seed_offset_one(x->lane, offset)) : rc;
}

int sptr_set_denoise_history(sptr_ctx* x, const sptr_history_params* p) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "denoise history: not on a lane context");
  sptr_history_params q{};
  if (p) q = *p;
  if (q.max_history > 1024u) return fail(c, SPTR_ERR_INVALID, "denoise history: max_history above 1024");
  for (uint32_t r : q.reserved)
    if (r != 0u) return fail(c, SPTR_ERR_INVALID, "denoise history: reserved words must be 0");
  auto& d = x->dn;
  d.hp = q;
  // the history held is dropped; so is the plane cache, so that the next pass writes side 0 again (a pending
  // pass keeps the buffers it was enqueued with: nothing is freed here)
  d.last.valid = d.carry.valid = false;
  d.hist_ran = false;
  d.aov_epoch = 0;
  d.aov_side = 0;
  return SPTR_OK;
}

int sptr_read_history(sptr_ctx* x, float* rgbm) {
  if (!x || !rgbm) return SPTR_ERR_INVALID;
  Context& c = x->c;
  auto& d = x->dn;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "read_history: not on a lane context");
  if (!d.ran || !d.hist_ran)
    return fail(c, SPTR_ERR_INVALID, "read_history: the last render call ran no pass with history on (sptr_set_denoise_history)");
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  API_HIP(hipMemcpy(rgbm, d.hist[d.hist_slot].p, (size_t)d.last_W * d.last_H * 16, hipMemcpyDeviceToHost));
  return SPTR_OK;
}

int sptr_history_info(sptr_ctx* x, uint32_t* reprojected, double* ms_reproject, uint32_t* carried) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "history_info: not on a lane context");
  const auto& d = x->dn;
  uint32_t n = 0;
  float ms = 0.0f;
  const bool ran = d.ran && d.hist_ran;
  if (ran) {
    API_HIP(hipSetDevice(c.device));
    API_HIP(hipEventSynchronize(d.ev[3]));  // the pass's end
    (void)hipEventElapsedTime(&ms, d.hev[0], d.hev[1]);
    API_HIP(hipMemcpy(&n, d.hcount.p, 4, hipMemcpyDeviceToHost));
  }
  if (reprojected) *reprojected = n;
  if (ms_reproject) *ms_reproject = ms;
  if (carried) *carried = ran && d.hist_carried ? 1u : 0u;
  return SPTR_OK;
}

// ---- motion vectors: the history across geometry updates -----------------------------
int sptr_set_history_motion(sptr_ctx* x, uint32_t on) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "history motion: not on a lane context");
  auto& d = x->dn;
  d.motion_on = on != 0u;
  // the history held and the snapshot are dropped, as sptr_set_denoise_history drops the history (nothing
  // is freed here: a pending pass keeps the buffers it was enqueued with)
  d.last.valid = d.carry.valid = false;
  d.snap_valid = false;
  d.hist_ran = false;
  d.motion_used = false;
  d.aov_epoch = 0;
  d.aov_side = 0;
  return SPTR_OK;
}

int sptr_read_motion(sptr_ctx* x, float* out) {
  if (!x || !out) return SPTR_ERR_INVALID;
  Context& c = x->c;
  auto& d = x->dn;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "read_motion: not on a lane context");
  if (!d.ran || !d.hist_ran || !d.motion_used)
    return fail(c, SPTR_ERR_INVALID, "read_motion: the last render call ran no pass on the motion path (sptr_set_history_motion)");
  API_HIP(hipSetDevice(c.device));
  if (sync_pending(c) != SPTR_OK) return SPTR_ERR_HIP;
  API_HIP(hipMemcpy(out, d.motion.p, (size_t)d.last_W * d.last_H * 8, hipMemcpyDeviceToHost));
  return SPTR_OK;
}

int sptr_motion_info(sptr_ctx* x, uint32_t* snapshots, double* ms_snapshot, uint32_t* used) {
  if (!x) return SPTR_ERR_INVALID;
  Context& c = x->c;
  if (x->is_lane) return fail(c, SPTR_ERR_INVALID, "motion_info: not on a lane context");
  const auto& d = x->dn;
  if (snapshots) *snapshots = c.rf.snapshots;
  if (ms_snapshot) *ms_snapshot = c.rf.ms_snapshot;
  if (used) *used = d.ran && d.hist_ran && d.motion_used ? 1u : 0u;
  return SPTR_OK;
}

// The shading setters change only this context: a pixel lane reads its parent's shading state
// (shading()).  A lane render still pending reads the parent's device buffers, so the setters that
// replace them wait for it first; every shading change drops the lane's captured graph (epoch).
static int lane_shading_sync(sptr_ctx* x) {
  if (!x || !x->lane || x->lane->c.pending == 0) return SPTR_OK;
  if (sync_pending(x->lane->c) != SPTR_OK) return fail(x->c, SPTR_ERR_HIP, std::string("pixel lane: ") + x->lane->c.err);
  return SPTR_OK;
}
static int lane_shading_changed(sptr_ctx* x, int rc) {
  if (x && x->lane) ++x->lane->c.epoch;
  return rc;
}

int sptr_set_debug_mode(sptr_ctx* x, int mode) { return lane_shading_changed(x, set_debug_mode_one(x, mode)); }

int sptr_set_leaf_size(sptr_ctx* x, uint32_t n) {
  const int rc = set_leaf_size_one(x, n);
  return rc == SPTR_OK ? lane_forward(x, set_leaf_size_one(x ? x->lane : nullptr, n)) : rc;
}

int sptr_set_tree_order(sptr_ctx* x, uint32_t mode) {
  const int rc = set_tree_order_one(x, mode);
  return rc == SPTR_OK ? lane_forward(x, set_tree_order_one(x ? x->lane : nullptr, mode)) : rc;
}

int sptr_tree_info(const sptr_ctx* x, sptr_tree_order_info* out) {
  if (!x || !out) return SPTR_ERR_INVALID;
  const Context::TreeInfo& t = x->c.tree_info;
  out->order = t.order;
  out->fallback = t.fallback;
  out->depth = t.depth;
  out->num_leaves = t.leaves;
  out->cost_sah = t.cost_sah;
  out->cost_morton = t.cost_morton;
  return SPTR_OK;
}

int sptr_set_bvh_width(sptr_ctx* x, uint32_t width) {
  const int rc = set_bvh_width_one(x, width);
  return rc == SPTR_OK ? lane_forward(x, set_bvh_width_one(x ? x->lane : nullptr, width)) : rc;
}

int sptr_set_tail_depth(sptr_ctx* x, uint32_t depth) {
  const int rc = set_tail_depth_one(x, depth);
  return rc == SPTR_OK ? lane_forward(x, set_tail_depth_one(x ? x->lane : nullptr, depth)) : rc;
}

int sptr_set_bounce_chain(sptr_ctx* x, uint32_t mode) {
  const int rc = set_bounce_chain_one(x, mode);
  return rc == SPTR_OK ? lane_forward(x, set_bounce_chain_one(x ? x->lane : nullptr, mode)) : rc;
}

int sptr_set_sky_split(sptr_ctx* x, uint32_t mode, uint32_t bulk_threads) {
  const int rc = set_sky_split_one(x, mode, bulk_threads);
  return rc == SPTR_OK ? lane_forward(x, set_sky_split_one(x ? x->lane : nullptr, mode, bulk_threads)) : rc;
}

int sptr_sky_split_info(sptr_ctx* x, uint32_t* bulk_threads) {
  if (!x || !bulk_threads) return SPTR_ERR_INVALID;
  *bulk_threads = x->c.sky_split_last;
  return SPTR_OK;
}

int sptr_set_shadow_entries(sptr_ctx* x, uint32_t mode) {
  const int rc = set_shadow_entries_one(x, mode);
  return rc == SPTR_OK ? lane_forward(x, set_shadow_entries_one(x ? x->lane : nullptr, mode)) : rc;
}

int sptr_shadow_entries_info(sptr_ctx* x, sptr_shadow_entries_info_t* out) {
  if (!x || !out) return SPTR_ERR_INVALID;
  Context& c = x->c;
  std::memset(out, 0, sizeof(*out));
  out->mode = c.shadow_mode;
  out->builds = c.se.builds;
  if (!shade_view(c).shadow_entry) return SPTR_OK;  // no current table
  const uint32_t R = c.se.frame.R, n = R * R;
  std::vector<uint32_t> words(n);
  API_HIP(hipSetDevice(c.device));
  API_HIP(hipDeviceSynchronize());  // (the build ran on the stream of the call that made it)
  API_HIP(hipMemcpy(words.data(), c.se.table.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  uint32_t below = 0u, none = 0u;
  for (uint32_t w : words) {
    below += w != c.root ? 1u : 0u;
    none += w == kNoHit ? 1u : 0u;
  }
  out->cells = R;
  out->bytes = n * 4u;
  out->cells_below_root = (float)below / (float)n;
  out->cells_unoccluded = (float)none / (float)n;
  return SPTR_OK;
}

int sptr_set_split_refs(sptr_ctx* x, uint32_t max_pieces) {
  const int rc = set_split_refs_one(x, max_pieces);
  return rc == SPTR_OK ? lane_forward(x, set_split_refs_one(x ? x->lane : nullptr, max_pieces)) : rc;
}

int sptr_set_stragglers(sptr_ctx* x, uint32_t lanes) {
  const int rc = set_stragglers_one(x, lanes);
  return rc == SPTR_OK ? lane_forward(x, set_stragglers_one(x ? x->lane : nullptr, lanes)) : rc;
}

int sptr_set_wave_paths(sptr_ctx* x, uint64_t max_paths) {
  const int rc = set_wave_paths_one(x, max_paths);
  return rc == SPTR_OK ? lane_forward(x, set_wave_paths_one(x ? x->lane : nullptr, max_paths)) : rc;
}

int sptr_set_materials(sptr_ctx* x, const sptr_material* m, uint32_t n) {
  const int rs = lane_shading_sync(x);
  if (rs != SPTR_OK) return rs;
  const int rc = lane_shading_changed(x, set_materials_one(x, m, n));
  if (rc != SPTR_OK || !x->lane) return rc;
  // the lane's slot table follows this context's geom_mat; without a current copy of the scene it has none
  if (!x->lane_scene) {
    x->lane->c.prim_mat_n = 0u;
    return rc;
  }
  return lane_forward(x, build_prim_materials(x->lane->c));
}

int sptr_set_lights(sptr_ctx* x, const sptr_light* l, uint32_t n) {
  return lane_shading_changed(x, set_lights_one(x, l, n));  // (by value in every launch's arguments)
}

int sptr_set_environment(sptr_ctx* x, const sptr_environment* e) {
  const int rs = lane_shading_sync(x);
  if (rs != SPTR_OK) return rs;
  return lane_shading_changed(x, set_environment_one(x, e));
}

int sptr_set_launch_mode(sptr_ctx* x, uint32_t mode) {
  const int rc = set_launch_mode_one(x, mode);
  return rc == SPTR_OK ? lane_forward(x, set_launch_mode_one(x->lane, mode)) : rc;
}

}  // extern "C"
