/* sptr_hip.h — C ABI of libsptr_hip.so, the MI355X (gfx950) wavefront path-tracing backend.
 *
 * Drop-in boundary: these entry points are what a binding for the reference's GPU backend slot
 * needs.  The reference has no abstract backend interface; GLRenderer::renderLoop drives the
 * concrete OptixBackend class (/root/reference/src/GLRenderer.cpp:116-176) through the surface in
 * /root/reference/include/backends/OptixBackend.h:39-71.  Mapping (each entry cites what it replaces):
 *
 *   sptr_create / sptr_destroy   <- OptixBackend::OptixBackend / destroy()        (OptixBackend.h:41-66)
 *   sptr_upload_scene            <- OptixBackend::build(const SceneDesc&)         (OptixBackend.h:46;
 *                                   GAS/IAS builds at src/backends/OptixBackend.cpp:916-1308), fed the
 *                                   world-space flattening of EmbreeBackend::build
 *                                   (src/backends/EmbreeBackend.cpp:18-193) so geomIDs match the CPU path
 *   sptr_set_materials           <- OptixBackend::setMaterialManager              (OptixBackend.h:59)
 *   sptr_set_lights              <- OptixBackend::setLightManager                 (OptixBackend.h:63)
 *   sptr_set_environment         <- OptixBackend::setEnvironment                  (OptixBackend.h:55)
 *   sptr_render + sptr_read_rgb8 <- OptixBackend::render(uint8_t* rgb,w,h,Camera) (OptixBackend.h:51;
 *                                   src/backends/OptixBackend.cpp:1506-1850)
 *   sptr_set_debug_mode          <- OptixBackend::setDebugMode                    (OptixBackend.h:71)
 *
 * Semantics are those of the CPU Embree wavefront integrator (src/wavefront/wf_pt_cpu.cpp:61-255
 * driven by src/GLRenderer.cpp:353-435), not of the OptiX device programs.
 *
 * Conventions: 0 = OK, negative = error (sptr_last_error has the text); no exceptions, no exit()
 * across the ABI.  The caller owns every host buffer; upload calls copy.  One context per GPU, used
 * from one host thread at a time; contexts are independent.  Device pointers handed out stay valid
 * until the next render call with a different size, or sptr_destroy.
 */
#ifndef SPTR_HIP_H
#define SPTR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPTR_ABI_VERSION 9

enum sptr_status {
  SPTR_OK = 0,
  SPTR_ERR_INVALID = -1,   /* bad argument / shape */
  SPTR_ERR_HIP = -2,       /* HIP runtime error */
  SPTR_ERR_NO_SCENE = -3,  /* render before upload / materials */
  SPTR_ERR_OOM = -4,
  SPTR_ERR_NO_DEVICE = -5
};

typedef struct sptr_ctx sptr_ctx;

/* World-space flattened scene, geomID order of EmbreeBackend::build: one triangle geometry per
 * SceneDesc instance (geomIDs 0..num_tri_geoms-1), then one geometry per analytic sphere. */
typedef struct sptr_scene {
  const float* positions; /* 3 floats per vertex, world space */
  uint32_t num_verts;
  const uint32_t* indices; /* 3 global vertex indices per triangle */
  uint32_t num_tris;
  const uint32_t* tri_geom_first; /* num_tri_geoms+1 prefix offsets into the triangle list */
  uint32_t num_tri_geoms;
  const float* spheres; /* cx, cy, cz, radius per sphere */
  uint32_t num_spheres;
  const uint32_t* geom_material; /* geomID -> material index (EmbreeBackend::geomMaterialId_) */
} sptr_scene;

/* One entry of MaterialManager's table (include/Material.h:19-39, values after the ctor clamps). */
typedef struct sptr_material {
  float albedo[3];
  float metallic;
  float roughness;
  float emission[3];
  float ior;
  int32_t type; /* 0 PBR, 1 DIELECTRIC (informational; shading follows metallic/ior) */
  float pad[2];
} sptr_material;

/* LightManager entry (include/Light.h:43-81): type 0 = directional (v = direction of the light's
 * rays, as passed to addDirectionalLight), 1 = point (v = position). */
typedef struct sptr_light {
  int32_t type;
  float v[3];
  float color[3];
  float intensity;
} sptr_light;

/* EnvironmentManager state: faces == NULL selects the procedural sky
 * (src/EnvironmentManager.cpp:35-61); otherwise 6 cube faces (+X,-X,+Y,-Y,+Z,-Z) of size*size RGB
 * floats, sampled bilinearly as Cubemap::sample (src/Cubemap.cpp:82-180).  2 <= size <= 26754 (the
 * device indexes texels in 32 bits: 6 * size * size < 2^32); any other size is SPTR_ERR_INVALID,
 * refused before faces is read. */
typedef struct sptr_environment {
  const float* faces;
  int32_t size;
  float intensity; /* 0.8 in the reference (EnvironmentManager.h:12) */
  float max_clamp; /* 5.0 */
} sptr_environment;

/* Camera basis as Camera::updateCameraVectors leaves it (src/Camera.cpp:33-50). */
typedef struct sptr_camera {
  float pos[3];
  float forward[3];
  float right[3];
  float up[3];
  float half_width;
  float half_height;
} sptr_camera;

enum sptr_frame_flags {
  SPTR_FRAME_TIMING = 1u,     /* per-stage times (adds sync at the end of the call).  The trace, fused-bounce
                                 and shadow launches time themselves (one launch chain's trace launches on
                                 the device wall clock, up to 4096 per collection window — later ones in
                                 the window go untimed; the shadow launches and the pixel lanes' launches
                                 by their dispatch events); the other stages by HIP events around them */
  SPTR_FRAME_NO_RESOLVE = 2u, /* skip the tonemap/resolve pass */
  SPTR_FRAME_COUNT_VISITS = 4u, /* one instrumented trace pass: count BVH node / primitive fetches */
  SPTR_FRAME_ASYNC = 8u, /* enqueue only: return without waiting; stats are left zero and the call's
                            counters and stage times accumulate until sptr_collect_stats */
  SPTR_FRAME_TIMING_TRACE = 16u, /* the trace and shadow launches' times only (ms_trace,
                                   ms_trace0, trace_launches, ms_shadow, shadow_launches): the other
                                   stages run back to back, and ms_total / ms_cull stay 0 */
  SPTR_FRAME_NO_CULL = 32u, /* diagnostic: bounce 0 traverses every camera ray, without the pixel-frustum
                               cull (the image is the same either way) */
  SPTR_FRAME_RECULL = 64u /* recompute the bounce-0 pixel-frustum cull mask in this call even when the
                             camera and scene are unchanged (the per-frame cost of a moving camera;
                             bench.py times its steps this way) */
};

/* Integrators (sptr_frame.integrator).  The reference selects between them per frame in
 * GLRenderer::renderLoop (src/GLRenderer.cpp:163-176):
 *   SPTR_INTEGRATOR_WAVEFRONT : WavefrontPathTracerCPU semantics (src/wavefront/wf_pt_cpu.cpp:61-255,
 *                               seeded and resolved by GLRenderer::renderWavefrontTileTask, :353-435):
 *                               one jittered sample per frame, deterministic wang-hash RNG, ACES +
 *                               gamma at resolve.  The default, and the parity / benchmark path.
 *   SPTR_INTEGRATOR_PATHTRACER: PathTracer semantics, the reference's default CPU integrator
 *                               (src/PathTracer.cpp:113-391): pixel-corner rays without jitter,
 *                               samples_per_frame recursive samples per frame averaged, ACES + gamma
 *                               per frame, tonemapped frames accumulated.  The reference draws from a
 *                               non-reproducible mt19937(random_device); this mode uses a
 *                               deterministic per-(pixel, frame, sample) wang-hash stream instead
 *                               (DESIGN.md), so it matches the reference in distribution only.
 *   SPTR_INTEGRATOR_OPTIX     : the shading of the reference's OptiX device programs
 *                               (src/optix/device_programs.cu:220-690, 854-899; the 'G' key's GPU
 *                               path): pixel-centre rays, wang_hash((pixel+1) ^ (frame*9781+1)) seeds,
 *                               tmin 1e-3, direct sun light without shadow rays, GGX-sampled metals,
 *                               delta dielectrics, depth-cap normal visualisation, exposure 2.2 +
 *                               Reinhard + gamma at resolve.  Exact functions replace CUDA's
 *                               approximate rsqrtf/sincosf. */
enum sptr_integrator { SPTR_INTEGRATOR_WAVEFRONT = 0, SPTR_INTEGRATOR_PATHTRACER = 1, SPTR_INTEGRATOR_OPTIX = 2 };

/* One render call = `spp` progressive frames starting at accumulation index frame_begin (1-based,
 * as GLRenderer::m_accumulated_samples; frame_begin == 1 clears the accumulation).  A wavefront
 * frame is one sample per pixel; a PathTracer frame is samples_per_frame samples (0 = 4, the
 * reference's setupPathTracer, src/main.cpp:105-113).  Pixels are rendered in 32x32 tiles
 * (GLRenderer.h:36); with shard_count > 1 only tiles t with t % shard_count == shard_rank are
 * rendered (interleaved multi-GPU sharding). */
typedef struct sptr_frame {
  int32_t width, height;
  sptr_camera camera;
  uint32_t frame_begin;
  uint32_t spp;
  uint32_t max_depth;
  int32_t shard_rank, shard_count;
  uint32_t flags;
  uint32_t integrator;        /* sptr_integrator */
  uint32_t samples_per_frame; /* PathTracer mode only */
} sptr_frame;

typedef struct sptr_stats {
  uint64_t rays_closest; /* closest-hit queries (primary + extension) = rtcIntersect1 calls */
  uint64_t rays_shadow;  /* any-hit queries = rtcOccluded1 calls */
  uint64_t samples;      /* pixel samples completed */
  uint64_t waves;        /* wavefront batches launched */
  double ms_total;       /* SPTR_FRAME_TIMING: wall time of the call on the device stream */
  double ms_raygen, ms_trace, ms_shade, ms_shadow, ms_accum; /* SPTR_FRAME_TIMING only; raygen is fused
                                                                into the bounce-0 trace (ms_raygen = 0);
                                                                ms_accum includes the culled pixels'
                                                                environment sums (k_sky) */
  uint64_t trace_launches;
  uint64_t node_visits, tri_tests, sphere_tests; /* SPTR_FRAME_COUNT_VISITS only */
  uint64_t shadow_node_visits, shadow_prim_tests;
  double ms_trace0, ms_shade0; /* SPTR_FRAME_TIMING: bounce-0 parts of ms_trace / ms_shade */
  uint64_t rays_tail;          /* closest-hit queries (of rays_closest) traced by the path-per-thread tail */
  double ms_tail;              /* SPTR_FRAME_TIMING: the tail launch */
  /* ABI 4: the rays the trace stage (ms_trace / trace_launches) actually traversed.  Camera rays of
   * frustum-culled pixels count as closest-hit queries (rays_closest) but never reach a traversal:
   * traced_primary = unculled pixel samples of bounce 0, traced_bounce = queued rays of bounces >= 1
   * traced by the wavefront trace kernels (not the fused bounce or path-per-thread tail kernels). */
  uint64_t traced_primary, traced_bounce;
  uint64_t node_visits_primary, tri_tests_primary, sphere_tests_primary; /* SPTR_FRAME_COUNT_VISITS: the
                                                                           bounce-0 part of node_visits,
                                                                           tri_tests, sphere_tests */
  double ms_cull;              /* SPTR_FRAME_TIMING: the pixel-cull launches (k_cull) */
  uint64_t cull_launches;      /* calls whose cull mask was (re)computed */
  uint64_t shadow_launches;    /* SPTR_FRAME_TIMING / _TIMING_TRACE: shadow-stage launches (ms_shadow) */
  /* Per bounce d (index 7: bounces >= 7): rays the wavefront trace kernels traversed (every call) and
   * their BVH node visits (SPTR_FRAME_COUNT_VISITS).  Histograms (SPTR_FRAME_COUNT_VISITS): closest-hit
   * rays of the trace kernels / any-hit queries of the shadow stage by node visits, bin b counting the
   * rays with 2^(b-1) <= visits < 2^b (bin 0: no visit, bin 15: >= 2^14). */
  uint64_t traced_by_depth[8];
  uint64_t nodes_by_depth[8];
  uint64_t trace_visit_hist[16];
  uint64_t shadow_visit_hist[16];
  uint64_t hits_primary, hits_bounce; /* SPTR_FRAME_COUNT_VISITS: closest hits the trace kernels found
                                         (of traced_primary / traced_bounce) */
  uint64_t paths_handed_off;          /* ABI 6: paths a bounce trace handed to the straggler kernel
                                         (sptr_set_stragglers) */
  uint64_t strag_visits[3];           /* ABI 6: node visits, triangle and sphere tests of the handed-off
                                         rays' walks made by the straggler kernel (every call) */
  double ms_trace_busy;               /* ABI 8, SPTR_FRAME_TIMING / _TIMING_TRACE: the trace launches'
                                         busy time, the union of their intervals (= ms_trace for one
                                         launch chain; two pixel lanes' trace launches overlap) */
  uint64_t traced_fused;              /* ABI 8: queued rays of bounces >= 1 traced by the fused bounce
                                         kernel (k_bounce: trace and shading of a bounce in one launch,
                                         LDS-staged scenes; every call).  Its launches count as trace
                                         launches (ms_trace, trace_launches, ms_trace_busy), and its rays
                                         are in traced_by_depth, not in traced_bounce */
} sptr_stats;

/* ---- context ---------------------------------------------------------------------------------- */
int sptr_abi_version(void);
/* Contexts alive at once in one process: every context creates six streams, which the HIP runtime maps onto
 * the process's four hardware queues.  The library is tested with the session's context and up to two more
 * alive at once.  A process that held eight (and had filled the library's per-process table of launch sizes, as
 * it stood then) saw a later launch-graph replay of the first context end in a host segmentation fault inside
 * the HIP runtime; which of the two conditions it takes is not established, so hold as few as
 * the work needs and destroy the ones that are done. */
int sptr_create(int device, sptr_ctx** out);
int sptr_destroy(sptr_ctx* ctx);
const char* sptr_last_error(const sptr_ctx* ctx);
int sptr_set_debug_mode(sptr_ctx* ctx, int mode);
/* Largest number of paths (pixels x samples) processed per wavefront batch (at most 2^30).
 * 0 = default: 2^29, capped by what half of the device's free memory holds (at least 2^24). */
int sptr_set_wave_paths(sptr_ctx* ctx, uint64_t max_paths);
/* First bounce traced path-per-thread (one launch carries every surviving path to its end; earlier
 * bounces run as trace/shade/shadow wavefront stages).  0 = automatic: scenes traversed from L2/HBM
 * 2 (L2-resident) or 3; LDS-staged scenes 4 for batches of at most 2^25 paths (e.g. the per-rank share
 * of a sharded 1080p frame), none for larger batches; >= max_depth = none.  The image and the query
 * counts do not depend on it. */
int sptr_set_tail_depth(sptr_ctx* ctx, uint32_t depth);
/* Bounce chain (a symbol added within ABI 9: no existing struct or entry point changed): the wavefront
 * bounces 1 .. tail_depth-1 of an LDS-staged one-light scene (with bounce 0's shading) run as one launch, in
 * which every block traces the continuation rays it wrote itself, instead of one launch per bounce.
 * 0 = automatic (the default): off for every batch size measured so far (no gain outside the run-to-run
 * spread); 1 = off; 2 = on wherever it applies (other scenes and the visit-count pass
 * keep their launch sequence whatever the setting).  The image and the counters do not
 * depend on it. */
int sptr_set_bounce_chain(sptr_ctx* ctx, uint32_t mode);
/* Sky split (symbols added within ABI 9: no existing struct or entry point changed): in a lane-group bounce 0
 * of an LDS-staged scene with a cull mask, the bulk of the culled pixels, whose camera rays all miss, is summed
 * one thread per pixel by a launch of its own, every thread the same number of pixels, and the lane groups
 * take the unculled pixels and the culled remainder.  mode 0 = automatic (the default): on for batches with at
 * least 5/4 pixels per bulk thread (the pixel lanes of a 1080p frame and of its 2-way shard); 1 = off; 2 = on
 * wherever that bounce 0 runs.  bulk_threads: 0 = automatic (three quarters of the launch's resident threads);
 * any other value is for tests.  The image and the
 * counters do not depend on either.  sptr_sky_split_info: the bulk thread count of the last wavefront call's
 * first batch, 0 if it did not split. */
int sptr_set_sky_split(sptr_ctx* ctx, uint32_t mode, uint32_t bulk_threads);
int sptr_sky_split_info(sptr_ctx* ctx, uint32_t* bulk_threads);
/* Shadow entries (symbols added within ABI 9: no existing struct or entry point changed): for a scene staged in
 * LDS with one directional light, whose shadow rays are traced in place by the shading launches, a table of
 * R x R light-space cells holds where a shadow ray whose origin projects into the cell starts its walk of the
 * BVH: nowhere (nothing can occlude it), at a node, or at one leaf's sub-range.  The table is built at the
 * first render call that qualifies and serves every call until the scene (upload, refit, transforms) or the
 * light changes.  mode 0 = off; 1 = automatic (the default): the first table after an upload is built by a
 * wavefront call of at least 2^23 samples, a table that replaces one ended by a refit, a transform update or
 * another light direction only by a call of at least 2^27 (an animated scene walks from the root below that
 * and pays no build), and a cached table is used by every call; 2 = built by any wavefront call.  The image and the ray counters
 * do not depend on it.  sptr_shadow_entries_info: the setting, the builds so far and, while a table is
 * current, its cells per side, its bytes, and the shares of cells whose walk starts below the root and of
 * cells whose rays are unoccluded without a walk. */
typedef struct sptr_shadow_entries_info_t {
  uint32_t mode, cells, bytes, builds;
  float cells_below_root, cells_unoccluded;
} sptr_shadow_entries_info_t;
int sptr_set_shadow_entries(sptr_ctx* ctx, uint32_t mode);
int sptr_shadow_entries_info(sptr_ctx* ctx, sptr_shadow_entries_info_t* out);
/* Maximum primitives per BVH leaf range (1..16; 0 = automatic, the default: 8 for scenes staged in
 * LDS, 1 otherwise); applies to the next sptr_upload_scene. */
int sptr_set_leaf_size(sptr_ctx* ctx, uint32_t max_prims);
/* Order of the BVH2 of a scene staged in LDS with leaf ranges (leaf size > 1, no split references).
 * 0 = automatic (the default): the references are ordered by a sweep-SAH tree built on the host at upload,
 * which separates spheres from triangles and takes fewer primitive tests per ray than the Morton-order
 * tree; 1 = Morton order.  Applies to the next sptr_upload_scene.  Hits do not depend on it, except which
 * of two exactly tying primitives is reported.  Every other scene is in Morton order either way.
 * sptr_tree_info, about the last upload: order = 0 SAH / 1 Morton; fallback = why Morton (0 = SAH in use,
 * 1 = asked for, 2 = the scene is not of the kind above, 3 = a SAH path longer than 63 bits, 4 = SAH tree
 * deeper than the Morton tree and than the walk's LDS stack, 5 = modelled cost not below the Morton
 * tree's); depth and num_leaves of the tree in use, cost_sah / cost_morton = the builder's modelled cost of
 * either tree (all four 0 when fallback is 1 or 2). */
int sptr_set_tree_order(sptr_ctx* ctx, uint32_t mode);
typedef struct sptr_tree_order_info {
  uint32_t order, fallback, depth, num_leaves;
  double cost_sah, cost_morton;
} sptr_tree_order_info;
int sptr_tree_info(const sptr_ctx* ctx, sptr_tree_order_info* out);
/* Split references (early split clipping) for scenes traversed from L2/HBM: a triangle whose box is
 * much larger than the triangle (a sliver lying across the axes) is referenced up to max_pieces times,
 * each reference bounding one piece of it, so that rays near a fan of slivers stop testing every
 * sliver's box.  0 = default (1: no splits — measured no faster on the 10M-triangle mesh),
 * else a power of two up to 32; applies to the next sptr_upload_scene.  Results do not depend on it
 * (each reference tests the same triangle). */
int sptr_set_split_refs(sptr_ctx* ctx, uint32_t max_pieces);
/* Straggler hand-off (ABI 6) for scenes traversed from HBM (a wide BVH beyond an XCD's L2): once a
 * wave of a bounce trace has no rays left to start and at most `lanes` of its 64 lanes are still
 * tracing, those rays are handed to a path-per-thread kernel beside the launch chain, which resumes
 * each walk from the state the trace saved (node, stack, closest hit so far) and finishes the path,
 * so the launch no longer lasts as long as its longest ray.
 * 0 = off, 1..64 (default 12).  Results do not depend on it (each path makes the same operations in
 * the same order wherever it runs); sptr_stats::paths_handed_off counts the paths. */
int sptr_set_stragglers(sptr_ctx* ctx, uint32_t lanes);
/* 0 (default): a render-call shape of at least 2^24 samples seen twice in a row (same frame parameters
 * except frame_begin, same state) is captured into a hipGraph once and replayed from then on — one
 * graph launch per call instead of ~20 kernel launches, the per-call accumulation index passed as a
 * kernel-node argument — except a call whose launches fork to the side streams (the graph executor
 * runs a graph's branches one after another, so such calls launch directly; a shape whose capture
 * fails or is rejected also launches directly from then on).  Smaller calls (the 1-spp interactive
 * frames) launch directly: their replays were no faster and had wall-time spikes;
 * 1: direct kernel launches for every call; 2: direct launches, all on the render stream (no launch
 * overlapped on the context's second stream); 3: as 0 for every repeated shape, whatever its size or
 * side-stream launches.
 * Calls with stage timing (SPTR_FRAME_TIMING*) launch directly in every mode.  Results are identical
 * in every mode. */
int sptr_set_launch_mode(sptr_ctx* ctx, uint32_t mode);
/* Pixel lanes (ABI 8): 2 = a wavefront call renders the even and the odd half of its shard's tiles as
 * two launch chains on two streams of the same GPU, each with its own buffers (the context holds a
 * second, internal context with a copy of the scene), so that each chain's launch tails run beside the
 * other's work; 1 = one chain; 0 (default) = two lanes for calls of >= 2^24 samples, one chain otherwise.
 * Only scenes staged into LDS (sptr_scene_layout_info: lds_bytes > 0) and the wavefront integrator run
 * in two lanes; other calls run as one chain whatever the setting.  An accumulation keeps the lane mode
 * of its first call (frame_begin 1); a change of setting or scene starts a new one.
 * Results are identical either way (each pixel's samples are the same operations in the same order);
 * sptr_tiles_device, sptr_read_rgb8 and sptr_read_accum return the shard as one chain would. */
int sptr_set_pixel_lanes(sptr_ctx* ctx, uint32_t lanes);
/* The pixel-lane setting (0, 1 or 2) and whether the current accumulation runs in two lanes (0 / 1). */
int sptr_pixel_lanes_info(const sptr_ctx* ctx, uint32_t* requested, uint32_t* active);
/* The launch graph the context holds (launch modes 0 and 3): valid = 1 once a call shape was captured; its
 * node count, dependency edges and the nodes on its longest path; captures = graphs captured so far;
 * capture_status = the hipError_t of the last capture attempt that fell back to direct launches (0:
 * none).  Every captured graph is checked to be acyclic before it is instantiated (a rejected capture
 * falls back to direct launches for that shape, reported here and by sptr_capture_error).  Any
 * pointer may be NULL. */
int sptr_graph_info(const sptr_ctx* ctx, uint32_t* valid, uint32_t* nodes, uint32_t* edges, uint32_t* depth,
                    uint32_t* captures, int32_t* capture_status);
/* The call that made the last capture attempt fall back to direct launches, with its error text ("" if none). */
const char* sptr_capture_error(const sptr_ctx* ctx);
/* Whether the context's side streams run beside its render stream on this device: ms[0] = two 200-us
 * one-wave spins on the render stream, ms[1] = one there and one on the shadow side stream, ms[2] = one
 * there and one on the k_sky side stream (device events).  ms[1], ms[2] near ms[0] / 2: the side
 * stream has a hardware queue of its own; near ms[0]: its launches serialise with the render stream's. */
int sptr_overlap_probe(sptr_ctx* ctx, double ms[3]);
/* Traversal width: 2 (the LBVH as built), 4 (collapsed to 64-B quantised BVH4 nodes), or 0 = automatic (the
 * default: 2 for scenes staged in LDS, 4 otherwise). */
int sptr_set_bvh_width(sptr_ctx* ctx, uint32_t width);

/* ---- scene / state (OptixBackend::build and setters) -------------------------------------------- */
int sptr_upload_scene(sptr_ctx* ctx, const sptr_scene* scene); /* builds the LBVH on the device */
int sptr_set_materials(sptr_ctx* ctx, const sptr_material* mats, uint32_t count);
int sptr_set_lights(sptr_ctx* ctx, const sptr_light* lights, uint32_t count);
int sptr_set_environment(sptr_ctx* ctx, const sptr_environment* env);
int sptr_scene_info(const sptr_ctx* ctx, uint32_t* num_prims, uint32_t* num_nodes, uint32_t* bvh_depth,
                    double* build_ms);
/* Device layout of the uploaded scene (DESIGN.md "Data layout in HBM"). lds_bytes = bytes staged into
 * LDS per block by the trace/shadow kernels, 0 when the scene is traversed from HBM/L2. */
typedef struct sptr_scene_layout {
  uint32_t num_tris, num_spheres, num_nodes, leaf_size, bvh_depth, lds_bytes;
  uint64_t node_bytes, tri_bytes, sphere_bytes, prim_ref_bytes;
  uint32_t bvh_width; /* num_nodes / node_bytes describe the traversed (BVH2 or BVH4) nodes */
  uint32_t num_prim_refs; /* primitive references the BVH is built over: num_tris + num_spheres, plus the
                             extra references of split triangles (sptr_set_split_refs) */
} sptr_scene_layout;
int sptr_scene_layout_info(const sptr_ctx* ctx, sptr_scene_layout* out);

/* ---- rendering ---------------------------------------------------------------------------------- */
/* Renders on the context's stream, or on `stream` (a hipStream_t) when not NULL.  Returns after the
 * work completes, with the stats of this call and of any SPTR_FRAME_ASYNC calls still uncollected;
 * with SPTR_FRAME_ASYNC it only enqueues (consecutive asynchronous calls must use one stream).
 * OptixBackend::render blocks three times per bounce (OptixBackend.cpp:1678-1789); asynchronous
 * calls let a caller queue frames, the tile copy and the multi-GPU gather back to back. */
int sptr_render(sptr_ctx* ctx, const sptr_frame* frame, void* stream, sptr_stats* stats);
/* Wait for the uncollected render calls and return their summed stats (zero when there are none). */
int sptr_collect_stats(sptr_ctx* ctx, sptr_stats* stats);
/* Full image RGB8 (width*height*3; only this shard's tiles are written) and the accumulation sums
 * (width*height*3 floats; divide by the frame count for the mean): linear radiance in wavefront
 * mode, tonemapped per-frame colours in PathTracer mode (what GLRenderer accumulates).  While the
 * denoiser is on (sptr_set_denoise), sptr_read_rgb8 and sptr_read_rgb8_lagged return the filtered image. */
int sptr_read_rgb8(sptr_ctx* ctx, uint8_t* rgb);
/* ABI 9, the interactive loop's readback with one frame of latency (GLRenderer::renderLoop calls render()
 * once per frame, src/GLRenderer.cpp:161-176): call it after an asynchronous render (SPTR_FRAME_ASYNC).  The
 * image of that call is snapshotted on the device (a device-to-device copy ordered after it); the snapshot
 * taken by the previous sptr_read_rgb8_lagged call, if it is of the same size, is copied into rgb on a
 * copy stream of its own — beside the render just enqueued — and waited for: *got = 1.  Otherwise rgb is
 * left alone and *got = 0 (the first frame, or a resize: read that frame with sptr_read_rgb8).  rgb is
 * page-locked (hipHostRegister) while the context uses it as a destination, so the copy is a DMA that
 * overlaps the next frame's kernels; it is unregistered when another buffer takes its place and by
 * sptr_destroy.  The render stream is not waited for: sptr_collect_stats collects the calls' counters. */
int sptr_read_rgb8_lagged(sptr_ctx* ctx, uint8_t* rgb, uint32_t* got);
int sptr_read_accum(sptr_ctx* ctx, float* accum);
/* Device view of this shard's resolved tiles: RGBA8, [local tile][32][32] uint32, for the
 * multi-GPU gather.  *bytes = local_tiles * 4096. */
int sptr_tiles_device(sptr_ctx* ctx, void** dptr, size_t* bytes);
/* Scatter gathered tile buffers (rank-major: rank r's local tiles at offset r*tiles_per_rank*4096
 * bytes) into an RGB8 device image width*height*3.  With stream == NULL it runs on the context's
 * stream and waits; on a caller's stream it only enqueues. */
int sptr_unpack_tiles(sptr_ctx* ctx, const void* gathered, int32_t shard_count, uint32_t tiles_per_rank,
                      int32_t width, int32_t height, void* rgb8_out, void* stream);

/* ---- first-hit AOVs and the edge-avoiding denoiser (symbols added within ABI 9: no existing struct or
 *      entry point changed, so SPTR_ABI_VERSION stays 9) ------------------------------------------------
 * The interactive loop renders 1 spp per call; these entry points give such a frame a filtered image and
 * give an external denoiser its feature buffers.  The filter is an a-trous wavelet filter steered by the
 * first hit's normal, depth and albedo and by the colour itself (DESIGN.md "Denoiser"): iteration i
 * (i = 0 .. iterations-1) takes a 5x5 B3-spline footprint with a step of 2^i pixels; the colour weight's
 * sigma fades as 1 / n with the accumulation's frame count n, so a converging image is left alone; pixels
 * whose camera ray leaves the scene (the environment) and pixels whose mean is not finite pass through.
 * Only + - x, correctly rounded division, max and compares: a float32 restatement in the same order is
 * bit-exact (tests/denoise_ref.py). */
typedef struct sptr_denoise_params {
  uint32_t iterations;        /* 0 = off (default); 1..5 */
  float sigma_color;          /* 0 -> 0.5  */
  float sigma_depth;          /* 0 -> 0.05 */
  float sigma_albedo;         /* 0 -> 0.2  */
  uint32_t normal_log2_power; /* 0 -> 6 (cos^64); at most 16 */
  uint32_t reserved[3];       /* 0 */
} sptr_denoise_params;
/* params == NULL or iterations == 0: off.  With the denoiser on, a denoise pass follows every wavefront
 * render call that resolves (not SPTR_FRAME_NO_RESOLVE), on the call's stream and outside any captured
 * launch graph, so it also follows SPTR_FRAME_ASYNC calls; it writes a second RGB8 device image, which
 * sptr_read_rgb8 and sptr_read_rgb8_lagged then return.  The accumulation, sptr_read_accum,
 * sptr_tiles_device and the stats are untouched, and with the denoiser off a render call issues exactly
 * the launches it issued before these entry points existed.  With the denoiser on, sptr_render returns
 * SPTR_ERR_INVALID for a call that is not SPTR_INTEGRATOR_WAVEFRONT or has shard_count > 1 (a shard's
 * interleaved tiles have no neighbours).  Changing the parameters does not restart the accumulation. */
int sptr_set_denoise(sptr_ctx* ctx, const sptr_denoise_params* params);
/* First-hit feature buffers of the last render call's camera and size (any integrator, denoiser on or
 * off), from one closest-hit query per pixel along the pixel-centre ray (no jitter, tnear 0):
 *   SPTR_AOV_ALBEDO: W*H*3 floats, materials[geom_material[geomID]].albedo;
 *   SPTR_AOV_NORMAL: W*H*3 floats, the normalised geometric normal, facing the camera (N.d <= 0);
 *   SPTR_AOV_DEPTH : W*H floats, the hit distance t;
 *   SPTR_AOV_ID    : W*H*2 uint32, (geomID, primID) as sptr_intersect reports them;
 *   SPTR_AOV_UV    : W*H*2 floats, the hit's barycentrics u, v exactly as sptr_query_rays defines them
 *                    (0, 0 on a sphere).  This plane is allocated and written only when it is asked for or
 *                    sptr_set_history_motion is on; cached buffers that lack it are computed again.
 * A miss gives albedo 0, normal 0, depth -1, ids 0xFFFFFFFF and uv 0.  The buffers are cached per camera, size
 * and scene state, as the cull mask is: a static camera pays for them once (sptr_denoise_info). */
enum { SPTR_AOV_ALBEDO = 0, SPTR_AOV_NORMAL = 1, SPTR_AOV_DEPTH = 2, SPTR_AOV_ID = 3, SPTR_AOV_UV = 4 };
int sptr_read_aov(sptr_ctx* ctx, int kind, void* out);
/* The filter's output before the resolve: W*H*3 linear radiance.  An error unless the last render call
 * ran the denoise pass. */
int sptr_read_denoised(sptr_ctx* ctx, float* rgb);
/* Waits for the last denoise pass: device time of its AOV launch (0 when the cached buffers were used)
 * and of its filter launches (mean, iterations, resolve), and the AOV passes computed so far.  Any
 * pointer may be NULL. */
int sptr_denoise_info(const sptr_ctx* ctx, double* ms_aov, double* ms_filter, uint32_t* aov_passes);

/* ---- temporal reprojection: the denoiser's history across camera moves (symbols added within ABI 9: no
 *      existing struct or entry point changed) --------------------------------------------------------
 * A caller restarts the accumulation (frame_begin 1) when the camera moves, so every frame of a camera move
 * is a fresh 1-spp image.  Two settings carry what earlier frames saw across such a restart (DESIGN.md
 * "Temporal reprojection"); with both at their defaults a render call issues exactly the launches it issued
 * before these entry points existed and returns the same bytes.
 *
 * Seed offset: a wavefront render call seeds its frames as if its accumulation index were frame_begin +
 * offset, so that restarted accumulations need not draw the same per-pixel random streams again.  The clear
 * of the accumulation (frame_begin == 1), the continuity check and the divisor still follow frame_begin.
 * sptr_render returns SPTR_ERR_INVALID when offset + frame_begin + spp - 1 overflows 32 bits, and for a
 * call of another integrator while the offset is not 0.  Default 0. */
int sptr_set_seed_offset(sptr_ctx* ctx, uint32_t offset);
/* History: while the denoiser is on, each denoise pass first integrates the accumulation's mean c_0 with
 * the image an earlier pass integrated (the carry), reprojected through the first hit's world position:
 * t_0 = (n c_0 + m h) / (n + m), where h and m <= max_history are the carry's colour and history length
 * under the four bilinear taps that show the same surface (same geomID, normal and depth weights of the
 * filter itself at least 0.5 together); when the carry's camera is not the call's, h is first clipped to
 * the mean -+ half a standard deviation of c_0 over the pixel's 3x3 neighbours on the same geometry, since
 * what a glossy surface shows belongs to the view.  The filter's colour sigma then fades with n + m per
 * pixel instead of n.  When a call with frame_begin == 1 runs a pass, the image the previous pass integrated becomes the
 * carry, with that pass's first-hit planes and camera; calls that continue the accumulation keep reading
 * the same carry.  The carry is dropped when the size changes, when the scene state changes (whatever
 * recomputes the first-hit planes of an unchanged camera: uploads, sptr_update_geometry unless
 * sptr_set_history_motion is on, the material, light and environment setters, ...) and by any call of
 * sptr_set_denoise_history.  Without a carry the
 * pass equals the pass without history bit for bit.  Costs about 56 bytes per pixel of device memory. */
typedef struct sptr_history_params {
  uint32_t max_history;   /* 0 = off (default); else the cap M on a pixel's history length, in frames; at most 1024 */
  uint32_t reserved[3];   /* 0 */
} sptr_history_params;
int sptr_set_denoise_history(sptr_ctx* ctx, const sptr_history_params* params);  /* NULL = off; any call drops the history held */
/* The last pass's integrated colour t_0 and history length m' (n + m; 0 where the filter passes the pixel
 * through): W*H*4 floats.  An error unless the last render call ran a pass with history on. */
int sptr_read_history(sptr_ctx* ctx, float* rgbm);
/* Waits for the last pass, as sptr_denoise_info: the pixels that took history (m > 0), the device time of
 * the reprojection launch, and whether the pass had a carry to read.  All 0 when the last render call ran
 * no pass with history on.  Any pointer may be NULL. */
int sptr_history_info(sptr_ctx* ctx, uint32_t* reprojected, double* ms_reproject, uint32_t* carried);

/* ---- motion vectors: the history survives geometry updates (symbols added within ABI 9: no existing
 *      struct or entry point changed) --------------------------------------------------------------------
 * With this setting on, sptr_update_geometry no longer drops the denoiser's history (DESIGN.md "Motion
 * vectors").  Before a refit overwrites them, the triangle records and spheres the last history pass saw
 * are copied device-to-device into a snapshot (48 B per triangle, 16 B per sphere; only if that pass ran on
 * the current geometry, so several updates between two passes keep the carry's geometry).  The next pass
 * whose carry saw that geometry carries each pixel's surface point there (a triangle hit through its
 * barycentrics, a sphere hit through its unit offset from the centre), projects that point into the carry's
 * camera, and uses its distance and the old geometry's normal there in the taps' weights; the history taken
 * is always clipped as after a camera move, since shadows and reflections belong to the scene state as they
 * belong to the view.  A carry whose geometry the snapshot does not hold is dropped.  Everything else that
 * changes the scene state (uploads, the material, light and environment setters, a size change) drops the
 * history as before.  Default 0: every call issues the launches it issued before this entry point existed
 * and returns the same bytes.  Any call drops the history held and the snapshot.  SPTR_ERR_INVALID on a
 * lane context. */
int sptr_set_history_motion(sptr_ctx* ctx, uint32_t on);
/* The motion vectors of the last pass that read its carry through a snapshot: W*H*2 floats, per pixel
 * (fx - x, fy - y), where (fx, fy) is the place of the pixel's surface point in the carry's image (pixel
 * centres at integers).  A quiet NaN twice for a pixel that never reaches the projection (a miss, a mean
 * that is not finite).  An error unless the last render call ran such a pass. */
int sptr_read_motion(sptr_ctx* ctx, float* out);
/* Snapshots taken since the upload, device ms of the last one, and whether the last pass read its carry
 * through a snapshot (0 / 1).  Any pointer may be NULL. */
int sptr_motion_info(sptr_ctx* ctx, uint32_t* snapshots, double* ms_snapshot, uint32_t* used);

/* ---- dynamic scenes: refit the BVH in place when geometry moves (symbols added within ABI 9: no
 *      existing struct or entry point changed) --------------------------------------------------------
 * A scene whose coordinates change but whose topology does not (an animated or edited mesh, moving
 * spheres) need not be uploaded again: sptr_update_geometry recomputes the triangle records, the spheres
 * and every box of the BVH2 and of the wide BVH in place, with the tree topology and the slot order of
 * the upload (DESIGN.md "Dynamic scenes").  No sort, tree construction, treelet or collapse pass runs.
 * The records and the quantised nodes come from the device functions the build itself calls, so a hit's t
 * and Ng equal those of a fresh upload of the moved scene bit for bit, and the original coordinates give
 * the original nodes back.  The tree's quality degrades as the geometry deforms away from the uploaded
 * one (the boxes stay tight, their overlap grows): upload again when traversal gets slow. */
/* 1: the next sptr_upload_scene keeps what a refit needs (the index triples in slot order, a box per
 * slot, the BVH2 nodes grouped by subtree height, per wide node the BVH2 boxes its children came from:
 * about 44 B per triangle + 4 B per BVH2 node + 16 B per wide node); the tree and every result are those
 * of an ordinary upload.  0 (default): uploads allocate, launch and keep exactly what they always did. */
int sptr_set_dynamic(sptr_ctx* ctx, uint32_t on);

enum { SPTR_UPDATE_DEVICE_PTRS = 1u };  /* positions / spheres are device pointers on ctx's device */
/* New coordinates for the uploaded topology: positions = num_verts*3 floats or NULL (unchanged),
 * spheres = num_spheres*4 floats or NULL (unchanged).  Counts must equal the upload's.  The indices, the
 * geometry order and the material map stay as uploaded.  Waits for pending renders, as the upload does,
 * and returns when the refit is complete (a pixel lane's copy of the scene included).  The state epoch is
 * bumped: the cull mask, the AOV cache and captured launch graphs are invalidated as after an upload.
 * Restarting the accumulation (frame_begin = 1) is the caller's job, as after an upload.
 * Triangles that were exactly degenerate (zero Ng) at upload were left out of the tree and stay out: their
 * records follow the new coordinates, but no ray can hit them until the scene is uploaded again.
 * SPTR_ERR_NO_SCENE before an upload; SPTR_ERR_INVALID when the scene was not uploaded with
 * sptr_set_dynamic(1), a count differs from the upload's, both pointers are NULL, or the scene was built
 * with split references (sptr_set_split_refs took effect: num_prim_refs > num_tris + num_spheres). */
int sptr_update_geometry(sptr_ctx* ctx, const float* positions, uint32_t num_verts,
                         const float* spheres, uint32_t num_spheres, uint32_t flags);
/* refits since the upload; wall ms of the last one (as build_ms is measured); device ms of its kernels;
 * triangles left out of the tree because they were exactly degenerate at upload. Any pointer may be NULL. */
int sptr_refit_info(const sptr_ctx* ctx, uint32_t* refits, double* ms_wall, double* ms_device,
                    uint32_t* excluded_prims);

/* ---- dynamic scenes: per-geometry transforms applied on the device (symbols added within ABI 9: no
 *      existing struct or entry point changed) --------------------------------------------------------
 * Rigid motion needs no new vertices: the caller hands over one matrix per triangle geometry, and the refit's
 * slot pass transforms a kept copy of the vertices, the rest pose, while it gathers them (DESIGN.md "Dynamic
 * scenes", transforms).  64 bytes per geometry cross the bus instead of 12 per vertex.
 *
 * Values of sptr_set_dynamic.  Any non-zero value keeps the refit tables, as before.  With the bit
 * SPTR_DYNAMIC_TRANSFORMS the next upload also keeps a device copy of the uploaded positions, the rest pose
 * (12 B per vertex), and records the cost of its tree (sptr_tree_cost) once, at its end.  Without that bit an
 * upload allocates, launches and keeps exactly what it did before these entry points existed. */
enum { SPTR_DYNAMIC_REFIT = 1u, SPTR_DYNAMIC_TRANSFORMS = 2u };
/* Replaces the rest pose: num_verts * 3 floats, num_verts equal to the upload's; flags takes
 * SPTR_UPDATE_DEVICE_PTRS.  Nothing visible changes until the next sptr_update_transforms.  A caller uploads the
 * world-space flattening, so that the tree is built over the scene as it looks, sets the object-space vertices as
 * the rest pose, and from then on sends the instances' matrices.  Without this call the matrices are relative to
 * the uploaded pose.  Errors as sptr_update_transforms. */
int sptr_set_rest_positions(sptr_ctx* ctx, const float* positions, uint32_t num_verts, uint32_t flags);
/* xforms = num_tri_geoms * 16 floats, one glm-layout mat4 per triangle geometry in geomID order: column-major,
 * m[col][row], as InstanceData::worldFromObject holds it; or NULL: the triangles keep their records.  spheres as
 * in sptr_update_geometry, or NULL; not both NULL.  A triangle of geometry g takes each of its three vertices as
 * glm's M_g * vec4(rest[v], 1) without its w: per component k, m0 = M[0][k] x, m1 = M[1][k] y, m2 = M[2][k] z,
 * m3 = M[3][k] 1.0f, result (m0 + m1) + (m2 + m3), in float32 without contraction: the bits the host layer's
 * flattening gives.  Row 3 of the matrix is ignored.  A vertex shared by triangles of two geometries is
 * transformed per triangle; no world-position buffer is written.  Each call determines the triangles from the
 * rest pose alone: transforms do not accumulate.  A later sptr_update_geometry(positions) sets world positions
 * as ever and leaves the rest pose alone.  Everything else is sptr_update_geometry's: it waits for pending
 * renders, refits on the context's stream and then the pixel lane's copy, bumps the state epoch, takes the
 * sptr_set_history_motion snapshot first under the same condition, and counts in sptr_refit_info.
 * SPTR_ERR_NO_SCENE before an upload; SPTR_ERR_INVALID when the scene was not uploaded with
 * SPTR_DYNAMIC_TRANSFORMS, a count differs from the upload's, both pointers are NULL, a flag is unknown, the
 * scene uses split references, the context is a lane context, or a host-pointer matrix has an entry that is
 * not finite.  Matrices given by device pointer (SPTR_UPDATE_DEVICE_PTRS) are not inspected: what a NaN or an
 * infinity in them does to the boxes is the caller's to avoid. */
int sptr_update_transforms(sptr_ctx* ctx, const float* xforms, uint32_t num_tri_geoms,
                           const float* spheres, uint32_t num_spheres, uint32_t flags);
/* When does an upload pay?  A refit keeps the upload's topology, and boxes that mix two objects grow as the
 * objects part.  cost = the sum, over the inner nodes of the BVH2 that a walk can reach and over both child
 * boxes b of each, of w * A(b), with A(b) = 2 (dx dy + dy dz + dz dx) computed in double from the float extents
 * and w = 1 for an inner child, the leaf range's primitive count for a leaf child; root_area = A of the union
 * of the root's two child boxes.  Both for the tree as it stands, and as the upload recorded them (0 when the
 * scene was not uploaded with SPTR_DYNAMIC_TRANSFORMS).  The cost is absolute, not divided by the root area:
 * a fixed set of camera rays has a fixed line density, and a root that grows because one object left would
 * make a relative figure improve.  Scenes walked as BVH4 report the BVH2 they were collapsed from (a refit
 * re-quantises their wide boxes from those boxes).  A scene of one leaf range has no inner node a walk reaches:
 * cost 0.  The sum has a fixed shape (per-thread sums in node order, a block tree, the blocks in order on the
 * host), so the same tree gives the same bits on every call.  Waits for pending renders; one launch.  Any
 * output pointer may be NULL.  SPTR_ERR_NO_SCENE before an upload. */
int sptr_tree_cost(sptr_ctx* ctx, double* cost, double* root_area, double* cost_at_upload, double* root_area_at_upload);

/* ---- ray queries on caller buffers (symbols added within ABI 9: no existing struct or entry point
 *      changed) ------------------------------------------------------------------------------------------
 * Batched closest-hit / any-hit queries against the uploaded (and possibly refitted) scene, for callers that
 * hold rays in device memory and want the answers there: AO or visibility baking, sensor simulation,
 * picking, feeding an external denoiser or a learning pipeline.  The rays are walked by the traversal the
 * render kernels use (scenes staged into LDS are staged, wide scenes take the BVH4 walk), so a ray's hit is
 * the renderer's hit; (geomID, primID) are resolved on the device (DESIGN.md "Ray queries").
 *
 * rays: n x 8 floats (o3, d3, tnear, tfar), as sptr_intersect.  Closest-hit outputs, reported exactly as
 * sptr_intersect reports them; each pointer may be NULL and is then not written:
 *   geom, prim: n uint32 each; a miss gives 0xFFFFFFFF twice; a sphere gives prim 0;
 *   t         : n floats; a miss gives +inf;
 *   ng        : n x 3 floats, the unnormalised geometric normal; a miss gives 0;
 *   uv        : n x 2 floats, the barycentrics of a triangle hit: u = U / |den|, v = V / |den| of the
 *               Moeller-Trumbore terms of the triangle finally hit (IEEE division, as for t), so that the hit
 *               point is (1 - u - v) v0 + u v1 + v v2 with v0, v1, v2 in the order of the uploaded index
 *               triple; a sphere hit (the reference's sphere callbacks set no u or v) and a miss give 0.
 * With SPTR_QUERY_ANY_HIT the only output is occluded (n bytes, 1 = something lies in (tnear, tfar)), as
 * sptr_occluded; the other output pointers are ignored.
 *
 * Pointers: with SPTR_QUERY_DEVICE_PTRS every pointer is a device pointer on the context's device, and the
 * ray buffer must be 16-byte aligned (SPTR_ERR_INVALID otherwise); without it every pointer is a host
 * pointer, the library stages the arrays, and the call is synchronous (a non-NULL stream is
 * SPTR_ERR_INVALID).
 * Streams: stream == NULL runs on the context's stream, after any pending renders, and returns when the
 * results are written.  A non-NULL stream (a hipStream_t, device pointers only) only enqueues, as
 * sptr_unpack_tiles does: consecutive enqueued queries must use one stream (they share the context's
 * scratch), and the caller synchronises that stream before any upload (sptr_upload_scene, sptr_set_*),
 * sptr_update_geometry or sptr_destroy: an enqueued query reads the scene in place.
 * Order: SPTR_QUERY_SORT traces the batch in the order of a per-ray key (a Morton code of the origin, then
 * the direction's octant and octahedral cell), sorted on the device by the build's radix sort; the results
 * are written at each ray's own index and do not depend on the order.  SPTR_QUERY_NO_SORT traces in
 * the caller's order.  With neither flag the library decides (at present it never sorts).
 * n == 0 returns SPTR_OK with no launch.  SPTR_ERR_INVALID: both sort flags, n > 2^28, NULL rays with n > 0,
 * SPTR_QUERY_ANY_HIT without occluded, unknown flags, a lane context; SPTR_ERR_NO_SCENE before an upload. */
enum { SPTR_QUERY_ANY_HIT = 1u, SPTR_QUERY_DEVICE_PTRS = 2u, SPTR_QUERY_SORT = 4u, SPTR_QUERY_NO_SORT = 8u };
typedef struct sptr_ray_query {
  const float* rays;   /* n x 8 floats: o3 d3 tnear tfar, as sptr_intersect */
  uint32_t n;          /* <= 2^28 */
  uint32_t flags;
  uint32_t* geom;      /* outputs; each may be NULL and is then not written */
  uint32_t* prim;
  float* t;            /* n */
  float* ng;           /* n x 3, unnormalised, as sptr_intersect */
  float* uv;           /* n x 2 barycentrics */
  uint8_t* occluded;   /* n; the only output of SPTR_QUERY_ANY_HIT */
  uint64_t reserved[4];/* 0 */
} sptr_ray_query;
int sptr_query_rays(sptr_ctx* ctx, const sptr_ray_query* query, void* stream);
/* Waits for the last query: the device times of its sort phase (keys and radix sort; 0 when it was traced
 * unsorted) and of its trace launch, whether it was sorted (0 / 1), and the queries launched so far (one
 * with n == 0 launches nothing and is not counted).  SPTR_ERR_HIP, with the text sptr_intersect gives, if the last query set the
 * traversal-stack-overflow flag (a synchronous query checks the flag itself).  Any pointer may be NULL. */
int sptr_query_info(sptr_ctx* ctx, double* ms_sort, double* ms_trace, uint32_t* sorted, uint32_t* queries);

/* ---- multi-hit ray queries (symbols added within ABI 9: no existing struct or entry point changed) ---------
 * The K = max_hits nearest hits along each ray, in order: lidar with several returns, the thickness of an
 * object (entry and exit), what lies behind a glass surface, how many surfaces a ray crosses, picking through
 * the front surface.  One walk per ray that keeps a list instead of a minimum (k_rayquery_multi).
 *
 * Candidate hits of ray i with interval (tnear, tfar), read as sptr_query_rays reads it, per primitive:
 *   triangle: at most one, what the closest-hit triangle test reports for that triangle on the ray's own
 *             interval (same arithmetic, same acceptance |den| tnear < T <= |den| tfar);
 *   sphere  : at most two.  The first is what the closest-hit sphere test reports on (tnear, tfar), at t_a;
 *             the second, if there is a first, is what the same test reports on (t_a, tfar) — a second
 *             evaluation with tnear = t_a, quirks included (the test's t > 0 rule; a tangent sphere with
 *             t1 == t2 gives one hit).  The first is reported with prim = 0, the second with prim = 1.
 *   A triangle left out of the tree because it was exactly degenerate at upload gives nothing; a triangle the
 *   tree references several times (sptr_set_split_refs) is one primitive and gives one hit.
 * Result: the first K candidates in ascending order of the key (t, geomID, primID), t compared as float and
 * the ids as unsigned, resolved exactly as sptr_query_rays reports them.  The order therefore depends on
 * nothing but the scene and the ray: not on the tree, the walk, the leaf size, the tree order, a refit or the
 * trace order.  count[i] = min(K, number of candidates).  Hit j of ray i is element i * K + j of every per-hit
 * array.  Slot j < count[i] holds geom, prim, t, the unnormalised Ng (the stored triangle normal, or
 * (P - c) / r with P = o + t d for a sphere) and uv (sptr_query_rays' barycentrics for a triangle, 0 for a
 * sphere).  Slots j >= count[i] are filled: ids 0xFFFFFFFF, t = +inf, Ng = 0, uv = 0.
 * With K = 1, t equals sptr_query_rays' closest-hit t bit for bit, and the ids equal its ids unless two
 * primitives tie exactly at that t.
 *
 * Pointers, streams, order and scratch: the rules of sptr_query_rays, word for word.  Host pointers are staged
 * and the call is synchronous; a non-NULL stream is for device pointers only and only enqueues; consecutive
 * enqueued queries (of either kind) must share one stream; n == 0 returns SPTR_OK with no launch; a
 * traversal-stack overflow is reported as sptr_query_rays reports it.
 * SPTR_ERR_INVALID: SPTR_QUERY_ANY_HIT or an unknown flag, both sort flags, max_hits outside
 * 1 .. SPTR_MULTI_HIT_MAX, n > 2^28 or n * max_hits > 2^28, NULL count or rays with n > 0, non-zero pad or
 * reserved, a misaligned device ray buffer, host pointers with a stream, a lane context.  SPTR_ERR_NO_SCENE
 * before an upload.  A refused call writes nothing and leaves the context as it was. */
enum { SPTR_MULTI_HIT_MAX = 16 };
typedef struct sptr_multi_hit_query {
  const float* rays;   /* n x 8 floats: o3 d3 tnear tfar; 16-byte aligned when a device pointer */
  uint32_t n;          /* <= 2^28, and n * max_hits <= 2^28 */
  uint32_t flags;      /* SPTR_QUERY_DEVICE_PTRS | SPTR_QUERY_SORT | SPTR_QUERY_NO_SORT */
  uint32_t max_hits;   /* K: 1 .. SPTR_MULTI_HIT_MAX */
  uint32_t pad;        /* 0 */
  uint32_t* count;     /* n; required */
  uint32_t* geom;      /* n*K; each of these may be NULL and is then not written */
  uint32_t* prim;
  float* t;
  float* ng;           /* n*K x 3 */
  float* uv;           /* n*K x 2 */
  uint64_t reserved[4];/* 0 */
} sptr_multi_hit_query;
int sptr_query_multi_hit(sptr_ctx* ctx, const sptr_multi_hit_query* query, void* stream);
/* Waits for the last multi-hit query: the device times of its sort phase and of its trace launch, whether it
 * was sorted, the multi-hit queries launched so far, and the list capacity (entries per ray) and LDS bytes per
 * block (static and dynamic) of the kernel instantiation it launched; zeros before the first.  SPTR_ERR_HIP if
 * it set the traversal-stack-overflow flag, as sptr_query_info.  Any pointer may be NULL. */
int sptr_multi_hit_info(sptr_ctx* ctx, double* ms_sort, double* ms_trace, uint32_t* sorted, uint32_t* queries,
                        uint32_t* list_capacity, uint32_t* lds_bytes);

/* ---- closest-point queries (symbols added within ABI 9: no existing struct or entry point changed) ---------
 * Which surface point is nearest to this point, and how far is it: distance fields, collision and contact,
 * snapping, registration, occupancy.  One walk per point, pruned by the distance to a node's box
 * (k_pointquery).  csrc/closest_point.h is the normative text; in words:
 *
 * Candidate of a primitive for point p:
 *   triangle: from the stored record (v0, e1 = v0 - v1, e2 = v2 - v0, in the uploaded index order), the nearest
 *             of four points in float32: the clamped projections of p onto the three edges, and the projection
 *             onto the face (an orthogonalised two-by-two solve) when its weights are inside the triangle.  Each
 *             is a convex combination q = (1 - u - v) v0 + u v1 + v v2 with clamped weights (sptr_query_rays'
 *             vertex convention), and its d2 is dot(p - q, p - q) of that q, never a plane distance.  A triangle
 *             left out of the tree because it is exactly degenerate (a stored normal of exactly zero) gives
 *             nothing; a triangle the tree references several times (sptr_set_split_refs) is one primitive.
 *   sphere  : a surface, as for rays: m = p - c, len = sqrt(m.m), d2 = (len - r)^2, q = c + m (r / len), or
 *             c + (r, 0, 0) when len == 0; ng = (q - c) / r per component (0 for a radius of 0); uv = 0.
 * Result of point i (p.xyz, max_dist): the candidate with the smallest key (d2, geomID, primID) among those
 * with d2 <= max_dist * max_dist (one float32 multiply), d2 compared as float and the ids as unsigned, resolved
 * as sptr_query_rays reports them (a sphere has prim 0).  max_dist = +inf accepts everything.  The result
 * depends on nothing but the scene and the point: not on the tree, its width, the leaf size, the tree order,
 * split references, a refit or the order of the walk.  Outputs: geom, prim, dist2 = d2, dist = sqrt(dist2)
 * (correctly rounded), point = q, uv = (u, v), ng (the stored unnormalised triangle normal, as
 * sptr_query_rays).  A miss — nothing within max_dist, max_dist negative or NaN, a coordinate of p that is
 * not finite (no walk for the last two) — gives ids 0xFFFFFFFF, dist2 = dist = +inf, point = uv = ng = 0.
 * Coordinates so large that their differences overflow float32 are outside the definition.
 *
 * Pointers, streams, order and scratch: the rules of sptr_query_rays, word for word.  Host pointers are staged
 * and the call is synchronous; a non-NULL stream is for device pointers only and only enqueues; consecutive
 * enqueued queries (of any kind) must share one stream; n == 0 returns SPTR_OK with no launch; a
 * traversal-stack overflow is reported as sptr_query_rays reports it.  SPTR_QUERY_SORT walks the batch in the
 * order of a 30-bit Morton code of p; with neither sort flag the library decides (at present it never sorts).
 * SPTR_POINT_COUNT makes the kernel count its node visits and primitive tests (sptr_point_query_info).
 * SPTR_ERR_INVALID: SPTR_QUERY_ANY_HIT or an unknown flag, both sort flags, n > 2^28, NULL points with n > 0,
 * non-zero reserved, a device point buffer not 16-byte aligned or a device output not 4-byte aligned, host
 * pointers with a stream, a lane context.  SPTR_ERR_NO_SCENE before an upload.  A refused call writes nothing
 * and leaves the context as it was. */
enum { SPTR_POINT_COUNT = 16u };            /* with SPTR_QUERY_DEVICE_PTRS | SPTR_QUERY_SORT | SPTR_QUERY_NO_SORT */
typedef struct sptr_point_query {
  const float* points;   /* n x 4 floats: p.xyz, max_dist; 16-byte aligned when a device pointer */
  uint32_t n;            /* <= 2^28 */
  uint32_t flags;
  uint32_t* geom;        /* outputs; each may be NULL and is then not written */
  uint32_t* prim;
  float* dist2;          /* n */
  float* dist;           /* n; sqrt(dist2), correctly rounded */
  float* point;          /* n x 3 */
  float* uv;             /* n x 2 */
  float* ng;             /* n x 3, unnormalised, as sptr_query_rays */
  uint64_t reserved[4];  /* 0 */
} sptr_point_query;
int sptr_query_points(sptr_ctx* ctx, const sptr_point_query* query, void* stream);
/* Waits for the last point query: the device times of its sort phase and of its walk, whether it was sorted,
 * the point queries launched so far, and the node visits and primitive tests of the last query if it set
 * SPTR_POINT_COUNT (0 otherwise); zeros before the first.  SPTR_ERR_HIP if it set the traversal-stack-overflow
 * flag, as sptr_query_info.  Any pointer may be NULL. */
int sptr_point_query_info(sptr_ctx* ctx, double* ms_sort, double* ms_walk, uint32_t* sorted, uint32_t* queries,
                          uint64_t* node_visits, uint64_t* prim_tests);
/* The host twin: the same definition by brute force over every primitive of `scene`, host pointers only, no
 * context and no device (flags must be 0 or sort flags, which are ignored).  The records are built with the
 * expressions the device uses.  It is the CPU fallback of HipBackend::queryPoints and the tests' yardstick. */
int sptr_host_query_points(const sptr_scene* scene, const sptr_point_query* query);

/* ---- signed distance queries (symbols added within ABI 9: no existing struct or entry point changed) -------
 * sptr_query_points with a sign: positive on the side the normals point to, negative on the other, decided by
 * the angle-weighted pseudonormal of the closest feature (Baerentzen & Aanaes).
 * csrc/pseudonormal.h is the normative text; in words:
 *
 * Tables.  A triangle is live if its stored Ng is not exactly zero; others take no part.  Its unit normal n is
 * Ng scaled by its largest absolute component and then normalised (contributes nothing if not finite).  Corners
 * of live triangles of one geometry whose positions compare equal as floats (-0 == +0, NaN equals nothing) are
 * one welded vertex; geometries never weld with each other.  N_v of a welded vertex: the float32 sum, in
 * ascending corner index 3t + k, of angle_c * n_t (the triangle's angle at that corner, pn_angle).  N_e of an
 * unordered pair of distinct welded vertices: the float32 sum, in ascending (t, k), of n_t over the live
 * triangles with that pair as edge k (edge 0 = v0v1, 1 = v0v2, 2 = v1v2).  An edge is open with exactly one
 * incidence and irregular unless it has exactly two that traverse it in opposite directions.
 *
 * Result of point i: the winner, dist and point q of sptr_query_points, unchanged.  feature says where q lies on
 * the winner: 0 face, 1 / 2 / 3 edge v0v1 / v0v2 / v1v2, 4 / 5 / 6 vertex v0 / v1 / v2, 7 a sphere, 0xFFFFFFFF a
 * miss.  normal = N: the stored Ng, N_e or N_v accordingly.  s = ((p-q).x N.x + (p-q).y N.y) + (p-q).z N.z;
 * signed_dist = -dist if s < 0, else +dist (0 and NaN count as positive); SPTR_SIGNED_FLIP_TRIANGLES negates the
 * sign of triangle results (for meshes whose stored normals point inward, such as the built-in cube and sphere
 * mesh).  A sphere: negative iff |p - c| < r, normal = ng; the flip flag does not apply.  A miss: +inf, 0.
 * The sign is relative to the geometry that owns the nearest surface point: for disjoint closed solids that is
 * the sign of their union; for intersecting solids it is not.  Open meshes and cracks between vertices that are
 * not bit-equal give the sign of the nearest feature's pseudonormal, whatever that means there.
 *
 * sptr_set_signed_distance(ctx, 1) makes the next sptr_upload_scene keep the triangles' corner positions and
 * build the tables on the device at its end; sptr_update_geometry and sptr_update_transforms rebuild them
 * (welding included) before they return.  Without it an upload allocates, launches and keeps what it did
 * before.  A scene with triangles but no triangle geometry builds no tables.
 *
 * sptr_query_signed_distance runs the point query of `q` (same kernels, same outputs) and one sign pass after
 * it on the same stream.  q.flags: those of sptr_query_points plus SPTR_SIGNED_FLIP_TRIANGLES.  Every rule of
 * sptr_query_points holds: pointers, streams, sorting, n == 0, refused calls, lane contexts, alignment (the
 * three new outputs are 4-byte aligned device pointers, each may be NULL).  SPTR_ERR_INVALID also when the scene
 * was uploaded without sptr_set_signed_distance(1). */
enum { SPTR_SIGNED_FLIP_TRIANGLES = 32u };
enum { SPTR_FEATURE_FACE = 0, SPTR_FEATURE_EDGE = 1, SPTR_FEATURE_VERTEX = 4, SPTR_FEATURE_SPHERE = 7 };
typedef struct sptr_signed_query {
  sptr_point_query q;
  float* signed_dist;    /* n */
  float* normal;         /* n x 3, N, unnormalised */
  uint32_t* feature;     /* n */
  uint64_t reserved[4];  /* 0 */
} sptr_signed_query;
typedef struct sptr_signed_info_t {
  uint64_t welded_vertices, edges, open_edges, irregular_edges;
  uint64_t table_bytes;  /* N_v and N_e per triangle corner and edge (72 B per triangle) and the kept corners (36 B) */
  uint32_t builds;       /* since the context was created */
  uint32_t valid;        /* the current scene has tables */
  uint32_t num_tris;     /* triangles the tables cover (0 without tables) */
  uint32_t pad;
  double ms_build;       /* device ms of the last build */
  double ms_sign;        /* device ms of the last sign pass (waits for it) */
} sptr_signed_info_t;
int sptr_set_signed_distance(sptr_ctx* ctx, uint32_t on);
int sptr_query_signed_distance(sptr_ctx* ctx, const sptr_signed_query* query, void* stream);
int sptr_signed_info(sptr_ctx* ctx, sptr_signed_info_t* out);
/* N_v and N_e per uploaded triangle, num_tris x 3 x 3 floats each (corner k, edge k; 0 for a triangle that is not
 * live), to host memory.  Either pointer may be NULL. */
int sptr_read_pseudonormals(sptr_ctx* ctx, float* nv, float* ne);
/* The host twins: the same tables with a stable sort and the same sums in the same order, and the query by
 * brute force (sptr_host_query_points, then the sign); csrc/pseudonormal.h on both sides, so the device's bits.
 * counts: welded vertices, edges, open edges, irregular edges; any pointer may be NULL. */
int sptr_host_pseudonormals(const sptr_scene* scene, float* nv, float* ne, uint64_t counts[4]);
int sptr_host_query_signed_distance(const sptr_scene* scene, const sptr_signed_query* query);

/* ---- path-traced radiance for caller-supplied rays (symbols added within ABI 9: no existing struct or
 *      entry point changed) ------------------------------------------------------------------------------
 * sptr_render renders through the reference's pinhole camera and sptr_query_rays answers what a ray hits; this
 * entry point takes arbitrary rays and returns what the wavefront integrator sees along them: fisheye,
 * equirectangular, orthographic and stereo cameras, irradiance and reflection probes, lightmap texels, sensor
 * models.  It is not a second integrator: a producer writes the rays into the integrator's ray stream, the
 * chain of trace / shade / shadow stages (and the path-per-thread tail) runs from depth 0 through the
 * instantiations that bounces >= 1 use, and a consumer sums the paths' radiance (DESIGN.md "Ray rendering").
 * A ray given the origin, direction and rng state of a camera path returns that path's radiance bit for bit.
 *
 * rays: n x 8 floats as sptr_query_rays (o3, d3, and two words that are ignored): the first segment is traced as
 * a camera ray, tnear 0 and no tfar.  The direction is used as given and must be of unit length; with
 * SPTR_RAYS_NORMALIZE the library first applies the shading's safe_normalize (v / sqrt(v.v), both correctly
 * rounded; 0 for a zero vector) — a unit vector is not a fixed point of that function in float32, hence the flag.
 * Rng state of sample s (0 <= s < samples) of ray i: seeds[i] when seeds is not NULL and samples == 1; otherwise
 * wang_hash((b ^ (frame_index + s)) ^ 1) with b = seeds ? seeds[i] : i — the state the wavefront raygen gives
 * pixel seed b in frame frame_index + s, so ray i of a batch without seeds draws what pixel i of that frame
 * draws (sptr_primary_rays returns those states).
 * radiance: n x 3 floats, L_i = +0 + L(i, 0) + L(i, 1) + ... in sample order, one add each (the adds the
 * accumulation of sptr_render makes; divide by samples for the mean).  Stored, or with SPTR_RAYS_ACCUMULATE
 * radiance[i] = radiance[i] + L_i, one add per component.
 * The scene, materials, lights, environment, debug mode and refits are followed as a render call follows them;
 * the semantics are SPTR_INTEGRATOR_WAVEFRONT's.  The image of a render call, its accumulation, its stats, a
 * captured launch graph, the AOV cache and the denoiser's history are left as they were.
 *
 * Pointers: with SPTR_RAYS_DEVICE_PTRS every pointer is a device pointer on the context's device, and the ray
 * buffer must be 16-byte aligned (SPTR_ERR_INVALID otherwise); without it every pointer is a host pointer, the
 * library stages the arrays, and the call is synchronous (a non-NULL stream is SPTR_ERR_INVALID).
 * Streams: the work always runs on the context's stream, since it uses the context's wave buffers, which render
 * calls use too; a batch runs in chunks of whole rays that fit the capacity those buffers have
 * (sptr_set_wave_paths lowers it).  stream == NULL: the work follows the pending renders, and the call returns
 * when the output is written.  A non-NULL stream (a hipStream_t, device pointers only): the context's stream
 * waits for an event recorded on that stream, and that stream waits for the completion event; no host wait
 * happens, and the buffers must stay alive until that stream has passed the event.  Render calls that follow
 * use the context's stream or that one, and the caller synchronises it before any upload, as for queries.
 * n == 0 returns SPTR_OK with no launch.  SPTR_ERR_INVALID: NULL rays or radiance with n > 0, samples == 0,
 * max_depth == 0 (or above 32, as for sptr_render), frame_index == 0, frame_index + samples - 1 above 2^32 - 1,
 * unknown flags, non-zero reserved words, n > 2^28, n * samples > 2^29, a lane context; SPTR_ERR_NO_SCENE before
 * an upload or before materials are set. */
enum { SPTR_RAYS_DEVICE_PTRS = 1u, SPTR_RAYS_ACCUMULATE = 2u, SPTR_RAYS_NORMALIZE = 4u };
typedef struct sptr_ray_render {
  const float* rays;      /* n x 8 floats as sptr_query_rays: o.xyz, d.xyz, and two words that are ignored */
  const uint32_t* seeds;  /* n, or NULL */
  uint32_t n;             /* <= 2^28 */
  uint32_t samples;       /* paths per ray in this call, >= 1; n * samples <= 2^29 */
  uint32_t frame_index;   /* accumulation index of sample 0 (a frame's frame_begin), >= 1 */
  uint32_t max_depth;     /* as sptr_frame.max_depth */
  uint32_t flags;
  float* radiance;        /* n x 3 floats */
  uint32_t reserved[4];   /* 0 */
} sptr_ray_render;
int sptr_render_rays(sptr_ctx* ctx, const sptr_ray_render* batch, void* stream);
/* Waits for the last call's end event: its device time, its closest-hit and any-hit query counts (as
 * sptr_stats counts them; they are not added to any render call's stats) and the chunks it ran in.  All 0
 * before the first call; a call with n == 0 leaves the previous call's values.  SPTR_ERR_HIP if the call set the
 * traversal-stack or stream-overflow flag (a synchronous call checks them itself).  Any pointer may be NULL. */
int sptr_ray_render_info(sptr_ctx* ctx, double* ms, uint64_t* closest, uint64_t* shadow, uint32_t* chunks);

/* ---- adaptive sampling (symbols added within ABI 9: no existing struct or entry point changed) ------------
 * sptr_render takes spp samples at every pixel; this entry point keeps sampling only the pixels that have not
 * converged.  It is not a second integrator: a selection compacts the unconverged ("active") local pixels into
 * a list, a producer writes their next camera rays into the integrator's ray stream, the chain sptr_render_rays
 * uses runs them from depth 0, and a consumer folds the radiance into the per-pixel state.
 *
 * State per local pixel: S, the RGB sum of all its samples (the context's accumulation buffer: sptr_read_accum
 * returns it); E, the RGB sum of its samples with an even index; n, the samples taken (sptr_read_sample_counts).
 * Sample i (1-based) of a pixel is the sample frame i of sptr_render takes there (with sptr_set_seed_offset's
 * offset as a render call applies it); S = S + L_i is one add per component in index order from +0, E likewise
 * for even i.
 * Error of a pixel, in float32, every operation correctly rounded and none contracted:
 *   nf = float(n), hf = float(n / 2); I = S / nf, A = E / hf (per component);
 *   err = ((|I.r - A.r| + |I.g - A.g|) + |I.b - A.b|) / sqrt(max((I.r + I.g) + I.b, 1e-4f))
 * A pixel is active iff n < max_samples && !(n >= min_samples && err < threshold); a NaN err keeps it active.
 * Passes: every active pixel with n == 0 takes min_samples samples, any other min(step, max_samples - n); then
 * the selection runs again, until no pixel is active.  The selection is a pure function of the state and the
 * parameters, so a call with max 16 continued with max 32 equals one call with max 32, and with threshold 0 the
 * result is sptr_render's accumulation of max_samples frames, bit for bit.
 *
 * frame: width, height, camera, max_depth, shard_rank and shard_count as sptr_render reads them; frame_begin
 * must be 1, spp is ignored, the integrator must be SPTR_INTEGRATOR_WAVEFRONT, and the only flag accepted is
 * SPTR_FRAME_NO_RESOLVE.  Without it the call ends with a resolve of every pixel by its own n into the tiles
 * and the RGB8 image (sptr_read_rgb8, sptr_tiles_device and a multi-GPU gather work as after sptr_render).
 * Without SPTR_ADAPTIVE_CONTINUE the call starts a new accumulation (S = E = 0, n = 0); with it the call goes
 * on from the state the context's last adaptive call left, under the new parameters: the size, camera, depth,
 * shard and state epoch (scene, materials, lights, environment, settings) must be unchanged and no render call
 * may have run in between, else SPTR_ERR_INVALID.
 * The call is synchronous: after each selection the host reads the selection's result words (the list length
 * among them) to size the next pass, and it returns when the image is written.  It follows the scene,
 * materials, lights, environment, debug mode and refits as a render call does; its rays are counted in info
 * only, never in a later call's sptr_stats.  Afterwards a sptr_render with frame_begin != 1 is SPTR_ERR_INVALID
 * (the accumulation holds unequal counts), one with frame_begin == 1 behaves as ever.
 * SPTR_ERR_INVALID: the denoiser is on, a lane context, a parameter outside its bounds, an unknown flag, a
 * non-zero reserved word, frame parameters sptr_render would reject; SPTR_ERR_NO_SCENE as for sptr_render;
 * SPTR_ERR_HIP if a launch set the traversal-stack or stream-overflow flag or a guard word of the state was
 * overwritten (internal errors). */
enum { SPTR_ADAPTIVE_CONTINUE = 1u };
typedef struct sptr_adaptive_params {
  float threshold;       /* >= 0, finite */
  uint32_t min_samples;  /* >= 2 */
  uint32_t max_samples;  /* >= min_samples, <= 65536 */
  uint32_t step;         /* >= 1 */
  uint32_t flags;
  uint32_t reserved[3];  /* 0 */
} sptr_adaptive_params;
typedef struct sptr_adaptive_info {
  uint64_t samples;          /* taken by this call = sum of the increase of n */
  uint64_t rays_closest, rays_shadow;
  uint32_t passes, chunks;
  uint32_t active_first, active_last;   /* list lengths of the first and last pass */
  uint32_t min_count, max_count;        /* over valid local pixels, after the call */
  double ms;                            /* device time, first launch to last */
  uint32_t reserved[4];
} sptr_adaptive_info;
/* info may be NULL. */
int sptr_render_adaptive(sptr_ctx* ctx, const sptr_frame* frame, const sptr_adaptive_params* params,
                         sptr_adaptive_info* info);
/* counts: width * height words of the last adaptive call's image, row-major; pixels of other shards 0.
 * SPTR_ERR_INVALID when the context holds no adaptive state. */
int sptr_read_sample_counts(sptr_ctx* ctx, uint32_t* counts);

/* ---- query entry points (tests / tooling) -------------------------------------------------------- */
/* Closest-hit / any-hit queries on the device BVH: rays = n*8 floats (o3, d3, tnear, tfar).
 * Outputs as rtcIntersect1 reports them: geomID (0xFFFFFFFF on miss), primID, t, unnormalised Ng. */
int sptr_intersect(sptr_ctx* ctx, const float* rays, uint32_t n, uint32_t* geom, uint32_t* prim, float* t,
                   float* ng);
int sptr_occluded(sptr_ctx* ctx, const float* rays, uint32_t n, uint8_t* occluded);
/* Primary rays of the wavefront raygen for a W x H image at accumulation index acc: directions
 * (W*H*3) and initial path RNG states (W*H), computed by the device kernel. */
int sptr_primary_rays(sptr_ctx* ctx, const sptr_camera* cam, int32_t width, int32_t height, uint32_t acc,
                      float* dirs, uint32_t* rng);
/* The LBVH build's device primitives (kernels_sort.hip), exposed for their own tests; they replace
 * the rocPRIM calls Embree's replacement would otherwise make (EmbreeBackend.cpp:82-181 builds on the
 * CPU).  Host arrays in and out, n entries each; every call allocates device scratch and waits.
 *   sptr_sort_pairs_u64: stable ascending LSD radix sort of (keys, vals) (equal keys keep their order);
 *   sptr_scan_u32: exclusive prefix sum of 32-bit counts (mod 2^32); out may equal in. */
int sptr_sort_pairs_u64(sptr_ctx* ctx, const uint64_t* keys, const uint32_t* vals, uint32_t n, uint64_t* keys_out,
                        uint32_t* vals_out);
int sptr_scan_u32(sptr_ctx* ctx, const uint32_t* in, uint32_t n, uint32_t* out);
/* The device's values of the wavefront path's two library calls, for the parity residue classifier:
 * fn SPTR_MATH_COSINE_SINCOS: (sinf, cosf) of the cosine sample's phi = 2 pi r1 for every
 *   r1 = k / 2^24 (wf_math.h:51-72), out = 2^25 floats, pairs by k; x and n are ignored;
 * fn SPTR_MATH_GAMMA: powf(x[i], 1/2.2) as the resolve computes it (GLRenderer.cpp:416-430), n values. */
enum { SPTR_MATH_COSINE_SINCOS = 0, SPTR_MATH_GAMMA = 1 };
int sptr_eval_math(sptr_ctx* ctx, int fn, const float* x, uint32_t n, float* out);

/* ---- host-side scene layer (the C++ SceneDesc / Camera / MaterialManager / LightManager mirror) ---- */
typedef struct sptr_host_scene sptr_host_scene;
/* name: "default", "default_emitter", "sphere_mesh" (p0 = stacks, p1 = slices), "test_triangle",
 * or "gltf:<path>" (p0 = material id for the mesh). */
int sptr_host_builtin_scene(const char* name, uint32_t p0, uint32_t p1, sptr_host_scene** out);
int sptr_host_scene_view(const sptr_host_scene* s, sptr_scene* view);
void sptr_host_scene_free(sptr_host_scene* s);
int sptr_host_camera_lookat(const float pos[3], const float target[3], float fov_deg, float aspect,
                            sptr_camera* out);
/* MaterialManager::setupDefaultMaterials presets; with_light appends Materials::Light() as index 9. */
int sptr_host_preset_materials(int with_light, sptr_material* out, int capacity);
/* setupLights in src/main.cpp:85-94: one directional sun. */
int sptr_host_default_lights(sptr_light* out, int capacity);
/* Cubemap::loadEquirectangular: RGB float equirect (w x h) -> 6 faces of size x size. */
int sptr_host_equirect_to_faces(const float* rgb, int32_t w, int32_t h, int32_t size, float* faces);
/* Host twins of the device tile packing (interleaved 32x32 tiles, shard R of G; see sptr_render):
 * pack this shard's pixels of an RGB8 image into RGBA8 tile-packed words, and scatter gathered
 * rank-major tile buffers back into an RGB8 image. */
int sptr_host_pack_tiles(const uint8_t* rgb, int32_t width, int32_t height, int32_t shard_count, int32_t shard_rank,
                         uint32_t* tiles);
int sptr_host_unpack_tiles(const uint32_t* gathered, int32_t shard_count, uint32_t tiles_per_rank, int32_t width,
                           int32_t height, uint8_t* rgb);
/* Radiance .hdr reader (RGBE, RLE) -> RGB float; caller frees with sptr_host_free. */
int sptr_host_load_hdr(const char* path, float** rgb, int32_t* w, int32_t* h);
void sptr_host_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* SPTR_HIP_H */
