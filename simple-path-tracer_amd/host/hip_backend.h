// hip_backend.h — backends::HipBackend, the MI355X drop-in for the reference's GPU backend slot.
// Public surface = backends::OptixBackend (include/backends/OptixBackend.h:39-71): build(SceneDesc),
// render(rgb, w, h, Camera), setEnvironment / setMaterialManager / setLightManager (non-owning;
// the pointees must outlive rendering), destroy(), setDebugMode().  Progressive accumulation is
// owned by the backend and restarts on resize or camera change, as OptixBackend::render does
// (src/backends/OptixBackend.cpp:1518-1542).  Extras: setSettings, renderLinear, stats.
// Errors: build() returns false; render() logs and leaves the buffer untouched (no exit()).
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "scene_desc.h"
#include "shading.h"

namespace backends {

class HipBackend {
 public:
  struct Settings {
    uint32_t spp_per_call = 1;  // progressive frames per render() call (GLRenderer renders 1)
    uint32_t max_depth = 6;     // PathTracer::Settings::max_depth used by the wavefront tile task
    // SPTR_INTEGRATOR_WAVEFRONT (the 'T' key's wavefront CPU semantics, default) or
    // SPTR_INTEGRATOR_PATHTRACER (the default key's PathTracer semantics, src/GLRenderer.cpp:172-176)
    uint32_t integrator = SPTR_INTEGRATOR_WAVEFRONT;
    uint32_t samples_per_frame = 4;  // PathTracer::Settings::samples_per_pixel (src/main.cpp:107)
    // sptr_set_launch_mode: 0 = replay a captured graph for repeated call shapes (default), 1 = direct
    // launches, 2 = direct on one stream, 3 = a graph for every repeated shape
    uint32_t launch_mode = 0;
    // sptr_set_pixel_lanes: 0 = two concurrent launch chains for calls of >= 2^24 samples on scenes
    // staged in LDS (default), 1 = one chain, 2 = two chains; a change restarts the accumulation
    uint32_t pixel_lanes = 0;
    // render() returns the previous call's image (one frame of latency) so that the read back of one frame
    // runs beside the next frame's kernels (sptr_read_rgb8_lagged); the first frame after a reset or a
    // resize is read synchronously.  The pixel buffer stays page-locked while render() writes into it.
    // Counters (stats()) are collected every kLaggedCollect calls and by flushStats().
    bool lagged_readback = false;
    // sptr_set_denoise: iterations 0 = off (default); 1..5 = every render() returns the frame filtered by
    // the edge-avoiding a-trous denoiser (wavefront integrator only; with lagged_readback, the denoised
    // previous frame).  Zero sigmas / power take the defaults.  A change does not restart the accumulation.
    sptr_denoise_params denoise{};
    // sptr_set_denoise_history: max_history 0 = off (default); else, while the denoiser is on, its passes carry
    // the integrated image across the restarts a camera move causes (kDefaultMaxHistory is the cap to ask for
    // without a number of one's own), and each restart advances the seed offset (sptr_set_seed_offset) by the
    // frames of the accumulation it ends, so that consecutive restarts draw fresh samples
    sptr_history_params history{};
    // sptr_set_history_motion, applied with the history settings: update() keeps the history, which the next
    // pass reads through a snapshot of the geometry it saw (motion vectors)
    bool motion = false;
    // sptr_set_dynamic, applied before build(): the build keeps what update() needs to refit the BVH in
    // place when only coordinates change
    bool dynamic = false;
    // sptr_set_dynamic's SPTR_DYNAMIC_TRANSFORMS bit (implies dynamic), applied before build(): the build also
    // sets the meshes' object-space vertices as the device's rest pose, and update() sends only the instances'
    // matrices (and the spheres) when nothing else changed
    bool transforms = false;
    // sptr_set_signed_distance, applied before build(): the build keeps the triangles' corners and builds the
    // pseudonormal tables querySignedDistance() needs; update() rebuilds them
    bool signed_distance = false;
  };
  static constexpr uint32_t kLaggedCollect = 32;
  static constexpr uint32_t kDefaultMaxHistory = 4;  // lowest last-frame RMSE of the caps tried

  explicit HipBackend(int device = 0);
  ~HipBackend();
  HipBackend(const HipBackend&) = delete;
  HipBackend& operator=(const HipBackend&) = delete;

  bool build(const scene::SceneDesc& sceneDesc);
  // The scene after a change: flattens as build() does; when the counts, the indices, the geometry order
  // and the material map equal the built scene's (and Settings::dynamic was set for that build), the new
  // coordinates are refitted in place (sptr_update_geometry), otherwise the scene is built again.  Either
  // way the accumulation restarts.  With Settings::transforms, when in addition every mesh's vertices equal
  // the built scene's (only worldFromObject or the spheres differ), the instances' matrices are sent instead of
  // the vertices (sptr_update_transforms): 64 bytes per instance.
  bool update(const scene::SceneDesc& sceneDesc);
  // sptr_tree_cost: the BVH2's cost and root area now and as the last build recorded them (0 without
  // Settings::transforms); compare the first pair with the second to decide when build() would pay
  bool treeCost(double* cost, double* root_area, double* cost_at_build, double* root_area_at_build) const {
    return ctx_ && sptr_tree_cost(ctx_, cost, root_area, cost_at_build, root_area_at_build) == SPTR_OK;
  }
  // whether the last update() went through sptr_update_transforms
  bool lastUpdateSentTransforms() const { return sent_transforms_; }
  // sptr_refit_info: refits since the last build, wall / device ms of the last one, excluded primitives
  bool refitInfo(uint32_t* refits, double* ms_wall, double* ms_device, uint32_t* excluded_prims) const {
    return ctx_ && sptr_refit_info(ctx_, refits, ms_wall, ms_device, excluded_prims) == SPTR_OK;
  }
  // sptr_scene_info's build_ms of the last build
  double buildMs() const {
    double ms = 0.0;
    return ctx_ && sptr_scene_info(ctx_, nullptr, nullptr, nullptr, &ms) == SPTR_OK ? ms : 0.0;
  }
  void render(unsigned char* pixels, int width, int height, const Camera& camera);
  void setEnvironment(const EnvironmentManager* env) { env_ = env; env_dirty_ = true; }
  void setMaterialManager(const MaterialManager* mm) { mm_ = mm; mats_dirty_ = true; }
  void setLightManager(const LightManager* lm) { lm_ = lm; lights_dirty_ = true; }
  void destroy();
  void setDebugMode(int mode);

  void setSettings(const Settings& s) { settings_ = s; }
  const Settings& getSettings() const { return settings_; }
  // linear accumulated radiance mean (width*height*3) of the current accumulation
  bool renderLinear(float* rgb32, int width, int height, const Camera& camera);
  const sptr_stats& stats() const { return stats_; }
  // the counters of every render() since the last flush, summed (waits for the pending frames)
  sptr_stats flushStats();
  // sptr_denoise_info of the last render(): device ms of its AOV launch (0: cached) and filter launches
  // (waits for that pass), and the AOV passes computed so far
  bool denoiseInfo(double* ms_aov, double* ms_filter, uint32_t* aov_passes) const {
    return ctx_ && sptr_denoise_info(ctx_, ms_aov, ms_filter, aov_passes) == SPTR_OK;
  }
  // sptr_history_info of the last render(): pixels that took history, device ms of the reprojection launch
  // (waits for that pass), whether the pass had a carry
  bool historyInfo(uint32_t* reprojected, double* ms_reproject, uint32_t* carried) const {
    return ctx_ && sptr_history_info(ctx_, reprojected, ms_reproject, carried) == SPTR_OK;
  }
  // sptr_motion_info: snapshots since the last build, device ms of the last one, whether the last render()'s
  // pass took the motion path
  bool motionInfo(uint32_t* snapshots, double* ms_snapshot, uint32_t* used) const {
    return ctx_ && sptr_motion_info(ctx_, snapshots, ms_snapshot, used) == SPTR_OK;
  }
  // sptr_query_rays with host pointers: n rays of 8 floats (o3, d3, tnear, tfar) against the built scene,
  // traced by the renderer's traversal.  Closest hit fills geom, prim, t, ng (n x 3) and uv (n x 2) as
  // include/sptr_hip.h describes them (a miss: geom = prim = 0xFFFFFFFF, t = +inf); anyHit fills occluded.
  struct HitBuffers {
    std::vector<uint32_t> geom, prim;
    std::vector<float> t, ng, uv;
    std::vector<uint8_t> occluded;
  };
  bool queryRays(const float* rays, uint32_t n, bool anyHit, HitBuffers& out);
  // sptr_query_multi_hit with host pointers: per ray the maxHits nearest hits in ascending (t, geomID, primID).
  // count has n entries; hit j of ray i is element i * maxHits + j of geom, prim, t, ng (x 3) and uv (x 2), the
  // slots beyond a ray's count filled as include/sptr_hip.h describes.
  struct MultiHitBuffers {
    std::vector<uint32_t> count, geom, prim;
    std::vector<float> t, ng, uv;
  };
  bool queryMultiHit(const float* rays, uint32_t n, uint32_t maxHits, MultiHitBuffers& out);
  // sptr_query_points with host pointers: per point (n x 4 floats: p.xyz, max_dist) the nearest surface point
  // within max_dist, as include/sptr_hip.h defines it; point and ng hold 3 floats per point, uv 2.  Without a
  // device, sptr_host_query_points answers the same question over a flat scene.
  struct PointBuffers {
    std::vector<uint32_t> geom, prim;
    std::vector<float> dist2, dist, point, uv, ng;
  };
  bool queryPoints(const float* points, uint32_t n, PointBuffers& out);
  // sptr_query_signed_distance with host pointers (Settings::signed_distance at build()): queryPoints' outputs and,
  // per point, the signed distance (positive on the side the normals point to; flipTriangles negates triangle
  // results, for meshes wound like the built-in ones), the pseudonormal N (x 3) and the feature code.  counts: the
  // tables' welded vertices, edges, open and irregular edges.  Without a device, sptr_host_query_signed_distance
  // answers the same question over a flat scene.
  struct SignedBuffers {
    PointBuffers points;
    std::vector<float> signed_dist, normal;
    std::vector<uint32_t> feature;
    uint64_t counts[4] = {0, 0, 0, 0};
  };
  bool querySignedDistance(const float* points, uint32_t n, bool flipTriangles, SignedBuffers& out);
  // sptr_render_rays with host pointers: the wavefront integrator's radiance along n caller-supplied rays of 8
  // floats (o3, unit d3, two ignored words) against the built scene and the current materials, lights and
  // environment, Settings::max_depth bounces deep.  radiance (n x 3) takes, per ray, the sum of `samples` paths
  // seeded as include/sptr_hip.h describes (seeds: n words or null), or has it added with `accumulate`;
  // `normalize` applies the shading's safe_normalize to the directions first.  The image, the accumulation and
  // the stats of render() are left alone.  info (may be null): sptr_ray_render_info of the call.
  struct RayRenderInfo {
    double ms = 0.0;
    uint64_t closest = 0, shadow = 0;
    uint32_t chunks = 0;
  };
  bool renderRays(const float* rays, const uint32_t* seeds, uint32_t n, uint32_t samples, uint32_t frame_index,
                  float* radiance, bool accumulate = false, bool normalize = false, RayRenderInfo* info = nullptr);
  // sptr_render_adaptive: a new accumulation of the wavefront integrator that keeps sampling only the pixels whose
  // half-buffer error is not yet below `threshold` (at least min_samples, at most max_samples per pixel, `step`
  // more per pass; include/sptr_hip.h states the rule), Settings::max_depth bounces deep, with the current
  // materials, lights and environment.  rgb (width * height * 3, may be null) takes the image, every pixel
  // resolved by its own count; counts (width * height, may be null) the samples per pixel.  The next render()
  // starts a new accumulation.
  struct AdaptiveSettings {
    float threshold = 0.02f;
    uint32_t min_samples = 16, max_samples = 64, step = 16;
  };
  using AdaptiveInfo = sptr_adaptive_info;
  bool renderAdaptive(uint8_t* rgb, int width, int height, const Camera& camera, const AdaptiveSettings& as,
                      AdaptiveInfo* info = nullptr, uint32_t* counts = nullptr);
  uint32_t frameIndex() const { return frame_index_; }
  const std::string& lastError() const { return err_; }
  const std::vector<uint32_t>& getGeomMaterialMapping() const { return geom_material_; }

 private:
  bool ensureContext();
  bool buildFlat(const scene::FlatScene& flat);
  bool buildScene(const scene::SceneDesc& sd, const scene::FlatScene& flat);
  bool syncState();
  bool renderInternal(int width, int height, const Camera& camera, bool async = false);
  void addStats(const sptr_stats& s);

  int device_;
  sptr_ctx* ctx_ = nullptr;
  const EnvironmentManager* env_ = nullptr;
  const MaterialManager* mm_ = nullptr;
  const LightManager* lm_ = nullptr;
  bool env_dirty_ = true, mats_dirty_ = true, lights_dirty_ = true, built_ = false;
  Settings settings_;
  sptr_stats stats_{};
  uint32_t frame_index_ = 0;
  int last_w_ = 0, last_h_ = 0;
  bool has_last_camera_ = false;
  std::array<float, 9> last_cam_{};
  std::vector<uint32_t> geom_material_;
  // the built scene's topology (update() compares against it) and whether it was built dynamic
  std::vector<uint32_t> built_indices_, built_geom_first_;
  size_t built_verts_ = 0, built_spheres_ = 0;
  bool built_dynamic_ = false;
  // the rest pose the device holds (the built scene's object-space vertices in the flattening's order); empty:
  // none, update() sends vertices
  std::vector<float> built_rest_;
  bool sent_transforms_ = false;
  std::string err_;
  int debug_mode_ = 0;
  uint32_t lanes_applied_ = 0;  // the pixel-lane setting the context holds
  sptr_denoise_params denoise_applied_{};  // the denoiser parameters the context holds
  sptr_history_params history_applied_{};  // the history parameters the context holds
  bool motion_applied_ = false;            // the motion setting the context holds
  uint32_t seed_offset_ = 0;    // the seed offset the context holds (history on: advanced at every restart)
  uint32_t acc_frames_ = 0;     // frames of the accumulation the last render() call added to
  sptr_stats flushed_{};        // counters since the last flushStats()
  uint32_t async_calls_ = 0;    // lagged mode: render calls not yet collected
};

}  // namespace backends
