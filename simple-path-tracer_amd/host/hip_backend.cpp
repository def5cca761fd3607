// hip_backend.cpp — backends::HipBackend over the C ABI (include/sptr_hip.h).
#include "hip_backend.h"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace backends {

HipBackend::HipBackend(int device) : device_(device) {}
HipBackend::~HipBackend() { destroy(); }

bool HipBackend::ensureContext() {
  if (ctx_) return true;
  const int rc = sptr_create(device_, &ctx_);
  if (rc != SPTR_OK) {
    err_ = "HipBackend: sptr_create failed (" + std::to_string(rc) + ")";
    ctx_ = nullptr;
    return false;
  }
  sptr_set_debug_mode(ctx_, debug_mode_);
  return true;
}

void HipBackend::destroy() {
  if (ctx_) (void)flushStats();
  if (ctx_) sptr_destroy(ctx_);
  ctx_ = nullptr;
  built_ = false;
  frame_index_ = 0;
  has_last_camera_ = false;
}

void HipBackend::setDebugMode(int mode) {
  debug_mode_ = mode;
  if (ctx_) sptr_set_debug_mode(ctx_, mode);
  frame_index_ = 0;
}

bool HipBackend::build(const scene::SceneDesc& sd) {
  if (!ensureContext()) return false;
  return buildScene(sd, scene::Flatten(sd));
}

// The tree is built over the world-space flattening, the scene as it looks; with Settings::transforms the
// meshes' own vertices then become the rest pose the instances' matrices move.
bool HipBackend::buildScene(const scene::SceneDesc& sd, const scene::FlatScene& flat) {
  built_rest_.clear();
  if (!buildFlat(flat)) return false;
  if (settings_.transforms && built_verts_) {
    scene::FlatScene obj = scene::Flatten(sd, true);
    // (a scene built with split references keeps no rest pose: update() then sends vertices, and builds again)
    if (sptr_set_rest_positions(ctx_, obj.positions.data(), uint32_t(obj.positions.size() / 3), 0u) == SPTR_OK)
      built_rest_ = std::move(obj.positions);
  }
  return true;
}

bool HipBackend::buildFlat(const scene::FlatScene& flat) {
  const sptr_scene v = flat.view();
  built_ = false;
  const uint32_t dyn = settings_.transforms ? uint32_t(SPTR_DYNAMIC_REFIT | SPTR_DYNAMIC_TRANSFORMS)
                                            : (settings_.dynamic ? uint32_t(SPTR_DYNAMIC_REFIT) : 0u);
  if (sptr_set_dynamic(ctx_, dyn) != SPTR_OK) return false;
  if (sptr_set_signed_distance(ctx_, settings_.signed_distance ? 1u : 0u) != SPTR_OK) return false;
  const int rc = sptr_upload_scene(ctx_, &v);
  if (rc != SPTR_OK) {
    err_ = std::string("HipBackend::build: ") + sptr_last_error(ctx_);
    return false;
  }
  geom_material_ = flat.geom_material;
  built_indices_ = flat.indices;
  built_geom_first_ = flat.tri_geom_first;
  built_verts_ = flat.positions.size() / 3;
  built_spheres_ = flat.spheres.size() / 4;
  built_dynamic_ = settings_.dynamic || settings_.transforms;
  built_ = true;
  frame_index_ = 0;
  return true;
}

bool HipBackend::update(const scene::SceneDesc& sd) {
  if (!ensureContext()) return false;
  sent_transforms_ = false;
  if (built_ && built_dynamic_ && !built_rest_.empty()) {
    // the flattening without its transform: equal to the built one, only matrices and spheres can have moved
    const scene::FlatScene obj = scene::Flatten(sd, true);
    if (obj.positions == built_rest_ && obj.spheres.size() / 4 == built_spheres_ && obj.indices == built_indices_ &&
        obj.tri_geom_first == built_geom_first_ && obj.geom_material == geom_material_) {
      const std::vector<float> xf = scene::InstanceMatrices(sd);
      const int rc = sptr_update_transforms(ctx_, xf.data(), uint32_t(xf.size() / 16),
                                            built_spheres_ ? obj.spheres.data() : nullptr, uint32_t(built_spheres_), 0u);
      if (rc == SPTR_OK) {
        frame_index_ = 0;
        sent_transforms_ = true;
        return true;
      }
      // (a matrix that is not finite is refused: the vertices go the ordinary way below)
    }
  }
  const scene::FlatScene flat = scene::Flatten(sd);
  const bool same = built_ && built_dynamic_ && flat.positions.size() / 3 == built_verts_ &&
                    flat.spheres.size() / 4 == built_spheres_ && flat.indices == built_indices_ &&
                    flat.tri_geom_first == built_geom_first_ && flat.geom_material == geom_material_ &&
                    (built_verts_ || built_spheres_);
  if (same) {
    const int rc = sptr_update_geometry(ctx_, built_verts_ ? flat.positions.data() : nullptr, uint32_t(built_verts_),
                                        built_spheres_ ? flat.spheres.data() : nullptr, uint32_t(built_spheres_), 0u);
    if (rc == SPTR_OK) {
      frame_index_ = 0;
      return true;
    }
    // (a scene built with split references cannot be refitted: built again below)
  }
  return buildScene(sd, flat);
}

bool HipBackend::syncState() {
  if (mats_dirty_) {
    std::vector<sptr_material> m;
    if (mm_) mm_->buildDeviceMaterials(m);
    else MaterialManager().buildDeviceMaterials(m);
    if (sptr_set_materials(ctx_, m.data(), uint32_t(m.size())) != SPTR_OK) return false;
    mats_dirty_ = false;
    frame_index_ = 0;
  }
  if (lights_dirty_) {
    std::vector<sptr_light> l;
    if (lm_) lm_->buildDeviceLights(l);
    if (sptr_set_lights(ctx_, l.data(), uint32_t(l.size())) != SPTR_OK) return false;
    lights_dirty_ = false;
    frame_index_ = 0;
  }
  if (env_dirty_) {
    sptr_environment e{};
    e.intensity = 0.8f;
    e.max_clamp = 5.0f;
    if (env_) e = env_->toDevice();
    if (sptr_set_environment(ctx_, &e) != SPTR_OK) return false;
    env_dirty_ = false;
    frame_index_ = 0;
  }
  if (std::memcmp(&settings_.denoise, &denoise_applied_, sizeof(sptr_denoise_params)) != 0) {
    if (sptr_set_denoise(ctx_, &settings_.denoise) != SPTR_OK) return false;
    denoise_applied_ = settings_.denoise;  // (the accumulation goes on: the filter only reads it)
  }
  if (std::memcmp(&settings_.history, &history_applied_, sizeof(sptr_history_params)) != 0) {
    if (sptr_set_denoise_history(ctx_, &settings_.history) != SPTR_OK) return false;
    history_applied_ = settings_.history;
  }
  if (settings_.motion != motion_applied_) {
    if (sptr_set_history_motion(ctx_, settings_.motion ? 1u : 0u) != SPTR_OK) return false;
    motion_applied_ = settings_.motion;
  }
  return true;
}

void HipBackend::addStats(const sptr_stats& s) {
  flushed_.rays_closest += s.rays_closest;
  flushed_.rays_shadow += s.rays_shadow;
  flushed_.samples += s.samples;
  flushed_.waves += s.waves;
  flushed_.ms_total += s.ms_total;
  flushed_.ms_trace += s.ms_trace;
  flushed_.trace_launches += s.trace_launches;
}

sptr_stats HipBackend::flushStats() {
  if (ctx_ && async_calls_) {
    sptr_stats s{};
    if (sptr_collect_stats(ctx_, &s) == SPTR_OK) {
      stats_ = s;
      addStats(s);
    }
    async_calls_ = 0;
  }
  const sptr_stats out = flushed_;
  flushed_ = sptr_stats{};
  return out;
}

bool HipBackend::renderInternal(int w, int h, const Camera& camera, bool async) {
  if (!built_ || !ctx_) {
    err_ = "HipBackend::render: build() has not succeeded";
    return false;
  }
  if (!syncState()) {
    err_ = std::string("HipBackend: state upload failed: ") + sptr_last_error(ctx_);
    return false;
  }
  // progressive reset on resize / camera change (OptixBackend.cpp:1518-1542, eps 1e-4)
  const vec3 p = camera.getPosition(), f = camera.getFront(), u = camera.getUp();
  const std::array<float, 9> cam = {p.x, p.y, p.z, f.x, f.y, f.z, u.x, u.y, u.z};
  bool changed = !has_last_camera_ || w != last_w_ || h != last_h_;
  for (int i = 0; i < 9 && !changed; ++i) changed = std::fabs(cam[size_t(i)] - last_cam_[size_t(i)]) > 1e-4f;
  if (settings_.pixel_lanes != lanes_applied_) {
    if (sptr_set_pixel_lanes(ctx_, settings_.pixel_lanes) != SPTR_OK) {
      err_ = std::string("HipBackend::render: ") + sptr_last_error(ctx_);
      return false;
    }
    lanes_applied_ = settings_.pixel_lanes;
    changed = true;  // a new accumulation in the new lane mode
  }
  if (changed) frame_index_ = 0;
  // history on: a restart draws the samples after those of the accumulation it ends; off: the seeds as ever
  const bool history = settings_.history.max_history != 0u && settings_.denoise.iterations != 0u &&
                       settings_.integrator == SPTR_INTEGRATOR_WAVEFRONT;
  uint32_t offset = 0;
  if (history) {
    offset = seed_offset_;
    if (frame_index_ == 0) offset += acc_frames_;
    if (offset > 0xF0000000u) offset = 0;  // (far from the 32-bit end of the accumulation indices)
  }
  if (frame_index_ == 0) acc_frames_ = 0;
  if (offset != seed_offset_) {
    if (sptr_set_seed_offset(ctx_, offset) != SPTR_OK) {
      err_ = std::string("HipBackend::render: ") + sptr_last_error(ctx_);
      return false;
    }
    seed_offset_ = offset;
  }
  has_last_camera_ = true;
  last_cam_ = cam;
  last_w_ = w;
  last_h_ = h;

  sptr_frame fr{};
  fr.width = w;
  fr.height = h;
  fr.camera = camera.toDevice();
  fr.frame_begin = frame_index_ + 1;
  fr.spp = settings_.spp_per_call ? settings_.spp_per_call : 1;
  fr.max_depth = settings_.max_depth;
  fr.shard_rank = 0;
  fr.shard_count = 1;
  fr.integrator = settings_.integrator;
  fr.samples_per_frame = settings_.samples_per_frame;
  if (async) fr.flags |= SPTR_FRAME_ASYNC;
  if (sptr_set_launch_mode(ctx_, settings_.launch_mode) != SPTR_OK) {
    err_ = std::string("HipBackend::render: ") + sptr_last_error(ctx_);
    return false;
  }
  sptr_stats st{};
  const int rc = sptr_render(ctx_, &fr, nullptr, &st);
  if (rc != SPTR_OK) {
    err_ = std::string("HipBackend::render: ") + sptr_last_error(ctx_);
    return false;
  }
  if (async) {
    ++async_calls_;
  } else {
    stats_ = st;  // (a synchronous call also collects any pending asynchronous ones)
    addStats(st);
    async_calls_ = 0;
  }
  frame_index_ += fr.spp;
  acc_frames_ = frame_index_;
  return true;
}

void HipBackend::render(unsigned char* pixels, int width, int height, const Camera& camera) {
  const bool lagged = settings_.lagged_readback;
  if (!renderInternal(width, height, camera, lagged)) {
    std::fprintf(stderr, "%s\n", err_.c_str());
    return;
  }
  if (lagged) {
    // the previous frame's image, copied while this frame's kernels run; none yet (the first frame or a
    // resize): this frame's, synchronously
    uint32_t got = 0;
    if (sptr_read_rgb8_lagged(ctx_, pixels, &got) != SPTR_OK) {
      std::fprintf(stderr, "HipBackend: %s\n", sptr_last_error(ctx_));
      return;
    }
    if (!got && sptr_read_rgb8(ctx_, pixels) != SPTR_OK) std::fprintf(stderr, "HipBackend: %s\n", sptr_last_error(ctx_));
    if (async_calls_ >= kLaggedCollect) {  // bounded: each pending call holds its call-span events
      sptr_stats s{};
      if (sptr_collect_stats(ctx_, &s) == SPTR_OK) {
        stats_ = s;
        addStats(s);
      }
      async_calls_ = 0;
    }
    return;
  }
  if (sptr_read_rgb8(ctx_, pixels) != SPTR_OK) std::fprintf(stderr, "HipBackend: %s\n", sptr_last_error(ctx_));
}

bool HipBackend::renderLinear(float* rgb32, int width, int height, const Camera& camera) {
  if (!renderInternal(width, height, camera)) return false;
  if (sptr_read_accum(ctx_, rgb32) != SPTR_OK) return false;  // PathTracer mode: mean tonemapped colour
  const float n = float(frame_index_);
  for (size_t i = 0; i < size_t(width) * height * 3; ++i) rgb32[i] /= n;
  return true;
}

bool HipBackend::queryRays(const float* rays, uint32_t n, bool anyHit, HitBuffers& out) {
  if (!ctx_ || !built_) {
    err_ = "HipBackend::queryRays: build() has not succeeded";
    return false;
  }
  sptr_ray_query q{};
  q.rays = rays;
  q.n = n;
  if (anyHit) {
    out.occluded.assign(n, 0);
    q.flags = SPTR_QUERY_ANY_HIT;
    q.occluded = out.occluded.data();
  } else {
    out.geom.assign(n, 0u);
    out.prim.assign(n, 0u);
    out.t.assign(n, 0.0f);
    out.ng.assign(size_t(n) * 3, 0.0f);
    out.uv.assign(size_t(n) * 2, 0.0f);
    q.geom = out.geom.data();
    q.prim = out.prim.data();
    q.t = out.t.data();
    q.ng = out.ng.data();
    q.uv = out.uv.data();
  }
  if (n == 0u) return true;
  if (sptr_query_rays(ctx_, &q, nullptr) != SPTR_OK) {
    err_ = std::string("HipBackend::queryRays: ") + sptr_last_error(ctx_);
    return false;
  }
  return true;
}

bool HipBackend::queryMultiHit(const float* rays, uint32_t n, uint32_t maxHits, MultiHitBuffers& out) {
  if (!ctx_ || !built_) {
    err_ = "HipBackend::queryMultiHit: build() has not succeeded";
    return false;
  }
  const size_t m = size_t(n) * maxHits;
  out.count.assign(n, 0u);
  out.geom.assign(m, 0u);
  out.prim.assign(m, 0u);
  out.t.assign(m, 0.0f);
  out.ng.assign(m * 3, 0.0f);
  out.uv.assign(m * 2, 0.0f);
  sptr_multi_hit_query q{};
  q.rays = rays;
  q.n = n;
  q.max_hits = maxHits;
  q.count = out.count.data();
  q.geom = out.geom.data();
  q.prim = out.prim.data();
  q.t = out.t.data();
  q.ng = out.ng.data();
  q.uv = out.uv.data();
  if (sptr_query_multi_hit(ctx_, &q, nullptr) != SPTR_OK) {
    err_ = std::string("HipBackend::queryMultiHit: ") + sptr_last_error(ctx_);
    return false;
  }
  return true;
}

bool HipBackend::queryPoints(const float* points, uint32_t n, PointBuffers& out) {
  if (!ctx_ || !built_) {
    err_ = "HipBackend::queryPoints: build() has not succeeded";
    return false;
  }
  out.geom.assign(n, 0u);
  out.prim.assign(n, 0u);
  out.dist2.assign(n, 0.0f);
  out.dist.assign(n, 0.0f);
  out.point.assign(size_t(n) * 3, 0.0f);
  out.uv.assign(size_t(n) * 2, 0.0f);
  out.ng.assign(size_t(n) * 3, 0.0f);
  if (n == 0u) return true;
  sptr_point_query q{};
  q.points = points;
  q.n = n;
  q.geom = out.geom.data();
  q.prim = out.prim.data();
  q.dist2 = out.dist2.data();
  q.dist = out.dist.data();
  q.point = out.point.data();
  q.uv = out.uv.data();
  q.ng = out.ng.data();
  if (sptr_query_points(ctx_, &q, nullptr) != SPTR_OK) {
    err_ = std::string("HipBackend::queryPoints: ") + sptr_last_error(ctx_);
    return false;
  }
  return true;
}

bool HipBackend::querySignedDistance(const float* points, uint32_t n, bool flipTriangles, SignedBuffers& out) {
  if (!ctx_ || !built_) {
    err_ = "HipBackend::querySignedDistance: build() has not succeeded";
    return false;
  }
  PointBuffers& pb = out.points;
  pb.geom.assign(n, 0u);
  pb.prim.assign(n, 0u);
  pb.dist2.assign(n, 0.0f);
  pb.dist.assign(n, 0.0f);
  pb.point.assign(size_t(n) * 3, 0.0f);
  pb.uv.assign(size_t(n) * 2, 0.0f);
  pb.ng.assign(size_t(n) * 3, 0.0f);
  out.signed_dist.assign(n, 0.0f);
  out.normal.assign(size_t(n) * 3, 0.0f);
  out.feature.assign(n, 0u);
  sptr_signed_query q{};
  q.q.points = points;
  q.q.n = n;
  q.q.flags = flipTriangles ? uint32_t(SPTR_SIGNED_FLIP_TRIANGLES) : 0u;
  q.q.geom = pb.geom.data();
  q.q.prim = pb.prim.data();
  q.q.dist2 = pb.dist2.data();
  q.q.dist = pb.dist.data();
  q.q.point = pb.point.data();
  q.q.uv = pb.uv.data();
  q.q.ng = pb.ng.data();
  q.signed_dist = out.signed_dist.data();
  q.normal = out.normal.data();
  q.feature = out.feature.data();
  sptr_signed_info_t info{};
  if (sptr_query_signed_distance(ctx_, &q, nullptr) != SPTR_OK || sptr_signed_info(ctx_, &info) != SPTR_OK) {
    err_ = std::string("HipBackend::querySignedDistance: ") + sptr_last_error(ctx_);
    return false;
  }
  out.counts[0] = info.welded_vertices;
  out.counts[1] = info.edges;
  out.counts[2] = info.open_edges;
  out.counts[3] = info.irregular_edges;
  return true;
}

bool HipBackend::renderRays(const float* rays, const uint32_t* seeds, uint32_t n, uint32_t samples, uint32_t frame_index,
                            float* radiance, bool accumulate, bool normalize, RayRenderInfo* info) {
  if (!ctx_ || !built_) {
    err_ = "HipBackend::renderRays: build() has not succeeded";
    return false;
  }
  if (!syncState()) {
    err_ = std::string("HipBackend: state upload failed: ") + sptr_last_error(ctx_);
    return false;
  }
  sptr_ray_render q{};
  q.rays = rays;
  q.seeds = seeds;
  q.n = n;
  q.samples = samples;
  q.frame_index = frame_index;
  q.max_depth = settings_.max_depth;
  q.flags = (accumulate ? SPTR_RAYS_ACCUMULATE : 0u) | (normalize ? SPTR_RAYS_NORMALIZE : 0u);
  q.radiance = radiance;
  if (sptr_render_rays(ctx_, &q, nullptr) != SPTR_OK ||
      (info && sptr_ray_render_info(ctx_, &info->ms, &info->closest, &info->shadow, &info->chunks) != SPTR_OK)) {
    err_ = std::string("HipBackend::renderRays: ") + sptr_last_error(ctx_);
    return false;
  }
  return true;
}

bool HipBackend::renderAdaptive(uint8_t* rgb, int width, int height, const Camera& camera, const AdaptiveSettings& as,
                                AdaptiveInfo* info, uint32_t* counts) {
  if (!ctx_ || !built_) {
    err_ = "HipBackend::renderAdaptive: build() has not succeeded";
    return false;
  }
  if (!syncState()) {
    err_ = std::string("HipBackend: state upload failed: ") + sptr_last_error(ctx_);
    return false;
  }
  sptr_frame fr{};
  fr.width = width;
  fr.height = height;
  fr.camera = camera.toDevice();
  fr.frame_begin = 1;
  fr.spp = 1;
  fr.max_depth = settings_.max_depth;
  fr.shard_rank = 0;
  fr.shard_count = 1;
  fr.integrator = SPTR_INTEGRATOR_WAVEFRONT;
  sptr_adaptive_params ap{};
  ap.threshold = as.threshold;
  ap.min_samples = as.min_samples;
  ap.max_samples = as.max_samples;
  ap.step = as.step;
  // the accumulation now holds unequal counts: render() starts a new one
  frame_index_ = 0;
  has_last_camera_ = false;
  if (sptr_render_adaptive(ctx_, &fr, &ap, info) != SPTR_OK || (rgb && sptr_read_rgb8(ctx_, rgb) != SPTR_OK) ||
      (counts && sptr_read_sample_counts(ctx_, counts) != SPTR_OK)) {
    err_ = std::string("HipBackend::renderAdaptive: ") + sptr_last_error(ctx_);
    return false;
  }
  return true;
}

}  // namespace backends
