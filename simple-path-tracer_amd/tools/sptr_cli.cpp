// sptr_cli — headless harness for the HIP backend (the reference only has a GLFW window,
// src/GLRenderer.cpp:111-189).  Composes the same state as src/main.cpp (camera (0,3,8)->(0,1,0),
// fov 60, one sun, depth 6) and drives backends::HipBackend exactly as GLRenderer drives a backend:
// one render() per frame, progressive accumulation.
//   sptr_cli [--scene default|default_emitter|test_triangle|sphere_mesh:STACKS:SLICES|gltf:PATH]
//            [--w 800] [--h 600] [--spp 4] [--depth 6] [--env sky|FILE.hdr] [--out image.ppm]
//            [--warmup N] [--json] [--integrator wavefront|pathtracer|optix] [--spf 4] [--launch-mode 0-3]
//            [--lagged] [--denoise N] [--history [M]] [--motion] [--orbit DEG] [--animate K [--rebuild] [--rigid]] [--query-centre-rays [--multi-hit K]] [--query-points-grid N]
// --spp N renders N progressive frames of 1 spp each (GLRenderer's m_accumulated_samples loop);
// --warmup N renders N untimed frames first (then restarts the accumulation by a camera change);
// --json prints one line with per-frame wall-clock statistics (render + RGB8 read back, as the
// window loop pays them) for bench.py's interactive leg.  --lagged: HipBackend::Settings::lagged_readback
// (each render() returns the previous frame's image, read back beside the next frame's kernels).
// --denoise N: HipBackend::Settings::denoise with N a-trous iterations (1..5, default parameters): every
// frame comes back filtered, and the --json line's ms_aov / ms_filter are the per-frame means of the
// pass's device times (sptr_denoise_info; with --lagged, the last frame's alone).
// --history [M]: HipBackend::Settings::history with the cap M on a pixel's history length (without a number:
// HipBackend::kDefaultMaxHistory): with --denoise, the passes carry the integrated image across restarts of the
// accumulation, and every restart draws fresh samples; the --json line's reprojected / ms_reproject are the
// per-frame means of the pixels that took history and of the reprojection launch's device time.
// --orbit DEG: before every frame the camera moves on about the target by DEG degrees (about the vertical
// axis), so that every frame restarts the accumulation: the camera move the history is for.
// --animate K: K frames of --spp samples each; before frame k > 0 analytic sphere i moves by a fixed step
// (0.06 sin 1.7i, 0.04 (i mod 3), 0.05 cos 2.3i), the scene goes through HipBackend::update (a refit in
// place: Settings::dynamic) and the accumulation restarts; the last frame is written.  --rebuild: the same
// loop through HipBackend::build instead.  The --json line adds refits, the mean ms_refit_wall /
// ms_refit_device of the updates and the mean ms_build of the rebuild loop's builds.
// --rigid (with --animate K): every instance also moves rigidly, animation frame k's matrix made from its first
// one (a turn about +Y and a translation), and the scene is built with Settings::transforms, so that update()
// sends the matrices and the device moves the kept rest pose (sptr_update_transforms); without --rigid an
// update sends every vertex.  The --json line reports transform_updates (the updates that went that way) and,
// for every run, the tree's cost and root area after the last update and as built (sptr_tree_cost; the built
// figures are 0 unless --rigid kept them).
// --motion: HipBackend::Settings::motion, meaningful with --animate K --denoise N --history: the updates keep the
// history, read through a snapshot of the geometry it saw; the --json line's snapshots / ms_snapshot are the
// snapshots taken and the mean device time of one.
// --query-centre-rays: after the render, the W x H pixel-centre rays of the camera (the rays of the first-hit
// AOVs: direction getRayDirection((x + 0.5) / W, (y + 0.5) / H), tnear 0, tfar inf) go through
// HipBackend::queryRays; the --json line adds "query": {"rays": n, "hits": h, "tri_hits": k}.
// --multi-hit K (with --query-centre-rays): the same rays also go through HipBackend::queryMultiHit, and the
// "query" object gains "multi_hit": {"k": K, "hits": all hits listed, "count_hist": rays that listed 0 .. K hits}.
// --query-points-grid N --signed [--flip]: the grid goes through HipBackend::querySignedDistance instead (the scene is
// built with Settings::signed_distance) and the counts of negative, positive and missed points and the tables' welded
// vertex, edge, open and irregular edge counts are printed too.
// --query-points-grid N: after the render, an N x N x N grid of points goes through HipBackend::queryPoints with
// max_dist = inf.  The grid covers the flattened scene's bounds (vertices, and spheres as centre +- radius) grown by
// 10 % about their centre c with half-extent h (double): coordinate i of an axis is float((c - 1.1 h) + (2.2 h) *
// ((i + 0.5) / N)), x fastest, then y, then z.  The --json line adds "points": {"n", "found", "dist_min",
// "dist_max", "dist_sum" (double, summed in index order), "geom_hist": points per geomID}.
// --panorama W H: instead of the frames, an equirectangular panorama of W x H pixels from the camera position
// through HipBackend::renderRays (sptr_render_rays): row y has polar angle theta = pi (y + 0.5) / H from +Y and
// column x azimuth phi = 2 pi (x + 0.5) / W, both evaluated in float32 as written (float(pi) times the float
// sum, then the division); their sines and cosines are those of the float32 angle taken in double and rounded
// to float32; the direction is (sin theta cos phi, cos theta, sin theta sin phi) in float32.  --spp N gives every
// ray N samples (frame indices 1 .. N), --depth the bounces.  --out takes the linear image, the mean radiance, as
// a little-endian PFM (rows top to bottom in the file: scale -1, first row y = 0); the --json line is
// {"panorama": [W, H], "samples", "depth", "ms", "closest", "shadow", "chunks"} (sptr_ray_render_info).
// --adaptive THR [--min-spp A] [--spp B] [--step K] [--counts FILE]: instead of the frames, one adaptive call
// through HipBackend::renderAdaptive (sptr_render_adaptive): every pixel takes at least A (default 16) and at most
// B (default 64) samples, K (default 16) more per pass, until its error is below THR.  --out takes the image as
// usual, --counts the samples per pixel as a one-channel little-endian PFM (rows top to bottom: scale -1); the
// --json line is {"adaptive": THR, "min_spp", "max_spp", "step", "width", "height", "depth"} and sptr_adaptive_info's
// fields.
#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hip_backend.h"

static bool build_scene(const std::string& s, scene::SceneDesc& sd, MaterialManager& mm, std::string& err) {
  if (s == "default") sd = scene::BuildDefaultScene();
  else if (s == "default_emitter") {
    sd = scene::BuildDefaultSceneWithEmitter();
    mm.addMaterial(Materials::Light());
  } else if (s == "test_triangle") sd = scene::BuildTestTriangleScene();
  else if (s.rfind("sphere_mesh:", 0) == 0) {
    unsigned a = 0, b = 0;
    if (std::sscanf(s.c_str() + 12, "%u:%u", &a, &b) != 2) { err = "bad sphere_mesh spec"; return false; }
    sd = scene::BuildSphereMeshScene(a, b);
  } else if (s.rfind("gltf:", 0) == 0) {
    return scene::LoadGLTFScene(s.substr(5), 7, sd, &err);
  } else {
    err = "unknown scene " + s;
    return false;
  }
  return true;
}

int main(int argc, char** argv) {
  std::string scene_name = "default", env = "sky", out = "image.ppm";
  int w = 800, h = 600, spp = 4, depth = 6, warmup = 0;
  bool json = false, lagged = false, rebuild = false, query_centre = false, motion = false, rigid = false;
  int multi_hit = 0;  // --multi-hit K
  int points_grid = 0;  // --query-points-grid N
  bool pg_signed = false, pg_flip = false;  // --signed [--flip]
  int pano_w = 0, pano_h = 0;
  bool adaptive = false, spp_given = false;
  double adaptive_thr = 0.0;
  int min_spp = 16, step = 16;
  std::string counts_out;
  int animate = 0;
  std::string integrator = "wavefront";
  int spf = 4, launch_mode = 0, denoise = 0, history = 0;
  double orbit = 0.0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&](void) -> const char* { return i + 1 < argc ? argv[++i] : ""; };
    if (a == "--scene") scene_name = next();
    else if (a == "--w") w = std::atoi(next());
    else if (a == "--h") h = std::atoi(next());
    else if (a == "--spp") spp = std::atoi(next()), spp_given = true;
    else if (a == "--adaptive") adaptive = true, adaptive_thr = std::atof(next());
    else if (a == "--min-spp") min_spp = std::atoi(next());
    else if (a == "--step") step = std::atoi(next());
    else if (a == "--counts") counts_out = next();
    else if (a == "--depth") depth = std::atoi(next());
    else if (a == "--env") env = next();
    else if (a == "--out") out = next();
    else if (a == "--warmup") warmup = std::atoi(next());
    else if (a == "--json") json = true;
    else if (a == "--integrator") integrator = next();
    else if (a == "--spf") spf = std::atoi(next());
    else if (a == "--launch-mode") launch_mode = std::atoi(next());
    else if (a == "--lagged") lagged = true;
    else if (a == "--denoise") denoise = std::atoi(next());
    else if (a == "--history") {
      history = int(backends::HipBackend::kDefaultMaxHistory);
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') history = std::atoi(next());
    } else if (a == "--motion") motion = true;
    else if (a == "--orbit") orbit = std::atof(next());
    else if (a == "--animate") animate = std::atoi(next());
    else if (a == "--rebuild") rebuild = true;
    else if (a == "--rigid") rigid = true;
    else if (a == "--query-centre-rays") query_centre = true;
    else if (a == "--multi-hit" && i + 1 < argc) multi_hit = std::atoi(argv[++i]);
    else if (a == "--query-points-grid" && i + 1 < argc) points_grid = std::atoi(argv[++i]);
    else if (a == "--signed") pg_signed = true;
    else if (a == "--flip") pg_flip = true;
    else if (a == "--panorama") {
      pano_w = std::atoi(next());
      pano_h = std::atoi(next());
      if (pano_w <= 0 || pano_h <= 0) {
        std::fprintf(stderr, "--panorama W H: positive sizes\n");
        return 2;
      }
    }
    else {
      std::fprintf(stderr, "usage: %s [--scene S] [--w W] [--h H] [--spp N] [--depth D] [--env sky|F.hdr] [--out F] [--warmup N] [--json] [--lagged] [--denoise N] [--history [M]] [--motion] [--orbit DEG] [--animate K [--rebuild] [--rigid]] [--query-centre-rays [--multi-hit K]] [--query-points-grid N [--signed [--flip]]] [--panorama W H] [--adaptive THR [--min-spp A] [--step K] [--counts F]]\n",
                   argv[0]);
      return 2;
    }
  }
  scene::SceneDesc sd;
  MaterialManager mm;
  std::string err;
  if (!build_scene(scene_name, sd, mm, err)) {
    std::fprintf(stderr, "scene: %s\n", err.c_str());
    return 1;
  }
  LightManager lm;
  lm.addDirectionalLight(vec3{-0.5f, -1.0f, 0.3f}, vec3{1.0f, 0.95f, 0.8f}, 2.0f);
  EnvironmentManager em;
  if (env != "sky" && !em.loadCubemap(env, &err)) {
    std::fprintf(stderr, "env: %s (using procedural sky)\n", err.c_str());
  }
  Camera cam(vec3{0.0f, 3.0f, 8.0f}, vec3{0.0f, 1.0f, 0.0f}, vec3{0.0f, 1.0f, 0.0f}, 60.0f, float(w) / float(h));
  backends::HipBackend be(0);
  be.setMaterialManager(&mm);
  be.setLightManager(&lm);
  be.setEnvironment(&em);
  backends::HipBackend::Settings st;
  st.max_depth = uint32_t(depth);
  if (integrator == "pathtracer") st.integrator = SPTR_INTEGRATOR_PATHTRACER;
  else if (integrator == "optix") st.integrator = SPTR_INTEGRATOR_OPTIX;
  else if (integrator != "wavefront") {
    std::fprintf(stderr, "unknown integrator %s\n", integrator.c_str());
    return 2;
  }
  st.samples_per_frame = uint32_t(spf);
  st.launch_mode = uint32_t(launch_mode);
  st.lagged_readback = lagged;
  st.denoise.iterations = uint32_t(std::max(0, denoise));
  st.history.max_history = uint32_t(std::max(0, history));
  st.motion = motion;
  st.dynamic = animate > 0 && !rebuild;
  st.transforms = st.dynamic && rigid;
  st.signed_distance = pg_signed;
  be.setSettings(st);
  if (!be.build(sd)) {
    std::fprintf(stderr, "%s\n", be.lastError().c_str());
    return 1;
  }
  if (pano_w > 0) {
    const size_t n = size_t(pano_w) * size_t(pano_h);
    std::vector<float> rays(n * 8, 0.0f), rad(n * 3, 0.0f);
    const sptr_camera dc = cam.toDevice();
    const float pi = 3.14159265358979323846f;
    for (int y = 0; y < pano_h; ++y) {
      const float th = pi * (float(y) + 0.5f) / float(pano_h);
      const float st_ = float(std::sin(double(th))), ct = float(std::cos(double(th)));
      for (int x = 0; x < pano_w; ++x) {
        const float ph = 2.0f * pi * (float(x) + 0.5f) / float(pano_w);
        const float sp = float(std::sin(double(ph))), cp = float(std::cos(double(ph)));
        float* r = &rays[(size_t(y) * pano_w + x) * 8];
        r[0] = dc.pos[0], r[1] = dc.pos[1], r[2] = dc.pos[2];
        r[3] = st_ * cp, r[4] = ct, r[5] = st_ * sp;
      }
    }
    backends::HipBackend::RayRenderInfo ri;
    const uint32_t samples = uint32_t(std::max(1, spp));
    if (!be.renderRays(rays.data(), nullptr, uint32_t(n), samples, 1u, rad.data(), false, false, &ri)) {
      std::fprintf(stderr, "%s\n", be.lastError().c_str());
      return 1;
    }
    for (float& v : rad) v /= float(samples);
    if (json)
      std::printf("{\"panorama\": [%d, %d], \"scene\": \"%s\", \"samples\": %u, \"depth\": %d, \"ms\": %.4f, \"closest\": %llu, "
                  "\"shadow\": %llu, \"chunks\": %u}\n",
                  pano_w, pano_h, scene_name.c_str(), samples, depth, ri.ms, (unsigned long long)ri.closest,
                  (unsigned long long)ri.shadow, ri.chunks);
    else
      std::printf("scene=%s panorama %dx%d samples=%u depth=%d: %.2f ms device\n", scene_name.c_str(), pano_w, pano_h, samples,
                  depth, ri.ms);
    FILE* fp = std::fopen(out.c_str(), "wb");
    if (!fp) return 1;
    std::fprintf(fp, "PF\n%d %d\n-1.0\n", pano_w, pano_h);
    std::fwrite(rad.data(), sizeof(float), rad.size(), fp);
    std::fclose(fp);
    return 0;
  }
  if (adaptive) {
    std::vector<unsigned char> aimg(size_t(w) * h * 3);
    std::vector<uint32_t> cnt(size_t(w) * h);
    backends::HipBackend::AdaptiveSettings as;
    as.threshold = float(adaptive_thr);
    as.min_samples = uint32_t(std::max(0, min_spp));
    as.max_samples = uint32_t(std::max(0, spp_given ? spp : 64));
    as.step = uint32_t(std::max(0, step));
    backends::HipBackend::AdaptiveInfo ai{};
    if (!be.renderAdaptive(aimg.data(), w, h, cam, as, &ai, cnt.data())) {
      std::fprintf(stderr, "%s\n", be.lastError().c_str());
      return 1;
    }
    if (json)
      std::printf("{\"adaptive\": %.9g, \"scene\": \"%s\", \"min_spp\": %u, \"max_spp\": %u, \"step\": %u, \"width\": %d, "
                  "\"height\": %d, \"depth\": %d, \"samples\": %llu, \"rays_closest\": %llu, \"rays_shadow\": %llu, "
                  "\"passes\": %u, \"chunks\": %u, \"active_first\": %u, \"active_last\": %u, \"min_count\": %u, "
                  "\"max_count\": %u, \"ms\": %.4f}\n",
                  double(as.threshold), scene_name.c_str(), as.min_samples, as.max_samples, as.step, w, h, depth,
                  (unsigned long long)ai.samples, (unsigned long long)ai.rays_closest, (unsigned long long)ai.rays_shadow,
                  ai.passes, ai.chunks, ai.active_first, ai.active_last, ai.min_count, ai.max_count, ai.ms);
    else
      std::printf("scene=%s %dx%d adaptive %g, %u..%u spp: %.2f samples per pixel, %u passes, %.2f ms device\n", scene_name.c_str(),
                  w, h, double(as.threshold), as.min_samples, as.max_samples, double(ai.samples) / (double(w) * h), ai.passes, ai.ms);
    if (!counts_out.empty()) {
      std::vector<float> cf(cnt.begin(), cnt.end());
      FILE* fc = std::fopen(counts_out.c_str(), "wb");
      if (!fc) return 1;
      std::fprintf(fc, "Pf\n%d %d\n-1.0\n", w, h);
      std::fwrite(cf.data(), sizeof(float), cf.size(), fc);
      std::fclose(fc);
    }
    FILE* fa = std::fopen(out.c_str(), "wb");
    if (!fa) return 1;
    std::fprintf(fa, "P6\n%d %d\n255\n", w, h);
    std::fwrite(aimg.data(), 1, aimg.size(), fa);
    std::fclose(fa);
    return 0;
  }
  std::vector<unsigned char> img(size_t(w) * h * 3);
  if (warmup > 0) {
    Camera wcam(vec3{0.0f, 3.0f, 8.5f}, vec3{0.0f, 1.0f, 0.0f}, vec3{0.0f, 1.0f, 0.0f}, 60.0f, float(w) / float(h));
    for (int f = 0; f < warmup; ++f) be.render(img.data(), w, h, wcam);  // the camera change below resets
  }
  std::vector<double> frame_ms;
  frame_ms.reserve(size_t(spp) * size_t(std::max(1, animate)));
  double ms_aov = 0.0, ms_filter = 0.0, ms_reproject = 0.0, reprojected = 0.0;
  uint32_t aov_passes = 0;
  int dn_frames = 0;
  (void)be.flushStats();  // (the warmup's counters)
  double ms_refit_wall = 0.0, ms_refit_device = 0.0, ms_build = 0.0, ms_snapshot = 0.0;
  uint32_t refits = 0, snapshots = 0;
  int moves = 0;
  std::vector<scene::mat4> instance0;
  for (const scene::InstanceData& in : sd.instances) instance0.push_back(in.worldFromObject);
  int sent_transforms = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const int shots = std::max(1, animate), total_frames = shots * spp;
  for (int f = 0; f < total_frames; ++f) {
    if (f > 0 && f % spp == 0) {  // the next animation frame: move the spheres, refit or rebuild
      for (size_t i = 0; i < sd.spheres.size(); ++i) {
        const float fi = float(i);
        sd.spheres[i].center = sd.spheres[i].center +
                               vec3{0.06f * std::sin(1.7f * fi), 0.04f * float(i % 3), 0.05f * std::cos(2.3f * fi)};
      }
      if (rigid) {  // ... and the instances: animation frame k's matrix from the first one, nothing accumulates
        const float k = float(f / spp);
        for (size_t i = 0; i < sd.instances.size(); ++i) {
          const float fi = float(i), a = 0.12f * k * (fi + 1.0f);
          scene::mat4 rot = scene::mat4::identity();  // about +Y through the instance's own origin
          rot.m[0][0] = std::cos(a), rot.m[0][2] = -std::sin(a), rot.m[2][0] = std::sin(a), rot.m[2][2] = std::cos(a);
          const scene::mat4 move = scene::translate(
              scene::mat4::identity(), vec3{0.08f * k * std::sin(1.3f * fi + 0.5f), 0.05f * k, 0.06f * k * std::cos(0.7f * fi)});
          sd.instances[i].worldFromObject = scene::multiply(move, scene::multiply(instance0[i], rot));
        }
      }
      if (!(rebuild ? be.build(sd) : be.update(sd))) {
        std::fprintf(stderr, "%s\n", be.lastError().c_str());
        return 1;
      }
      ++moves;
      if (rebuild) {
        ms_build += be.buildMs();
      } else {
        double mw = 0.0, md = 0.0;
        (void)be.refitInfo(&refits, &mw, &md, nullptr);
        ms_refit_wall += mw;
        ms_refit_device += md;
        if (be.lastUpdateSentTransforms()) ++sent_transforms;
        uint32_t sn = 0;
        double msn = 0.0;
        if (motion && be.motionInfo(&sn, &msn, nullptr) && sn != snapshots) {
          snapshots = sn;
          ms_snapshot += msn;
        }
      }
    }
    if (orbit != 0.0) {  // the next camera on the orbit about the target
      const double a = orbit * double(f + 1) * 3.14159265358979323846 / 180.0;
      cam = Camera(vec3{float(8.0 * std::sin(a)), 3.0f, float(8.0 * std::cos(a))}, vec3{0.0f, 1.0f, 0.0f}, vec3{0.0f, 1.0f, 0.0f},
                   60.0f, float(w) / float(h));
    }
    const auto f0 = std::chrono::steady_clock::now();
    be.render(img.data(), w, h, cam);
    if (denoise > 0 && (!lagged || f == total_frames - 1)) {  // (waits for the pass: a lagged loop asks once, at its end)
      double a = 0.0, fl = 0.0;
      if (be.denoiseInfo(&a, &fl, &aov_passes)) {
        ms_aov += a;
        ms_filter += fl;
        ++dn_frames;
      }
      uint32_t took = 0;
      double mr = 0.0;
      if (history > 0 && be.historyInfo(&took, &mr, nullptr)) {
        reprojected += double(took);
        ms_reproject += mr;
      }
    }
    frame_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f0).count());
  }
  const sptr_stats tot = be.flushStats();  // (lagged: waits for the last frames, inside the clock)
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const uint64_t rays = tot.rays_closest + tot.rays_shadow;
  size_t q_rays = 0, q_hits = 0, q_tri_hits = 0, mh_hits = 0;
  std::vector<size_t> mh_hist;
  if (multi_hit != 0 && (!query_centre || multi_hit < 0)) {
    std::fprintf(stderr, "--multi-hit K needs --query-centre-rays and K >= 1\n");
    return 1;
  }
  if (query_centre) {
    std::vector<float> qr(size_t(w) * h * 8);
    const sptr_camera dc = cam.toDevice();
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const vec3 d = cam.getRayDirection((float(x) + 0.5f) / float(w), (float(y) + 0.5f) / float(h));
        float* r = &qr[(size_t(y) * w + x) * 8];
        r[0] = dc.pos[0], r[1] = dc.pos[1], r[2] = dc.pos[2];
        r[3] = d.x, r[4] = d.y, r[5] = d.z;
        r[6] = 0.0f, r[7] = std::numeric_limits<float>::infinity();
      }
    backends::HipBackend::HitBuffers hb;
    if (!be.queryRays(qr.data(), uint32_t(size_t(w) * h), false, hb)) {
      std::fprintf(stderr, "%s\n", be.lastError().c_str());
      return 1;
    }
    // geomIDs: the triangle geometries first, then one per analytic sphere
    const size_t tri_geoms = be.getGeomMaterialMapping().size() - sd.spheres.size();
    q_rays = hb.geom.size();
    for (uint32_t g : hb.geom) {
      if (g == 0xFFFFFFFFu) continue;
      ++q_hits;
      if (g < tri_geoms) ++q_tri_hits;
    }
    if (multi_hit > 0) {  // the same rays through sptr_query_multi_hit: how many of them found 0, 1, .. K hits
      backends::HipBackend::MultiHitBuffers mb;
      if (!be.queryMultiHit(qr.data(), uint32_t(size_t(w) * h), uint32_t(multi_hit), mb)) {
        std::fprintf(stderr, "%s\n", be.lastError().c_str());
        return 1;
      }
      mh_hist.assign(size_t(multi_hit) + 1, 0);
      for (uint32_t c : mb.count) {
        mh_hits += c;
        ++mh_hist[std::min<size_t>(c, size_t(multi_hit))];
      }
    }
  }
  size_t pg_n = 0, pg_found = 0;
  double pg_min = 0.0, pg_max = 0.0, pg_sum = 0.0;
  std::vector<size_t> pg_hist;
  size_t sg_neg = 0, sg_pos = 0, sg_miss = 0;
  uint64_t sg_counts[4] = {0, 0, 0, 0};
  if (points_grid < 0 || points_grid > 512) {
    std::fprintf(stderr, "--query-points-grid N needs 1 <= N <= 512\n");
    return 1;
  }
  if (points_grid > 0) {
    const scene::FlatScene flat = scene::Flatten(sd);
    const sptr_scene fv = flat.view();
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    bool any = false;
    auto grow = [&](int a, double l, double h2) {
      lo[a] = any ? std::min(lo[a], l) : l;
      hi[a] = any ? std::max(hi[a], h2) : h2;
    };
    for (uint32_t v = 0; v < fv.num_verts; ++v) {
      for (int a = 0; a < 3; ++a) grow(a, fv.positions[size_t(v) * 3 + a], fv.positions[size_t(v) * 3 + a]);
      any = true;
    }
    for (uint32_t k = 0; k < fv.num_spheres; ++k) {
      const float* sp = fv.spheres + size_t(k) * 4;
      for (int a = 0; a < 3; ++a) grow(a, double(sp[a]) - double(sp[3]), double(sp[a]) + double(sp[3]));
      any = true;
    }
    const int N = points_grid;
    std::vector<float> pts(size_t(N) * N * N * 4);
    double c0[3], h0[3];
    for (int a = 0; a < 3; ++a) {
      c0[a] = (lo[a] + hi[a]) / 2.0;
      h0[a] = (hi[a] - lo[a]) / 2.0;
    }
    auto coord = [&](int a, int i) { return float((c0[a] - 1.1 * h0[a]) + (2.2 * h0[a]) * ((i + 0.5) / N)); };
    size_t at = 0;
    for (int z = 0; z < N; ++z)
      for (int y = 0; y < N; ++y)
        for (int x = 0; x < N; ++x) {
          pts[at++] = coord(0, x);
          pts[at++] = coord(1, y);
          pts[at++] = coord(2, z);
          pts[at++] = std::numeric_limits<float>::infinity();
        }
    backends::HipBackend::SignedBuffers sb;
    backends::HipBackend::PointBuffers& pb = sb.points;
    pg_n = pts.size() / 4;
    if (!(pg_signed ? be.querySignedDistance(pts.data(), uint32_t(pg_n), pg_flip, sb) : be.queryPoints(pts.data(), uint32_t(pg_n), pb))) {
      std::fprintf(stderr, "%s\n", be.lastError().c_str());
      return 1;
    }
    if (pg_signed) {
      for (size_t i = 0; i < pg_n; ++i) {
        if (sb.feature[i] == 0xFFFFFFFFu) ++sg_miss;
        else if (std::signbit(sb.signed_dist[i])) ++sg_neg;
        else ++sg_pos;
      }
      for (int i = 0; i < 4; ++i) sg_counts[i] = sb.counts[i];
    }
    pg_hist.assign(size_t(fv.num_tri_geoms) + fv.num_spheres, 0);
    for (size_t i = 0; i < pg_n; ++i) {
      if (pb.geom[i] == 0xFFFFFFFFu) continue;
      const double d = pb.dist[i];
      pg_min = pg_found ? std::min(pg_min, d) : d;
      pg_max = pg_found ? std::max(pg_max, d) : d;
      pg_sum += d;
      ++pg_found;
      if (pb.geom[i] < pg_hist.size()) ++pg_hist[pb.geom[i]];
    }
  }
  const double ms = tot.ms_total;
  if (json) {
    std::vector<double> s = frame_ms;
    std::sort(s.begin(), s.end());
    auto pct = [&](double q) { return s.empty() ? 0.0 : s[std::min(s.size() - 1, size_t(q * double(s.size())))]; };
    std::printf("{\"scene\": \"%s\", \"launch_mode\": %d, \"width\": %d, \"height\": %d, \"frames\": %d, \"spp_per_frame\": 1, "
                "\"depth\": %d, \"ms_per_frame_wall\": %.4f, \"ms_per_frame_p50\": %.4f, \"ms_per_frame_p99\": %.4f, "
                "\"ms_per_frame_device\": %.4f, \"fps\": %.1f, \"mrays_per_s_wall\": %.1f, "
                "\"lagged_readback\": %s, \"denoise\": %d, \"ms_aov\": %.4f, \"ms_filter\": %.4f, \"aov_passes\": %u, \"history\": %d, \"reprojected\": %.1f, \"ms_reproject\": %.4f, \"motion\": %d, \"snapshots\": %u, \"ms_snapshot\": %.4f, \"animate\": %d, \"refits\": %u, \"ms_refit_wall\": %.4f, \"ms_refit_device\": %.4f, \"ms_build\": %.4f, \"path\": \"backends::HipBackend::render (sptr_render + %s per frame)\"",
                scene_name.c_str(), launch_mode, w, h, total_frames, depth, wall / total_frames, pct(0.5), pct(0.99), ms / total_frames,
                wall > 0 ? 1e3 * total_frames / wall : 0.0, wall > 0 ? rays / (wall * 1e3) : 0.0, lagged ? "true" : "false", denoise, dn_frames ? ms_aov / dn_frames : 0.0,
                dn_frames ? ms_filter / dn_frames : 0.0, aov_passes, history, dn_frames ? reprojected / dn_frames : 0.0,
                dn_frames ? ms_reproject / dn_frames : 0.0, motion ? 1 : 0, snapshots, snapshots ? ms_snapshot / snapshots : 0.0, animate, refits,
                moves && !rebuild ? ms_refit_wall / moves : 0.0, moves && !rebuild ? ms_refit_device / moves : 0.0,
                moves && rebuild ? ms_build / moves : 0.0,
                lagged ? "sptr_read_rgb8_lagged" : "sptr_read_rgb8");
    // the tree after the last update against the tree as built (the latter 0 unless --rigid kept the figures)
    double tc[4] = {0.0, 0.0, 0.0, 0.0};
    (void)be.treeCost(&tc[0], &tc[1], &tc[2], &tc[3]);
    std::printf(", \"rigid\": %d, \"transform_updates\": %d, \"tree_cost\": %.17g, \"root_area\": %.17g, "
                "\"tree_cost_at_build\": %.17g, \"root_area_at_build\": %.17g",
                rigid ? 1 : 0, sent_transforms, tc[0], tc[1], tc[2], tc[3]);
    if (query_centre) {
      std::printf(", \"query\": {\"rays\": %zu, \"hits\": %zu, \"tri_hits\": %zu", q_rays, q_hits, q_tri_hits);
      if (multi_hit > 0) {
        std::printf(", \"multi_hit\": {\"k\": %d, \"hits\": %zu, \"count_hist\": [", multi_hit, mh_hits);
        for (size_t i = 0; i < mh_hist.size(); ++i) std::printf("%s%zu", i ? ", " : "", mh_hist[i]);
        std::printf("]}");
      }
      std::printf("}");
    }
    if (points_grid > 0) {
      std::printf(", \"points\": {\"n\": %zu, \"found\": %zu, \"dist_min\": %.17g, \"dist_max\": %.17g, \"dist_sum\": %.17g, "
                  "\"geom_hist\": [", pg_n, pg_found, pg_min, pg_max, pg_sum);
      for (size_t i = 0; i < pg_hist.size(); ++i) std::printf("%s%zu", i ? ", " : "", pg_hist[i]);
      std::printf("]}");
      if (pg_signed)
        std::printf(", \"signed\": {\"flip\": %d, \"negative\": %zu, \"positive\": %zu, \"missed\": %zu, \"welded_vertices\": %llu, "
                    "\"edges\": %llu, \"open_edges\": %llu, \"irregular_edges\": %llu}",
                    pg_flip ? 1 : 0, sg_neg, sg_pos, sg_miss, (unsigned long long)sg_counts[0], (unsigned long long)sg_counts[1],
                    (unsigned long long)sg_counts[2], (unsigned long long)sg_counts[3]);
    }
    std::printf("}\n");
  } else {
    std::printf("scene=%s %dx%d spp=%d depth=%d: %.2f ms device, %.2f ms wall, %.1f Mrays/s (device)\n",
                scene_name.c_str(), w, h, spp, depth, ms, wall, ms > 0 ? rays / (ms * 1e3) : 0.0);
  }
  FILE* fp = std::fopen(out.c_str(), "wb");
  if (!fp) return 1;
  std::fprintf(fp, "P6\n%d %d\n255\n", w, h);
  std::fwrite(img.data(), 1, img.size(), fp);
  std::fclose(fp);
  return 0;
}
