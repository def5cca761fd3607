// host_api.cpp — C ABI access to the host-side scene layer (sptr_host_* in include/sptr_hip.h), so
// foreign callers (ctypes harness, CLI) build scenes, cameras and material tables with exactly the
// C++ code the HipBackend uses.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/closest_point.h"
#include "../csrc/tile_map.h"
#include "scene_desc.h"
#include "shading.h"

struct sptr_host_scene {
  scene::FlatScene flat;
};

extern "C" {

int sptr_host_builtin_scene(const char* name, uint32_t p0, uint32_t p1, sptr_host_scene** out) {
  if (!name || !out) return SPTR_ERR_INVALID;
  *out = nullptr;
  const std::string n(name);
  scene::SceneDesc sd;
  if (n == "default") sd = scene::BuildDefaultScene();
  else if (n == "default_emitter") sd = scene::BuildDefaultSceneWithEmitter();
  else if (n == "test_triangle") sd = scene::BuildTestTriangleScene();
  else if (n == "sphere_mesh") {
    if (p0 == 0 || p1 == 0) return SPTR_ERR_INVALID;
    sd = scene::BuildSphereMeshScene(p0, p1);
  } else if (n.rfind("gltf:", 0) == 0) {
    std::string err;
    if (!scene::LoadGLTFScene(n.substr(5), p0, sd, &err)) return SPTR_ERR_INVALID;
  } else {
    return SPTR_ERR_INVALID;
  }
  sptr_host_scene* s = new sptr_host_scene();
  s->flat = scene::Flatten(sd);
  *out = s;
  return SPTR_OK;
}

int sptr_host_scene_view(const sptr_host_scene* s, sptr_scene* view) {
  if (!s || !view) return SPTR_ERR_INVALID;
  *view = s->flat.view();
  return SPTR_OK;
}

void sptr_host_scene_free(sptr_host_scene* s) { delete s; }

int sptr_host_camera_lookat(const float pos[3], const float target[3], float fov_deg, float aspect, sptr_camera* out) {
  if (!pos || !target || !out) return SPTR_ERR_INVALID;
  const Camera c(vec3{pos[0], pos[1], pos[2]}, vec3{target[0], target[1], target[2]}, vec3{0.0f, 1.0f, 0.0f}, fov_deg,
                 aspect);
  *out = c.toDevice();
  return SPTR_OK;
}

int sptr_host_preset_materials(int with_light, sptr_material* out, int capacity) {
  MaterialManager mm;
  if (with_light) mm.addMaterial(Materials::Light());
  std::vector<sptr_material> v;
  mm.buildDeviceMaterials(v);
  if (out)
    for (int i = 0; i < int(v.size()) && i < capacity; ++i) out[i] = v[size_t(i)];
  return int(v.size());
}

int sptr_host_default_lights(sptr_light* out, int capacity) {
  LightManager lm;  // setupLights, src/main.cpp:85-94
  lm.addDirectionalLight(vec3{-0.5f, -1.0f, 0.3f}, vec3{1.0f, 0.95f, 0.8f}, 2.0f);
  std::vector<sptr_light> v;
  lm.buildDeviceLights(v);
  if (out)
    for (int i = 0; i < int(v.size()) && i < capacity; ++i) out[i] = v[size_t(i)];
  return int(v.size());
}

int sptr_host_equirect_to_faces(const float* rgb, int32_t w, int32_t h, int32_t size, float* faces) {
  if (!rgb || !faces || w <= 0 || h <= 0 || size < 2) return SPTR_ERR_INVALID;
  EquirectToFaces(rgb, w, h, size, faces);
  return SPTR_OK;
}

int sptr_host_pack_tiles(const uint8_t* rgb, int32_t W, int32_t H, int32_t G, int32_t R, uint32_t* tiles) {
  if (!rgb || !tiles || W <= 0 || H <= 0 || G <= 0 || R < 0 || R >= G) return SPTR_ERR_INVALID;
  const uint32_t n = sptr::shard_tiles(W, H, G, R) * 1024u;
  for (uint32_t l = 0; l < n; ++l) {
    int x, y;
    if (!sptr::shard_pixel(W, H, G, R, l, x, y)) {
      tiles[l] = 0u;
      continue;
    }
    const uint8_t* p = rgb + ((size_t)y * W + x) * 3;
    tiles[l] = uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | 0xFF000000u;
  }
  return SPTR_OK;
}

int sptr_host_unpack_tiles(const uint32_t* g, int32_t G, uint32_t tpr, int32_t W, int32_t H, uint8_t* rgb) {
  if (!g || !rgb || W <= 0 || H <= 0 || G <= 0) return SPTR_ERR_INVALID;
  if ((uint64_t)tpr * (uint64_t)G < (uint64_t)sptr::tiles_total(W, H)) return SPTR_ERR_INVALID;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint32_t r, l;
      sptr::pixel_shard(W, G, x, y, r, l);
      const uint32_t px = g[(size_t)r * tpr * 1024u + l];
      uint8_t* o = rgb + ((size_t)y * W + x) * 3;
      o[0] = uint8_t(px & 0xFF);
      o[1] = uint8_t((px >> 8) & 0xFF);
      o[2] = uint8_t((px >> 16) & 0xFF);
    }
  return SPTR_OK;
}

int sptr_host_load_hdr(const char* path, float** rgb, int32_t* w, int32_t* h) {
  if (!path || !rgb || !w || !h) return SPTR_ERR_INVALID;
  std::vector<float> v;
  int ww = 0, hh = 0;
  if (!LoadRadianceHDR(path, v, ww, hh, nullptr)) return SPTR_ERR_INVALID;
  float* p = static_cast<float*>(std::malloc(v.size() * sizeof(float)));
  if (!p) return SPTR_ERR_OOM;
  std::memcpy(p, v.data(), v.size() * sizeof(float));
  *rgb = p;
  *w = ww;
  *h = hh;
  return SPTR_OK;
}

// The host twin of sptr_query_points: csrc/closest_point.h over every primitive.  The triangle records are built
// with the device's expressions (tri_record, tri_ng3 in csrc/lbvh_shared.h: e1 = v0 - v1, e2 = v2 - v0, the fmaf
// form of Ng), so a candidate here has the bits of the candidate there.
int sptr_host_query_points(const sptr_scene* sc, const sptr_point_query* q) {
  using namespace sptr;
  if (!sc || !q) return SPTR_ERR_INVALID;
  if (q->flags & ~uint32_t(SPTR_QUERY_SORT | SPTR_QUERY_NO_SORT)) return SPTR_ERR_INVALID;
  if ((q->flags & SPTR_QUERY_SORT) && (q->flags & SPTR_QUERY_NO_SORT)) return SPTR_ERR_INVALID;
  if (q->n > (1u << 28) || (q->n && !q->points)) return SPTR_ERR_INVALID;
  if (q->reserved[0] || q->reserved[1] || q->reserved[2] || q->reserved[3]) return SPTR_ERR_INVALID;
  struct Rec {
    vec3 v0, e1, e2, ng;
    uint32_t geom, prim;
    bool live;
  };
  std::vector<Rec> recs(sc->num_tris);
  uint32_t g = 0;
  for (uint32_t t = 0; t < sc->num_tris; ++t) {
    while (g + 1 < sc->num_tri_geoms && t >= sc->tri_geom_first[g + 1]) ++g;
    const uint32_t* ix = sc->indices + size_t(t) * 3;
    const float *a = sc->positions + size_t(ix[0]) * 3, *b = sc->positions + size_t(ix[1]) * 3,
                *c = sc->positions + size_t(ix[2]) * 3;
    Rec& r = recs[t];
    r.v0 = v3(a[0], a[1], a[2]);
    r.e1 = r.v0 - v3(b[0], b[1], b[2]);
    r.e2 = v3(c[0], c[1], c[2]) - r.v0;
    r.ng = v3(__builtin_fmaf(r.e2.y, r.e1.z, -(r.e2.z * r.e1.y)), __builtin_fmaf(r.e2.z, r.e1.x, -(r.e2.x * r.e1.z)),
              __builtin_fmaf(r.e2.x, r.e1.y, -(r.e2.y * r.e1.x)));
    r.geom = g;
    r.prim = t - (sc->num_tri_geoms ? sc->tri_geom_first[g] : 0u);
    r.live = cp_triangle_live(r.ng);
  }
  const float inf = __builtin_huge_valf();
  for (uint32_t i = 0; i < q->n; ++i) {
    const float* pp = q->points + size_t(i) * 4;
    const vec3 p = v3(pp[0], pp[1], pp[2]);
    float bd2 = pp[3] * pp[3];
    uint32_t bg = 0xFFFFFFFFu, bp = 0xFFFFFFFFu;
    int64_t bt = -1, bs = -1;
    if (cp_point_valid(p, pp[3])) {
      for (uint32_t t = 0; t < sc->num_tris; ++t) {
        const Rec& r = recs[t];
        if (!r.live) continue;
        const float d2 = cp_triangle(r.v0, r.e1, r.e2, p).d2;
        if (d2 <= bd2 && cp_key_less(d2, r.geom, r.prim, bd2, bg, bp)) {
          bd2 = d2;
          bg = r.geom;
          bp = r.prim;
          bt = t;
          bs = -1;
        }
      }
      for (uint32_t s = 0; s < sc->num_spheres; ++s) {
        const float* sp = sc->spheres + size_t(s) * 4;
        const float d2 = cp_sphere_d2(v3(sp[0], sp[1], sp[2]), sp[3], p);
        if (d2 <= bd2 && cp_key_less(d2, sc->num_tri_geoms + s, 0u, bd2, bg, bp)) {
          bd2 = d2;
          bg = sc->num_tri_geoms + s;
          bp = 0u;
          bs = s;
          bt = -1;
        }
      }
    }
    vec3 pt = v3(0.0f, 0.0f, 0.0f), ng = pt;
    float u = 0.0f, v = 0.0f, d2 = inf;
    if (bt >= 0) {
      const Rec& r = recs[size_t(bt)];
      const CpCand c = cp_triangle(r.v0, r.e1, r.e2, p);
      d2 = c.d2;
      pt = c.q;
      u = c.u;
      v = c.v;
      ng = r.ng;
    } else if (bs >= 0) {
      const float* sp = sc->spheres + size_t(bs) * 4;
      const CpCand c = cp_sphere(v3(sp[0], sp[1], sp[2]), sp[3], p, ng);
      d2 = c.d2;
      pt = c.q;
    }
    if (q->geom) q->geom[i] = bg;
    if (q->prim) q->prim[i] = bp;
    if (q->dist2) q->dist2[i] = d2;
    if (q->dist) q->dist[i] = sq_root(d2);
    if (q->point) {
      q->point[size_t(i) * 3 + 0] = pt.x;
      q->point[size_t(i) * 3 + 1] = pt.y;
      q->point[size_t(i) * 3 + 2] = pt.z;
    }
    if (q->uv) {
      q->uv[size_t(i) * 2 + 0] = u;
      q->uv[size_t(i) * 2 + 1] = v;
    }
    if (q->ng) {
      q->ng[size_t(i) * 3 + 0] = ng.x;
      q->ng[size_t(i) * 3 + 1] = ng.y;
      q->ng[size_t(i) * 3 + 2] = ng.z;
    }
  }
  return SPTR_OK;
}

void sptr_host_free(void* p) { std::free(p); }

}  // extern "C"
