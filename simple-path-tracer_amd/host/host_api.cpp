// host_api.cpp — C ABI access to the host-side scene layer (sptr_host_* in include/sptr_hip.h), so
// foreign callers (ctypes harness, CLI) build scenes, cameras and material tables with exactly the
// C++ code the HipBackend uses.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/closest_point.h"
#include "../csrc/pseudonormal.h"
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

// The host twin of the device's table build (kernels_signed.hip): csrc/pseudonormal.h's arithmetic, a stable sort
// where the device runs its stable radix sort, and every sum in the same order.
namespace {
struct PnTables {
  std::vector<float> pos;  // 9 per triangle: the corners
  std::vector<float> nv, ne;  // 9 per triangle each
  uint64_t counts[4] = {0, 0, 0, 0};
};
sptr::vec3 pn_corner(const PnTables& t, size_t c) { return sptr::v3(t.pos[3 * c], t.pos[3 * c + 1], t.pos[3 * c + 2]); }

void pn_build(const sptr_scene* sc, PnTables& T) {
  using namespace sptr;
  const size_t nt = sc->num_tris, nc = nt * 3;
  T.pos.assign(nc * 3, 0.0f);
  T.nv.assign(nc * 3, 0.0f);
  T.ne.assign(nc * 3, 0.0f);
  std::vector<uint32_t> geom(nt, 0u);
  std::vector<uint8_t> live(nt, 0);
  std::vector<vec3> nhat(nt), contrib(nc);
  uint32_t g = 0;
  for (size_t t = 0; t < nt; ++t) {
    while (g + 1 < sc->num_tri_geoms && t >= sc->tri_geom_first[g + 1]) ++g;
    geom[t] = g;
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) T.pos[(3 * t + k) * 3 + a] = sc->positions[size_t(sc->indices[3 * t + k]) * 3 + a];
    const vec3 v0 = pn_corner(T, 3 * t), v1 = pn_corner(T, 3 * t + 1), v2 = pn_corner(T, 3 * t + 2);
    const vec3 ng = pn_tri_ng(v0, v1, v2);
    live[t] = cp_triangle_live(ng);
    if (!live[t]) continue;
    nhat[t] = pn_unit_normal(ng);
    for (uint32_t k = 0; k < 3; ++k) contrib[3 * t + k] = nhat[t] * pn_corner_angle(v0, v1, v2, k);
  }
  // welding: live corners by (geom, x, y, z) keys, stable, then runs of equal positions
  std::vector<uint32_t> order;
  for (size_t c = 0; c < nc; ++c)
    if (live[c / 3]) order.push_back(uint32_t(c));
  auto key = [&](uint32_t c, uint64_t& hi, uint64_t& lo) {
    hi = (uint64_t(geom[c / 3]) << 32) | pn_pos_bits(T.pos[3 * size_t(c)]);
    lo = (uint64_t(pn_pos_bits(T.pos[3 * size_t(c) + 1])) << 32) | pn_pos_bits(T.pos[3 * size_t(c) + 2]);
  };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    uint64_t ah, al, bh, bl;
    key(a, ah, al);
    key(b, bh, bl);
    return ah < bh || (ah == bh && al < bl);
  });
  std::vector<uint32_t> wid(nc, 0xFFFFFFFFu);
  uint32_t nw = 0;
  for (size_t j = 0; j < order.size();) {
    size_t e = j + 1;
    while (e < order.size() && geom[order[e] / 3] == geom[order[e - 1] / 3] &&
           pn_same_pos(pn_corner(T, order[e]), pn_corner(T, order[e - 1])))
      ++e;
    vec3 sum = v3(0.0f, 0.0f, 0.0f);
    for (size_t i = j; i < e; ++i)
      if (pn_finite3(nhat[order[i] / 3])) sum = sum + contrib[order[i]];
    for (size_t i = j; i < e; ++i) {
      wid[order[i]] = nw;
      T.nv[3 * size_t(order[i])] = sum.x;
      T.nv[3 * size_t(order[i]) + 1] = sum.y;
      T.nv[3 * size_t(order[i]) + 2] = sum.z;
    }
    ++nw;
    j = e;
  }
  T.counts[0] = nw;
  // edges: slots 3t + k by the pair of welded ids, stable
  std::vector<uint32_t> eorder;
  std::vector<uint64_t> ekey(nc, kPnDeadKey);
  for (size_t t = 0; t < nt; ++t)
    if (live[t])
      for (uint32_t k = 0; k < 3; ++k) {
        ekey[3 * t + k] = pn_edge_key(wid[3 * t + pn_edge_lo(k)], wid[3 * t + pn_edge_hi(k)]);
        if (ekey[3 * t + k] != kPnDeadKey) eorder.push_back(uint32_t(3 * t + k));
      }
  std::stable_sort(eorder.begin(), eorder.end(), [&](uint32_t a, uint32_t b) { return ekey[a] < ekey[b]; });
  for (size_t j = 0; j < eorder.size();) {
    size_t e = j + 1;
    while (e < eorder.size() && ekey[eorder[e]] == ekey[eorder[j]]) ++e;
    vec3 sum = v3(0.0f, 0.0f, 0.0f);
    uint32_t fwd = 0, bwd = 0;
    for (size_t i = j; i < e; ++i) {
      const uint32_t s = eorder[i], t = s / 3, k = s % 3;
      if (pn_finite3(nhat[t])) sum = sum + nhat[t];
      if (pn_edge_forward(k, wid[3 * t + pn_edge_lo(k)], wid[3 * t + pn_edge_hi(k)])) ++fwd;
      else ++bwd;
    }
    for (size_t i = j; i < e; ++i) {
      T.ne[3 * size_t(eorder[i])] = sum.x;
      T.ne[3 * size_t(eorder[i]) + 1] = sum.y;
      T.ne[3 * size_t(eorder[i]) + 2] = sum.z;
    }
    ++T.counts[1];
    if (e - j == 1) ++T.counts[2];
    if (!(fwd == 1 && bwd == 1)) ++T.counts[3];
    j = e;
  }
}
}  // namespace

int sptr_host_pseudonormals(const sptr_scene* sc, float* nv, float* ne, uint64_t counts[4]) {
  if (!sc || (sc->num_tris && (!sc->indices || !sc->positions))) return SPTR_ERR_INVALID;
  if (sc->num_tris && sc->num_tri_geoms && !sc->tri_geom_first) return SPTR_ERR_INVALID;
  PnTables T;
  pn_build(sc, T);
  if (nv && !T.nv.empty()) std::memcpy(nv, T.nv.data(), T.nv.size() * 4);
  if (ne && !T.ne.empty()) std::memcpy(ne, T.ne.data(), T.ne.size() * 4);
  if (counts)
    for (int i = 0; i < 4; ++i) counts[i] = T.counts[i];
  return SPTR_OK;
}

// sptr_host_query_points, then the sign of each winner from the tables (pn_triangle_result, pn_sphere_result).
int sptr_host_query_signed_distance(const sptr_scene* sc, const sptr_signed_query* q) {
  using namespace sptr;
  if (!sc || !q) return SPTR_ERR_INVALID;
  if (q->reserved[0] || q->reserved[1] || q->reserved[2] || q->reserved[3]) return SPTR_ERR_INVALID;
  if (q->q.flags & ~uint32_t(SPTR_QUERY_SORT | SPTR_QUERY_NO_SORT | SPTR_SIGNED_FLIP_TRIANGLES)) return SPTR_ERR_INVALID;
  if (sc->num_tris && !sc->num_tri_geoms) return SPTR_ERR_INVALID;  // (no tables for triangles without a geometry)
  const bool flip = (q->q.flags & SPTR_SIGNED_FLIP_TRIANGLES) != 0u;
  sptr_point_query pq = q->q;
  pq.flags &= ~uint32_t(SPTR_SIGNED_FLIP_TRIANGLES);
  std::vector<uint32_t> geom, prim;
  if (!pq.geom) {
    geom.resize(pq.n ? pq.n : 1u);
    pq.geom = geom.data();
  }
  if (!pq.prim) {
    prim.resize(pq.n ? pq.n : 1u);
    pq.prim = prim.data();
  }
  const int rc = sptr_host_query_points(sc, &pq);
  if (rc != SPTR_OK) return rc;
  PnTables T;
  pn_build(sc, T);
  const float inf = __builtin_huge_valf();
  for (uint32_t i = 0; i < pq.n; ++i) {
    const float* pp = pq.points + size_t(i) * 4;
    const vec3 p = v3(pp[0], pp[1], pp[2]);
    const uint32_t g = pq.geom[i];
    float sd = inf;
    vec3 n = v3(0.0f, 0.0f, 0.0f);
    uint32_t f = kCpMiss;
    if (g != 0xFFFFFFFFu && g < sc->num_tri_geoms) {
      const size_t t = size_t(sc->tri_geom_first[g]) + pq.prim[i];
      sd = pn_triangle_result(pn_corner(T, 3 * t), pn_corner(T, 3 * t + 1), pn_corner(T, 3 * t + 2), &T.nv[9 * t], &T.ne[9 * t], p,
                              flip, n, f);
    } else if (g != 0xFFFFFFFFu) {
      const float* sp = sc->spheres + size_t(g - sc->num_tri_geoms) * 4;
      sd = pn_sphere_result(v3(sp[0], sp[1], sp[2]), sp[3], p, n);
      f = kCpSphere;
    }
    if (q->signed_dist) q->signed_dist[i] = sd;
    if (q->normal) {
      q->normal[size_t(i) * 3 + 0] = n.x;
      q->normal[size_t(i) * 3 + 1] = n.y;
      q->normal[size_t(i) * 3 + 2] = n.z;
    }
    if (q->feature) q->feature[i] = f;
  }
  return SPTR_OK;
}

void sptr_host_free(void* p) { std::free(p); }

}  // extern "C"
