// prim_mat_table.h — the per-primitive material table of an LDS-staged scene, for host and device.
//
// Shading a hit needs the material index of the primitive that was hit: geom_mat[tri_geom[slot]] for a triangle
// slot, geom_mat[sph_geom[slot]] for a sphere slot, two dependent loads.  The table holds that value per slot, so
// the shading reads it with one load that depends on the hit's reference alone:
//   entry i,              i < num_tris : the material of triangle slot i
//   entry num_tris + j,   j < num_sph  : the material of sphere slot j
// It is padded with zeros to whole 16 bytes (it is copied to LDS in 16-byte words).
//
// The fused bounce kernels stage it in their dynamic LDS behind the scene (SceneView::lds_bytes) and ahead of the
// segment offsets.  Its bytes are no part of lds_bytes or of the staging threshold: a scene is staged exactly
// when it was before, and a table that does not fit into the same kLdsSceneBytes beside its scene stays in
// global memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SPTR_PM __host__ __device__ __forceinline__
#else
#define SPTR_PM inline
#endif

namespace sptr {

// entries of the table
SPTR_PM uint32_t prim_mat_entries(uint32_t num_tris, uint32_t num_sph) { return num_tris + num_sph; }
// its size, padded to 16 bytes
SPTR_PM uint32_t prim_mat_bytes(uint32_t num_tris, uint32_t num_sph) {
  return (prim_mat_entries(num_tris, num_sph) * 4u + 15u) / 16u * 16u;
}
// entry of a hit: idx is the triangle or sphere slot
SPTR_PM uint32_t prim_mat_slot(uint32_t num_tris, bool sphere, uint32_t idx) { return sphere ? num_tris + idx : idx; }
// entry i of the table (i < prim_mat_bytes / 4): the padding is 0
SPTR_PM uint32_t prim_mat_entry(const uint32_t* tri_geom, const uint32_t* sph_geom, const uint32_t* geom_mat,
                                uint32_t num_tris, uint32_t num_sph, uint32_t i) {
  if (i < num_tris) return geom_mat[tri_geom[i]];
  if (i < num_tris + num_sph) return geom_mat[sph_geom[i - num_tris]];
  return 0u;
}
// LDS bytes the table takes beside a staged scene of scene_lds_bytes (0: not staged) under the limit `cap`
// (kLdsSceneBytes); 0: it stays in global memory
SPTR_PM uint32_t prim_mat_lds_bytes(uint32_t scene_lds_bytes, uint32_t num_tris, uint32_t num_sph, uint32_t cap) {
  const uint32_t tb = prim_mat_bytes(num_tris, num_sph);
  if (scene_lds_bytes == 0u || prim_mat_entries(num_tris, num_sph) == 0u) return 0u;
  return scene_lds_bytes + tb <= cap ? tb : 0u;
}

}  // namespace sptr
