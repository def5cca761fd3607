// The per-primitive material table's arithmetic (csrc/prim_mat_table.h) on the CPU, driven by
// tests/test_prim_mat_table_cpu.py.  Input (text, argv[1]): num_tris num_sph num_geoms cap scene_lds_bytes, then
// tri_geom[num_tris], sph_geom[num_sph], geom_mat[num_geoms].  Output: line 1 the padded size in bytes and the
// LDS bytes beside the scene; line 2 every table word, padding included; line 3 the entry prim_mat_slot gives
// every triangle slot and then every sphere slot.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "prim_mat_table.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned nt, ns, ng, cap, scene;
  if (std::fscanf(f, "%u %u %u %u %u", &nt, &ns, &ng, &cap, &scene) != 5) return 2;
  std::vector<uint32_t> tg(nt), sg(ns), gm(ng);
  for (std::vector<uint32_t>* v : {&tg, &sg, &gm})
    for (uint32_t& x : *v) {
      unsigned t;
      if (std::fscanf(f, "%u", &t) != 1) return 2;
      x = t;
    }
  std::fclose(f);
  const uint32_t bytes = sptr::prim_mat_bytes(nt, ns);
  std::printf("%u %u\n", bytes, sptr::prim_mat_lds_bytes(scene, nt, ns, cap));
  for (uint32_t i = 0; i < bytes / 4u; ++i)
    std::printf("%u ", sptr::prim_mat_entry(tg.data(), sg.data(), gm.data(), nt, ns, i));
  std::printf("\n");
  for (uint32_t i = 0; i < nt; ++i) std::printf("%u ", sptr::prim_mat_slot(nt, false, i));
  for (uint32_t j = 0; j < ns; ++j) std::printf("%u ", sptr::prim_mat_slot(nt, true, j));
  std::printf("\n");
  return 0;
}
