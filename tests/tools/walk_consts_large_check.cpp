// walk_consts_large_check.cpp — the large-list words of the GRID walk's constants block (csrc/rtow_walk_consts.h:
// large_rec, large_id, n_large_fast) as the host derives them from a grid image: CPU only, driven by
// tests/test_walk_consts_large_host.py, which compares them with its own reading of the image.
//
//   walk_consts_large_check IMAGE N_SPH
//
// IMAGE is a grid image as the builders write it (rtow_grid.h); N_SPH the static spheres of its scene.  The program
// derives the block the way rtow_scene.cpp's grid_resident does — make_grid_walk_consts from the header, fill_large_head
// from the first words of the large list — and prints
//   "n_large <n> large_first <i> n_large_fast <k> rec <r0> <r1> <r2> <r3> id <i0> <i1> <i2> <i3> size <bytes>"
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../raytracing-one-weekend_amd/csrc/rtow_walk_consts.h"

// the layout the kernels rely on (the block's own static_asserts name the same offsets): the head of the large list is
// one aligned run of eight words and the count behind it, in the block's third 64-byte line
static_assert(sizeof(GridWalkConsts) == 192 && alignof(GridWalkConsts) == 64, "three 64-byte lines");
static_assert(offsetof(GridWalkConsts, large_rec) == 128 && offsetof(GridWalkConsts, large_id) == 144 &&
                  offsetof(GridWalkConsts, n_large_fast) == 160,
              "GridWalkConsts: the large list's head");
static_assert(offsetof(GridWalkConsts, n_large) == 64 && offsetof(GridWalkConsts, neg_nxny) == 96, "words 0-24 stay");
static_assert(kWalkLargeFast == 4, "four entries");

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<unsigned char> img;
  unsigned char buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) img.insert(img.end(), buf, buf + n);
  std::fclose(f);
  if (img.size() < 64) return 4;
  const int n_sph = std::atoi(argv[2]);
  int32_t n[3];
  std::memcpy(n, img.data() + 36, 12);
  // section offsets by the rule of layout_grid_image (rtow_grid.h): header, cell words, ids, (fat lists,) records
  const uint32_t off_cells = 64u;
  const uint32_t off_ids = 64u + (((uint32_t)n[0] * (uint32_t)n[1] * (uint32_t)n[2] * 4u + 15u) / 16u) * 16u;
  GridWalkConsts w = make_grid_walk_consts(img.data(), off_ids, off_cells);
  uint32_t hu[4];
  std::memcpy(hu, img.data() + 48, 16);  // n_large, off_large, off_fat, fat_stride
  const uint32_t n_cell_ids = (hu[1] - off_ids) / 4u;
  const uint32_t off_sph = off_ids + ((4u * (n_cell_ids + hu[0]) + 15u) / 16u) * 16u + (hu[2] ? n_cell_ids * hu[3] : 0u);
  unsigned head[kWalkLargeFast] = {};
  const size_t cnt = w.n_large < kWalkLargeFast ? w.n_large : kWalkLargeFast;
  const size_t off_large = (size_t)off_ids + 4u * (size_t)w.large_first;
  if (off_large + 4 * cnt > img.size()) return 5;
  std::memcpy(head, img.data() + off_large, 4 * cnt);
  fill_large_head(w, head, n_sph, off_sph);
  for (int k = 0; k < 7; ++k)
    if (w.pad_[k] != 0 || w.pad2_[k] != 0) return 6;
  std::printf("n_large %u large_first %u n_large_fast %u rec %u %u %u %u id %u %u %u %u size %zu\n", w.n_large, w.large_first,
              w.n_large_fast, w.large_rec[0], w.large_rec[1], w.large_rec[2], w.large_rec[3], w.large_id[0], w.large_id[1],
              w.large_id[2], w.large_id[3], sizeof w);
  return 0;
}
