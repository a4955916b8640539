// rtow_walk_consts.h — the per-scene constants of the uniform-grid walk (rtow_trace_grid.h) as one block of kernel
// arguments, derived on the host from the 64-byte header of the RESIDENT grid image (rtow_grid.h) and from nothing else:
// the builders, the image and DevScene stay as they are.  Plain C++ without includes, so that the host (rtow_capi.cpp),
// the kernels and a host test program (tests/tools/walk_consts_check.cpp) compile the very same derivation.
//
// Why a block: the specialised instantiations of the trace kernels used to read the header from the global copy of the
// image at every entry of the walk — six scalar loads of mixed width, single-word reloads where the SGPRs ran out — and to
// re-derive per-scene terms on the vector unit in every trip (the far planes: a conversion, a move and a fused
// multiply-add per axis).  The block is laid out in the order the walk consumes it: the two-axis walk of a grid with one
// layer in y takes its first 19 words (a 16-word scalar load and a short one, one wait), the 3D walk six more.  Words
// 32-40 hold the head of the image's large-primitive list (fill_large_head below): loaded with them, behind the same wait.
//
// Every term is the kernel's own expression on the same binary32 / 32-bit integer operands, so a walk that reads the
// block visits the cells the header-reading walk visits: hx is fmaf((float)nx, cx, gx) in binary32, ONE rounding, as
// v_fma_f32 computes it (__builtin_fmaf: never a separate multiply and add, whatever -ffp-contract says).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTOW_WALK_FN __host__ __device__ inline
#else
#define RTOW_WALK_FN inline
#endif

struct alignas(64) GridWalkConsts {
  // words 0-19: every walk (ny, word 19: the 3D walk only)
  float gx, gy, gz;           // near planes: the grid's minimum corner (header words 0-2)
  float hx, hy, hz;           // far planes: fmaf((float)n, c, g) per axis
  float cx, cz;               // cell sizes in x and z
  float icx, icz;             // their reciprocals as the header holds them
  int nx, nxm1, nzm1;         // cells in x; nx - 1, nz - 1 (clamps, remaining-cell counters)
  int neg_nx;                 // -nx: the index stride against z (two-axis walk), against y (3D walk)
  unsigned cells;             // byte offset of the cell words in the image
  unsigned large_first;       // the large-primitive list's first index in the id section: (off_large - off_ids) >> 2
  unsigned n_large;           // entries of that list
  unsigned fat, fat_stride;   // byte offset and stride of the fat cell lists (0: plain id lists)
  int ny;
  // words 20-24: the 3D walk only
  float cy, icy;
  int nym1;                   // ny - 1
  int nxny, neg_nxny;         // the index stride along z, both signs
  int pad_[7];
  // words 32-40: the head of the always-test (large-primitive) list, for the class instantiations (read by the class
  // with moving spheres; rtow_trace_grid.h says why the class of static spheres keeps its id reads).  The ids of that list
  // and the records they name are the same for every wave of every launch on a resident image: entry j < n_large_fast
  // is the static sphere large_id[j], whose 32-byte record sits at byte large_rec[j] of the image.  The walk tests
  // these entries from wave-uniform values — no read of the id section, no per-lane address arithmetic — and the rest
  // of the list (entries from n_large_fast on) the way the generic walk does.  n_large_fast is the number of LEADING
  // entries, four at most, that are static spheres; 0 for a block made without the id section (fill_large_head not
  // called): the whole list then goes the generic way.
  unsigned large_rec[4];
  unsigned large_id[4];
  unsigned n_large_fast;
  int pad2_[7];
};
static_assert(sizeof(GridWalkConsts) == 192, "three 64-byte lines");
// (the head of the list: one aligned run of eight words, read with one wide scalar load, and the count behind it)
static_assert(__builtin_offsetof(GridWalkConsts, large_rec) == 128 && __builtin_offsetof(GridWalkConsts, large_id) == 144 &&
                  __builtin_offsetof(GridWalkConsts, n_large_fast) == 160,
              "GridWalkConsts: the large list's head");
constexpr unsigned kWalkLargeFast = 4;  // entries of the large list the block can hold

// `header`: the 64 bytes at the start of the grid image (rtow_grid.h: f32 gmin[3], cell[3], inv_cell[3], i32 n[3], u32
// n_large, off_large, off_fat, fat_stride); off_ids / off_cells: the image's section offsets (DevScene::g_off_*).
RTOW_WALK_FN GridWalkConsts make_grid_walk_consts(const unsigned char *header, unsigned off_ids, unsigned off_cells) {
  float hf[9];
  int hi[3];
  unsigned hu[4];
  __builtin_memcpy(hf, header, 36);
  __builtin_memcpy(hi, header + 36, 12);
  __builtin_memcpy(hu, header + 48, 16);
  GridWalkConsts w{};
  w.gx = hf[0], w.gy = hf[1], w.gz = hf[2];
  w.hx = __builtin_fmaf((float)hi[0], hf[3], hf[0]);
  w.hy = __builtin_fmaf((float)hi[1], hf[4], hf[1]);
  w.hz = __builtin_fmaf((float)hi[2], hf[5], hf[2]);
  w.cx = hf[3], w.cy = hf[4], w.cz = hf[5];
  w.icx = hf[6], w.icy = hf[7], w.icz = hf[8];
  w.nx = hi[0], w.ny = hi[1];
  w.nxm1 = hi[0] - 1, w.nym1 = hi[1] - 1, w.nzm1 = hi[2] - 1;
  w.neg_nx = -hi[0];
  w.nxny = hi[0] * hi[1], w.neg_nxny = -(hi[0] * hi[1]);
  w.cells = off_cells;
  w.n_large = hu[0];
  w.large_first = (hu[1] - off_ids) >> 2;
  w.fat = hu[2], w.fat_stride = hu[3];
  return w;
}

// The head of the large list into `w`.  `large_ids`: the first min(n_large, kWalkLargeFast) words of the list as the
// image holds them (at header word 13, off_large); n_sph: static spheres of the scene (ids below it); off_sph: byte
// offset of the image's static-sphere records (32 bytes each).
RTOW_WALK_FN void fill_large_head(GridWalkConsts &w, const unsigned *large_ids, int n_sph, unsigned off_sph) {
  const unsigned n = w.n_large < kWalkLargeFast ? w.n_large : kWalkLargeFast;
  unsigned k = 0;
  for (; k < n && large_ids[k] < (unsigned)n_sph; ++k) {
    w.large_id[k] = large_ids[k];
    w.large_rec[k] = off_sph + 32u * large_ids[k];
  }
  w.n_large_fast = k;
}
