// walk_consts_check.cpp — the host derivation of the GRID walk's constants (csrc/rtow_walk_consts.h, the block the
// specialised trace kernels read instead of the image header) against the kernel's own formulas (rtow_trace_grid.h, the
// generic walk), evaluated here independently: CPU only, driven by tests/test_walk_consts_host.py.
//
//   walk_consts_check [IMAGE...]
//
// Every IMAGE is a grid image as the builders write it (rtow_grid.h; its first 64 bytes are the header).  Besides those
// the program checks headers it makes itself by the rounding rules of grid_header(): a grid with three layers in y, a
// grid far from the origin, one cell per axis, 128 cells per axis, and a mixed one.  Per case it prints
//   "<name>: n <nx> <ny> <nz> h <hx> <hy> <hz> ok|BAD"
// and at the end "<cases> cases, <mismatches> mismatches"; exit 1 on a mismatch.
//
// The far planes must be the kernel's value BIT FOR BIT: v_fma_f32 rounds n * c + g once.  The reference here is that
// sum in binary128 — exact: an 8-bit integer times a 24-bit significand plus a 24-bit significand — rounded once to
// binary32; the separately rounded product-then-sum is computed too, to show that the cases tell the two apart.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracing-one-weekend_amd/csrc/rtow_grid.h"
#include "../../raytracing-one-weekend_amd/csrc/rtow_walk_consts.h"

// the layout the kernels rely on: the two-axis walk reads words 0-19, the 3D walk words 0-24
static_assert(offsetof(GridWalkConsts, gx) == 0 && offsetof(GridWalkConsts, hx) == 12 && offsetof(GridWalkConsts, cx) == 24 &&
                  offsetof(GridWalkConsts, icx) == 32 && offsetof(GridWalkConsts, nx) == 40 &&
                  offsetof(GridWalkConsts, neg_nx) == 52 && offsetof(GridWalkConsts, cells) == 56 &&
                  offsetof(GridWalkConsts, large_first) == 60 && offsetof(GridWalkConsts, n_large) == 64 &&
                  offsetof(GridWalkConsts, fat_stride) == 72 && offsetof(GridWalkConsts, ny) == 76 &&
                  offsetof(GridWalkConsts, cy) == 80 && offsetof(GridWalkConsts, neg_nxny) == 96,
              "GridWalkConsts layout");
static_assert(alignof(GridWalkConsts) == 64, "one wide load per 64-byte line");

namespace {

int g_cases = 0, g_bad = 0, g_fused_differs = 0;

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

float far_plane(int n, float c, float g) {  // n * c + g, rounded once
  const __float128 exact = (__float128)n * (__float128)c + (__float128)g;
  return (float)exact;
}

void check(const std::string &name, const unsigned char *h) {
  float hf[9];
  int32_t n[3];
  uint32_t hu[4];
  std::memcpy(hf, h, 36);
  std::memcpy(n, h + 36, 12);
  std::memcpy(hu, h + 48, 16);
  // section offsets by the rule of layout_grid_image (rtow_grid.h): header, cell words, ids
  const uint32_t off_cells = 64u;
  const uint32_t off_ids = 64u + (((uint32_t)n[0] * (uint32_t)n[1] * (uint32_t)n[2] * 4u + 15u) / 16u) * 16u;
  const GridWalkConsts w = make_grid_walk_consts(h, off_ids, off_cells);
  int bad = 0;
  auto same_f = [&](const char *what, float got, float want) {
    if (bits(got) != bits(want)) {
      std::fprintf(stderr, "%s: %s = %.9g (%08x), the kernel computes %.9g (%08x)\n", name.c_str(), what, got, bits(got),
                   want, bits(want));
      ++bad;
    }
  };
  auto same_i = [&](const char *what, long long got, long long want) {
    if (got != want) {
      std::fprintf(stderr, "%s: %s = %lld, the kernel computes %lld\n", name.c_str(), what, got, want);
      ++bad;
    }
  };
  // the kernel's header reads: gx..gz = hf[0..2], cx..cz = hf[3..5], icx..icz = hf[6..8]
  same_f("gx", w.gx, hf[0]), same_f("gy", w.gy, hf[1]), same_f("gz", w.gz, hf[2]);
  same_f("cx", w.cx, hf[3]), same_f("cy", w.cy, hf[4]), same_f("cz", w.cz, hf[5]);
  same_f("icx", w.icx, hf[6]), same_f("icy", w.icy, hf[7]), same_f("icz", w.icz, hf[8]);
  // hx = fmaf((float)nx, cx, gx) ...
  const float hx = far_plane(n[0], hf[3], hf[0]), hy = far_plane(n[1], hf[4], hf[1]), hz = far_plane(n[2], hf[5], hf[2]);
  same_f("hx", w.hx, hx), same_f("hy", w.hy, hy), same_f("hz", w.hz, hz);
  for (int k = 0; k < 3; ++k) {  // (what a product rounded on its own would give: not what the kernel computes)
    volatile float prod = (float)n[k] * hf[3 + k];
    volatile float two = prod + hf[k];
    if (bits(two) != bits(k == 0 ? hx : (k == 1 ? hy : hz))) ++g_fused_differs;
  }
  // c0 clamps to nx - 1, remx = nx - 1 - c0, incz = -nx or +-(nx * ny), idx = (c2 * ny + c1) * nx + c0
  same_i("nx", w.nx, n[0]), same_i("ny", w.ny, n[1]);
  same_i("nx - 1", w.nxm1, n[0] - 1), same_i("ny - 1", w.nym1, n[1] - 1), same_i("nz - 1", w.nzm1, n[2] - 1);
  same_i("-nx", w.neg_nx, -n[0]), same_i("nx * ny", w.nxny, n[0] * n[1]), same_i("-(nx * ny)", w.neg_nxny, -(n[0] * n[1]));
  // n_large = hi[12], lf = (off_large - off.ids) >> 2, off.fat = hi[14], off.fat_stride = hi[15]; cells = g_off_cells
  same_i("n_large", w.n_large, hu[0]), same_i("large_first", w.large_first, (hu[1] - off_ids) >> 2);
  same_i("fat", w.fat, hu[2]), same_i("fat_stride", w.fat_stride, hu[3]), same_i("cells", w.cells, off_cells);
  for (int k = 0; k < 7; ++k) same_i("pad", w.pad_[k], 0);
  std::printf("%s: n %d %d %d h %.9g %.9g %.9g %s\n", name.c_str(), n[0], n[1], n[2], w.hx, w.hy, w.hz, bad ? "BAD" : "ok");
  ++g_cases;
  g_bad += bad;
}

// a header by the rounding rules of grid_header() (rtow_grid.h) for given bounds and cell counts
void synthetic(const std::string &name, const double gmn[3], const double gmx[3], const int n[3], uint32_t n_large) {
  rtow::GridHeader hd;
  for (int k = 0; k < 3; ++k) {
    hd.n[k] = n[k];
    hd.gminf[k] = std::nextafterf((float)gmn[k], -INFINITY);
    hd.cellf[k] = std::nextafterf((float)((gmx[k] - (double)hd.gminf[k]) / n[k]), INFINITY);
    hd.invf[k] = 1.0f / hd.cellf[k];
  }
  const uint32_t ncell = (uint32_t)n[0] * (uint32_t)n[1] * (uint32_t)n[2];
  const uint32_t off_ids = 64u + ((ncell * 4u + 15u) / 16u) * 16u;
  const uint32_t total_small_ids = 3u * ncell + 5u;  // (any count: the large list starts behind the cells' ids)
  const uint32_t off_large = off_ids + 4u * total_small_ids;
  const uint32_t off_fat = off_ids + ((4u * (total_small_ids + n_large) + 15u) / 16u) * 16u;
  unsigned char h[64];
  rtow::write_grid_header(h, hd, n_large, off_large, off_fat, 48u);
  check(name, h);
}

}  // namespace

int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = std::fopen(argv[a], "rb");
    unsigned char h[64];
    if (!f || std::fread(h, 1, 64, f) != 64) {
      std::fprintf(stderr, "%s: no 64-byte header\n", argv[a]);
      return 2;
    }
    std::fclose(f);
    check(std::string("image") + std::to_string(a), h);
  }
  {
    const double lo[3] = {-5.2, 0.0, -5.2}, hi[3] = {5.2, 3.4, 5.2};
    const int n[3] = {11, 3, 11};
    synthetic("three_layers", lo, hi, n, 1);
  }
  {
    const double lo[3] = {99994.8, -0.7, -70005.2}, hi[3] = {100005.2, 1.3, -69994.8};
    const int n[3] = {35, 1, 35};
    synthetic("far_from_origin", lo, hi, n, 4);
    const int m[3] = {19, 7, 23};
    synthetic("far_from_origin_3d", lo, hi, m, 0);
  }
  {
    const double lo[3] = {-0.3, -0.3, -0.3}, hi[3] = {0.3, 0.3, 0.3};
    const int n[3] = {1, 1, 1};
    synthetic("one_cell", lo, hi, n, 0);
  }
  {
    const double lo[3] = {-11.3, -11.1, -10.9}, hi[3] = {12.7, 11.9, 13.3};
    const int n[3] = {128, 128, 128};
    synthetic("cells_128", lo, hi, n, 64);
    const int m[3] = {128, 1, 1};
    synthetic("cells_128_1_1", lo, hi, m, 2);
    const int q[3] = {1, 128, 37};
    synthetic("cells_1_128_37", lo, hi, q, 2);
  }
  std::printf("%d cases, %d mismatches, %d far planes where two roundings would differ\n", g_cases, g_bad, g_fused_differs);
  return g_bad ? 1 : 0;
}
