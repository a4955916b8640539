// The host builders' scene images (csrc/rtow_bvh.h, rtow_bvh4.h, rtow_grid.h) for one scene, written to files, CPU
// only (tests/test_accel_images_host.py checks them with tests/accel_images.py).  The per-primitive records, leaf
// sizes and leaf order are those of rtow_scene.cpp's upload with the host builder; compile with -ffp-contract=off.
//
//   dump_host_images IN OUTDIR
//   IN: int32 ns, nm, nt, n_mats; double cam[3]; double sphere[ns][4], moving[nm][8], triangle[nt][9];
//       int32 material index per primitive (class-major); material records [n_mats][48 bytes]
//   OUTDIR/image0.bin (BVH), image1.bin (grid; empty when the scene does not suit one), image4.bin + image5.bin (4-wide
//   image with 128-byte nodes and its frame record) and image4h.bin + image5h.bin (64-byte nodes) for triangle meshes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracing-one-weekend_amd/csrc/rtow_bvh.h"
#include "../../raytracing-one-weekend_amd/csrc/rtow_bvh4.h"
#include "../../raytracing-one-weekend_amd/csrc/rtow_grid.h"
#include "../../raytracing-one-weekend_amd/csrc/rtow_scene_records.h"

static bool put(const std::string &path, const void *p, size_t n) {
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = n == 0 || std::fwrite(p, 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}

static void frame(const rtow::Bvh4Image &img, unsigned char out[48]) {
  std::memset(out, 0, 48);
  float is[3];
  for (int k = 0; k < 3; ++k) is[k] = (float)(1.0 / img.map_s[k]);  // rtow_scene.cpp bvh4_set_frame: DevScene::b4_is
  const uint32_t half = img.half ? 1u : 0u;
  std::memcpy(out, img.map_c, 24);
  std::memcpy(out + 24, is, 12);
  std::memcpy(out + 36, &half, 4);
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t cnt[4];
  double cam[3];
  if (std::fread(cnt, 4, 4, f) != 4 || std::fread(cam, 8, 3, f) != 3) return 4;
  const int ns = cnt[0], nm = cnt[1], nt = cnt[2], nmat = cnt[3];
  std::vector<double> gs((size_t)ns * 4), gm((size_t)nm * 8), gt((size_t)nt * 9);
  std::vector<int32_t> pmat((size_t)ns + nm + nt);
  std::vector<unsigned char> mats((size_t)nmat * 48);
  if (std::fread(gs.data(), 8, gs.size(), f) != gs.size() || std::fread(gm.data(), 8, gm.size(), f) != gm.size() ||
      std::fread(gt.data(), 8, gt.size(), f) != gt.size() || std::fread(pmat.data(), 4, pmat.size(), f) != pmat.size() ||
      std::fread(mats.data(), 1, mats.size(), f) != mats.size())
    return 5;
  std::fclose(f);
  // records: those of a scene upload (csrc/rtow_scene_records.h)
  rtow::SceneRecords rec;
  rtow::geometry_records(gs.data(), ns, gm.data(), nm, gt.data(), nt, rec);
  const std::vector<double> &sph = rec.sph, &sph_r = rec.sph_r, &mov = rec.mov, &tri = rec.tri;
  const std::string out = argv[2];
  const bool mesh = ns == 0 && nm == 0 && nt > 0;
  rtow::HostBvh bvh;
  rtow::build_bvh(sph, sph_r, mov, tri, bvh, mesh ? 2 : 4, mesh ? 1.5 : 0.0, 0.0, 1.0);
  const std::vector<int32_t> prim_order = bvh.prim;
  rtow::SceneImage img;
  if (mesh) {  // leaf order (rtow_scene.cpp: triangle meshes with the host builder)
    std::vector<double> tri_img(tri.size());
    std::vector<int32_t> pmat_img(pmat.size());
    for (size_t sl = 0; sl < bvh.prim.size(); ++sl) {
      std::memcpy(&tri_img[sl * 12], &tri[(size_t)bvh.prim[sl] * 12], 96);
      pmat_img[sl] = pmat[bvh.prim[sl]];
      bvh.prim[sl] = (int32_t)sl;
    }
    rtow::make_scene_image(bvh, sph, mov, tri_img, cam, img, pmat_img, mats);
  } else {
    rtow::make_scene_image(bvh, sph, mov, tri, cam, img, pmat, mats);
  }
  if (!rtow::validate_scene_image(img, ns + nm + nt)) return 6;
  if (!put(out + "/image0.bin", img.blob.data(), img.blob.size())) return 7;
  rtow::GridImage gimg;
  if (nt <= 8192) rtow::build_grid_image(sph, sph_r, mov, tri, cam, gimg, 1.0, 4.0, 0.0, 1.0, pmat, mats);
  if (!put(out + "/image1.bin", gimg.blob.data(), gimg.ok ? gimg.blob.size() : 0)) return 8;
  if (mesh) {
    bvh.prim = prim_order;
    for (int half = 0; half < 2; ++half) {
      rtow::Bvh4Image img4;
      rtow::make_bvh4_image(bvh, tri, pmat, mats, cam, img4, half != 0);
      if (!rtow::validate_bvh4_image(img4, (size_t)nt)) return 9;
      unsigned char fr[48];
      frame(img4, fr);
      const std::string sfx = half ? "h.bin" : ".bin";
      if (!put(out + "/image4" + sfx, img4.blob.data(), img4.blob.size()) || !put(out + "/image5" + sfx, fr, 48)) return 10;
    }
  }
  return 0;
}
