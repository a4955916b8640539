// rtow_scene.cpp — how a scene becomes resident: rtow_scene_upload, the lean upload of rtow_render, rtow_scene_refit,
// and the diagnostics that read the resident images back (rtow_build_info, rtow_refit_info, rtow_debug_image).
//
// Both entry points are a sequence of stages ("Scene upload and refit"), and every fact about what is
// resident has ONE writer, called by the upload and the refit, by the host and the device builder alike:
// bvh4_resident / bvh4_set_frame, grid_resident, image32_resident, camera_resident, host_scene_copy,
// invalidate_resident; copy_record_sections is the one device-to-device scatter of the record arrays into an image.
// Built with -ffp-contract=off like every translation unit that computes records.

#include "rtow_ctx.h"
#include "rtow_scene_records.h"

namespace rtow {  // csrc/rtow_build.hip
int lbvh_build(const double *sph, const double *sph_r, const double *mov, const double *tri, int ns, int nm,
               int nt, double time0, double time1, const double cam_origin[3], int leaf_max, void *stream,
               void **handle, int *n_nodes, int ploc_radius);
int lbvh_emit(void *handle, int leaf_max, unsigned char *blob_dev, uint32_t off_ids, int n_nodes, void *stream);
int lbvh_bvh4_collapse(void *handle, int leaf_max, void *stream, int *n_nodes, int *depth, float root_box[6]);
int lbvh_bvh4_emit(void *handle, unsigned char *blob_dev, int half, const double map_c[3], const double map_s[3],
                   uint32_t off_tri, uint32_t off_pmat, const double *tri, const int32_t *prim_mat, void *stream);
// csrc/rtow_build_grid.hip
struct GridBuildBounds {
  double gmn[3], gmx[3];
  double scale_prims;
  int32_t n_small, n_large;
};
int grid_build_phase1(const double *sph, const double *sph_r, const double *mov, const double *tri, int ns, int nm,
                      int nt, double time0, double time1, double large_ratio, void *stream, void **handle,
                      GridBuildBounds *out);
int grid_build_phase2(void *handle, const float gminf[3], const float cellf[3], const int32_t n[3], double pad,
                      void *stream, unsigned long long *total_ids, unsigned long long *max_list);
int grid_build_phase3(void *handle, const float gminf[3], const float cellf[3], const int32_t n[3], double pad,
                      unsigned long long total_ids, unsigned char *blob_dev, uint32_t off_cells, uint32_t off_ids,
                      void *stream, const double *sph, uint32_t off_fat, const double *mov, int ns, uint32_t fat_stride);
// csrc/rtow_refit.hip (rtow_scene_refit): 0, or 1 when a launch failed
int refit_records(const double *g_sph, const double *g_mov, const double *g_tri, int ns, int nm, int nt, double *sph,
                  double *sph_r, double *mov, double *tri, double *tri16, void *stream);
int refit_prim_boxes(const double *sph, const double *sph_r, const double *mov, const double *tri, int ns, int nm, int nt,
                     double time0, double time1, double *pbox, void *stream);
int refit_tri_section(int nt, const double *tri, const int32_t *pmat_tri, const int32_t *map, unsigned char *dst,
                      uint32_t off_tri, uint32_t off_pmat, int f32, void *stream);
int refit_spheres32(int ns, int nm, const double *sph, const double *mov, unsigned char *dst, uint32_t off_sph32,
                    uint32_t off_mov32, void *stream);
int refit_bvh2_links(const unsigned char *blob, int n_nodes, int32_t *parent, void *stream);
int refit_bvh2(unsigned char *blob, int n_nodes, uint32_t off_ids, int n_ids, const int32_t *map, int cls_base,
               const double *pbox, const int32_t *parent, uint32_t *flags, double *nbox, double *partials, int emit,
               const double cam_origin[3], double *area_out, void *stream);
int refit_bvh4_links(const unsigned char *blob4, int n4, uint32_t node_bytes, uint32_t child_off, int32_t *parent,
                     int32_t *need, void *stream);
int refit_bvh4(unsigned char *blob4, int n4, uint32_t node_bytes, uint32_t child_off, int half, int n_rec, const int32_t *map,
               int cls_base, const double *pbox, const int32_t *parent, const int32_t *need, uint32_t *flags, double *nbox,
               double *sbox, const double cam_origin[3], double *frame, void *stream);

}  // namespace rtow

namespace {

// The arena of the upload or refit in progress on this thread, for upload() and h2d_block(); rewound first (behind the
// caller's device synchronisation: nothing reads the staging of the call before any more)
thread_local PinnedArena *g_arena = nullptr;
struct ArenaScope {
  explicit ArenaScope(PinnedArena *a) {
    a->used = 0;
    g_arena = a;
  }
  ~ArenaScope() { g_arena = nullptr; }
};

}  // namespace

int rtow::h2d_block(void *dst, const void *src, size_t n) {
  PinnedArena *a = g_arena;
  const size_t at = a ? (a->used + 255) / 256 * 256 : 0;
  if (a && a->p && at + n <= a->cap) {
    std::memcpy(a->p + at, src, n);
    a->used = at + n;
    HIPCHK(hipMemcpyAsync(dst, a->p + at, n, hipMemcpyHostToDevice, nullptr));
  } else {
    HIPCHK(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
  }
  return RTOW_OK;
}

namespace {

// Scene image of the f32 build, derived from a binary64 image: the same prefix (nodes or
// header+cells, then ids — everything before the sphere records), the binary64 sphere and moving
// records (large-primitive list, BVH kernel, shading), binary32 triangle records (the only
// triangle section), binary32 sphere and moving records (grid cells), material indices, materials.
struct Image32 {
  std::vector<unsigned char> blob;  // prefix left zeroed when `prefix` is NULL (filled on the device)
  uint32_t off_sph = 0, off_mov = 0, off_tri = 0, off_sph32 = 0, off_mov32 = 0, off_pmat = 0, off_mats = 0;
};
// the section offsets of that image; returns its size
size_t layout_image32(uint32_t prefix_bytes, size_t ns, size_t nm, size_t nt, size_t n_pmat, size_t mats_bytes, Image32 &out) {
  auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
  out.off_sph = prefix_bytes;
  out.off_mov = (uint32_t)(out.off_sph + ns * 32);
  out.off_tri = (uint32_t)(out.off_mov + nm * 64);
  out.off_sph32 = (uint32_t)up16(out.off_tri + nt * 48);
  out.off_mov32 = (uint32_t)(out.off_sph32 + ns * 16);
  out.off_pmat = (uint32_t)up16(out.off_mov32 + nm * 32);
  out.off_mats = (uint32_t)up16(out.off_pmat + n_pmat * 4);
  return up16(out.off_mats + mats_bytes);
}
void make_image32(const unsigned char *prefix, uint32_t prefix_bytes, const std::vector<double> &sph,
                  const std::vector<double> &mov, const std::vector<double> &tri, const std::vector<int32_t> &pmat,
                  const std::vector<unsigned char> &mats_bytes, Image32 &out) {
  const size_t ns = sph.size() / 4, nm = mov.size() / 8, nt = tri.size() / 12;
  out.blob.assign(layout_image32(prefix_bytes, ns, nm, nt, pmat.size(), mats_bytes.size(), out), 0);
  unsigned char *b = out.blob.data();
  if (prefix) std::memcpy(b, prefix, prefix_bytes);
  if (ns) std::memcpy(b + out.off_sph, sph.data(), ns * 32);
  if (nm) std::memcpy(b + out.off_mov, mov.data(), nm * 64);
  float *t32 = reinterpret_cast<float *>(b + out.off_tri);
  for (size_t i = 0; i < nt * 12; ++i) t32[i] = (float)tri[i];  // A e1 e2 n, 12 floats per triangle
  float *s32 = reinterpret_cast<float *>(b + out.off_sph32);
  for (size_t i = 0; i < ns * 4; ++i) s32[i] = (float)sph[i];    // cx cy cz copysign(r*r, r)
  float *m32 = reinterpret_cast<float *>(b + out.off_mov32);
  for (size_t i = 0; i < nm; ++i) {                              // c0xyz dx | dy dz copysign(r*r, r) 0
    for (int k = 0; k < 7; ++k) m32[i * 8 + k] = (float)mov[i * 8 + k];
    m32[i * 8 + 7] = 0.0f;
  }
  if (!pmat.empty()) std::memcpy(b + out.off_pmat, pmat.data(), pmat.size() * 4);
  if (!mats_bytes.empty()) std::memcpy(b + out.off_mats, mats_bytes.data(), mats_bytes.size());
}

}  // namespace

static void camera_record(const rtow_camera_t &k, rtow::DevCamera &dc) {
  for (int i = 0; i < 3; ++i) {
    dc.origin[i] = k.origin[i];
    dc.u[i] = k.u[i];
    dc.v[i] = k.v[i];
    dc.horizontal[i] = k.horizontal[i];
    dc.vertical[i] = k.vertical[i];
    dc.llc[i] = k.lower_left_corner[i];
  }
  dc.lens_radius = k.lens_radius;
  dc.t0 = k.t0;
  dc.t1 = k.t1;
}

// Material index per primitive (class-major) and the device material records
static void scene_materials(const rtow_scene_t *s, rtow::SceneRecords &rec) {
  const int ns = s->n_spheres, nm = s->n_moving, nt = s->n_triangles;
  std::vector<int32_t> &pmat = rec.pmat;
  pmat.resize((size_t)ns + nm + nt);
  for (int i = 0; i < ns; ++i) pmat[i] = s->sphere_mat[i];
  for (int i = 0; i < nm; ++i) pmat[(size_t)ns + i] = s->moving_mat[i];
  for (int i = 0; i < nt; ++i) pmat[(size_t)ns + nm + i] = s->triangle_mat[i];
  rec.mats_bytes.resize((size_t)s->n_materials * sizeof(rtow::DevMaterial));
  for (int i = 0; i < s->n_materials; ++i) {
    const rtow_material_t &m = s->materials[i];
    rtow::DevMaterial d;
    std::memset(&d, 0, sizeof d);
    const bool diel = m.kind == RTOW_MAT_DIELECTRIC;  // attenuation {1,1,1}, common-model.cpp:61
    for (int k = 0; k < 3; ++k) d.att[k] = diel ? 1.0 : m.albedo[k];
    d.fuzz = m.kind == RTOW_MAT_LAMBERTIAN ? 0.0 : m.fuzz;
    d.ir = m.ir;
    d.kind = m.kind;
    std::memcpy(&rec.mats_bytes[(size_t)i * sizeof d], &d, sizeof d);
  }
}

// Everything the upload computes on the host before it builds anything (rtow_scene_records.h has the arithmetic)
static rtow::SceneRecords make_scene_records(const rtow_scene_t *s) {
  rtow::SceneRecords rec;
  rtow::geometry_records(s->sphere_geom, s->n_spheres, s->moving_geom, s->n_moving, s->triangle_geom, s->n_triangles, rec);
  scene_materials(s, rec);
  return rec;
}

// ---- one writer per residency fact ------------------------------------------------------------------------------------

// Where an image keeps the class-major record arrays (kSkip: not in this image, or written by a kernel of its own)
constexpr uint32_t kSkip = ~0u;
struct RecordOffsets {
  uint32_t sph, mov, tri, pmat, mats;
};
// The one device-to-device scatter of the resident arrays (c->sph, mov, tri, prim_mat, mats) into an image's sections
static int copy_record_sections(unsigned char *dst, const RecordOffsets &o, const rtow_ctx *c, int ns, int nm, int nt, int np,
                                size_t mats_n) {
  const struct {
    uint32_t off;
    const void *src;
    size_t n;
  } parts[] = {{o.sph, c->sph.p, (size_t)ns * 32}, {o.mov, c->mov.p, (size_t)nm * 64}, {o.tri, c->tri.p, (size_t)nt * 96},
               {o.pmat, c->prim_mat.p, (size_t)np * 4}, {o.mats, c->mats.p, mats_n}};
  for (const auto &p : parts)
    if (p.off != kSkip && p.n) HIPCHK(hipMemcpyAsync(dst + p.off, p.src, p.n, hipMemcpyDeviceToDevice, nullptr));
  return RTOW_OK;
}
static hipError_t d2d(void *dst, const void *src, size_t n) {
  return n ? hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, nullptr) : hipSuccess;
}

// The frame the 4-wide walk decodes binary16 planes in (world = c + h / s): a launch parameter, in ds and its f32 twin
static void bvh4_set_frame(rtow_ctx *c, const double map_c[3], const double map_s[3]) {
  for (rtow::DevScene *d : {&c->ds, &c->ds32})
    for (int k = 0; k < 3; ++k) {
      d->b4_c[k] = map_c[k];
      d->b4_is[k] = (float)(1.0 / map_s[k]);
    }
}

// "The 4-wide image in c->blob4 is resident" (img4.ok; `bytes`: its size), or "there is none": both builders.  Without
// one the ds.b4_* of an earlier image stay as they are, behind have_bvh4.
static void bvh4_resident(rtow_ctx *c, const rtow::Bvh4Image &img4, size_t bytes) {
  c->have_bvh4 = img4.ok;
  c->build_info.bvh4_nodes = img4.ok ? img4.n_nodes : 0;
  c->build_info.bvh4_image_bytes = img4.ok ? (int32_t)bytes : 0;
  c->build_info.bvh4_node_bytes = img4.ok ? (int32_t)img4.node_bytes() : 0;
  if (!img4.ok) return;
  c->bvh4_depth = img4.depth;
  c->ds.blob4 = (const unsigned char *)c->blob4.p;
  c->ds.blob4_bytes = (uint32_t)bytes;
  c->ds.b4_off_tri = img4.off_tri;
  c->ds.b4_off_pmat = img4.off_pmat;
  c->ds.b4_off_mats = img4.off_mats;
  c->ds.b4_half = img4.half ? 1u : 0u;
  bvh4_set_frame(c, img4.map_c, img4.map_s);
}

// "The grid image in c->gblob is resident" (gimg.ok), or "there is no grid": every upload and refit, host- or
// device-built.  What the context remembers of the image comes from its 64-byte header: n[1] == 1 selects the two-axis
// walk; the specialised trace kernels read the walk's constants from the block derived here instead of the header.
// The block also carries the head of the image's large-primitive list (fill_large_head): read from the image itself —
// the host builder's copy of it, or, for an image built on the device, the sixteen bytes at the list's offset copied
// back (a blocking copy behind the build kernels; only for an image the class kernels can run on: fat cell lists).
// n_sph: static spheres of the scene the image was built from.
static int grid_resident(rtow_ctx *c, const rtow::GridImage &gimg, int n_sph) {
  c->have_grid = gimg.ok;
  c->grid_fat_stride = (gimg.ok && gimg.off_fat) ? gimg.fat_stride : 0u;
  c->grid_ny = gimg.ok ? gimg.n[1] : 0;
  c->grid_walk = gimg.ok ? make_grid_walk_consts(gimg.header, gimg.off_ids, gimg.off_cells) : GridWalkConsts{};
  if (gimg.ok && c->grid_walk.n_large != 0u && gimg.off_fat != 0u) {
    uint32_t head[kWalkLargeFast] = {};
    const size_t n = std::min<size_t>(c->grid_walk.n_large, kWalkLargeFast) * sizeof(uint32_t);
    const size_t off_large = (size_t)gimg.off_ids + 4u * (size_t)c->grid_walk.large_first;
    if (gimg.blob.size() >= off_large + n)
      std::memcpy(head, gimg.blob.data() + off_large, n);
    else
      HIPCHK(hipMemcpy(head, (const unsigned char *)c->gblob.p + off_large, n, hipMemcpyDeviceToHost));
    fill_large_head(c->grid_walk, head, n_sph, gimg.off_sph);
  }
  c->gblob_bytes = gimg.ok ? (uint32_t)gimg.total_bytes : 0u;
  rtow::DevScene &ds = c->ds;
  ds.gblob = (const unsigned char *)c->gblob.p;
  ds.gblob_bytes = c->gblob_bytes;
  ds.g_off_sph = gimg.off_sph;
  ds.g_off_mov = gimg.off_mov;
  ds.g_off_tri = gimg.off_tri;
  ds.g_off_pmat = gimg.off_pmat;
  ds.g_off_mats = gimg.off_mats;
  for (rtow::DevScene *d : {&c->ds, &c->ds32}) {  // (the f32 build's grid image has the same header, cells and ids)
    d->g_off_cells = gimg.off_cells;
    d->g_off_ids = gimg.off_ids;
  }
  return RTOW_OK;
}

// The f32 build's image fields (ds32 is otherwise a copy of ds).  grid false: the BVH image, in c->blob32; true: the
// grid image, in c->gblob32, or none (im NULL).
static void image32_resident(rtow::DevScene &d32, bool grid, const Image32 *im, const void *dev, size_t bytes) {
  (grid ? d32.gblob : d32.blob) = im ? (const unsigned char *)dev : nullptr;
  (grid ? d32.gblob_bytes : d32.blob_bytes) = im ? (uint32_t)bytes : 0u;
  if (!im) return;
  (grid ? d32.g_off_sph : d32.off_sph) = im->off_sph;
  (grid ? d32.g_off_mov : d32.off_mov) = im->off_mov;
  (grid ? d32.g_off_tri : d32.off_tri) = im->off_tri;
  (grid ? d32.g_off_sph32 : d32.off_sph32) = im->off_sph32;
  (grid ? d32.g_off_mov32 : d32.off_mov32) = im->off_mov32;
  (grid ? d32.g_off_pmat : d32.off_pmat) = im->off_pmat;
  (grid ? d32.g_off_mats : d32.off_mats) = im->off_mats;
}

// Camera record, its device copy and (f32) the binary32 copy of its 21 values
static int camera_resident(rtow_ctx *c, const rtow_camera_t &cam, bool f32) {
  camera_record(cam, c->cam);
  int rc;
  if ((rc = c->cam_dev.ensure(sizeof c->cam)) || (rc = h2d_block(c->cam_dev.p, &c->cam, sizeof c->cam))) return rc;
  if (!f32) return RTOW_OK;
  const double *cd = reinterpret_cast<const double *>(&c->cam);
  float cam32[21];
  for (int i = 0; i < 21; ++i) cam32[i] = (float)cd[i];
  if ((rc = c->cam32_dev.ensure(sizeof cam32))) return rc;
  return h2d_block(c->cam32_dev.p, cam32, sizeof cam32);
}

// The host copy of the scene as uploaded (the reference tree and the tile classes are made from it).  with_order: also
// the insertion order, checked (an upload; a refit has checked that the order is the resident one's).
static int host_scene_copy(rtow_ctx *c, const rtow_scene_t *s, bool with_order) {
  rtow_ctx::HostSceneCopy &h = c->host_scene;
  h.sg.assign(s->sphere_geom, s->sphere_geom + 4 * (size_t)s->n_spheres);
  h.mg.assign(s->moving_geom, s->moving_geom + 8 * (size_t)s->n_moving);
  h.tg.assign(s->triangle_geom, s->triangle_geom + 9 * (size_t)s->n_triangles);
  h.cam = s->camera;
  if (!with_order) return RTOW_OK;
  h.have_order = s->prim_kind && s->prim_index;
  if (h.have_order) {
    for (int i = 0; i < s->n_prims; ++i) {
      const int k = s->prim_kind[i], ix = s->prim_index[i];
      const int cnt = k == RTOW_PRIM_SPHERE ? s->n_spheres : k == RTOW_PRIM_MOVING_SPHERE ? s->n_moving
                      : k == RTOW_PRIM_TRIANGLE ? s->n_triangles : -1;
      if (ix < 0 || ix >= cnt) return fail(RTOW_EINVAL, "prim_kind / prim_index entry %d out of range", i);
    }
    h.pk.assign(s->prim_kind, s->prim_kind + s->n_prims);
    h.pi.assign(s->prim_index, s->prim_index + s->n_prims);
  } else {
    h.pk.clear();
    h.pi.clear();
  }
  return RTOW_OK;
}

// What is derived from the resident scene and kept outside its images: dropped at the top of an upload and at the
// bottom of a refit.
enum class Invalidate { Upload, Refit };
static void invalidate_resident(rtow_ctx *c, Invalidate what) {
  c->scene_gen++;  // (the tile table belongs to the old scene; a refit: geometry may have moved into tiles that were empty)
  c->have_rtree = false;  // (the reference tree is rebuilt from the host copy at its next use)
  for (auto &o : c->occ) o[0] = o[1] = o[2] = o[3] = o[4] = 0;  // (image sizes decide the launch shapes)
  c->q_map_ok[1] = c->q_map_ok[2] = false;  // (the ray queries' id tables of the leaf-ordered images; after a refit they
                                            // are rebuilt from the refit's slot maps)
  if (what == Invalidate::Refit) return;
  // A refit keeps three things an upload drops: table 0 (class-major ids do not move), what its first call derived
  // from the images as uploaded (rf), and build_info.ref_tree_* (the tree last built, until the next one is).
  c->q_map_ok[0] = false;
  c->rf.ready = false;
  c->rf.refits = 0;
  c->rf.refit_ms = 0.0;
  c->build_info.ref_tree_nodes = 0;
  c->build_info.ref_tree_stupid_volume = 0.0;
}

// ---- the uniform grid, built on the device ----------------------------------------------------------------------------
// The uniform grid built in HBM (csrc/rtow_build_grid.hip) from the record arrays resident in c->sph / mov / tri; the host
// does the scalar steps between the phases with the code the host builder uses, so the image is byte-identical.  gimg.ok
// stays false when the scene does not suit the grid.  rec.sph (host records) decides the fat-list format; mov, tri and pmat
// are read for their sizes only.  (build_grid, refit_grid_images)
static int grid_device_build(rtow_ctx *c, const rtow_camera_t &cam, const rtow::SceneRecords &rec, rtow::GridImage &gimg) {
  const std::vector<double> &sph = rec.sph, &mov = rec.mov, &tri = rec.tri;
  const int ns = (int)(sph.size() / 4), nm = (int)(mov.size() / 8), nt = (int)(tri.size() / 12);
  const double cpp = c->knobs.grid_cpp;
  const double large_ratio = c->knobs.grid_large;
  int rc;
  rtow::GridBuildBounds gb;
  int grc = rtow::grid_build_phase1((const double *)c->sph.p, (const double *)c->sph_r.p, (const double *)c->mov.p,
                                    (const double *)c->tri.p, ns, nm, nt, cam.t0, cam.t1, large_ratio,
                                    nullptr, &c->grid_scratch, &gb);
  if (grc) return fail(RTOW_EHIP, "device grid build failed (phase 1, stage %d): %s", grc, hipGetErrorString(hipGetLastError()));
  if (gb.n_small <= 0 || gb.n_large > 64) return RTOW_OK;
  rtow::GridHeader hd;
  rtow::grid_header(gb.gmn, gb.gmx, gb.scale_prims, cam.origin, (size_t)gb.n_small, cpp, hd);
  unsigned long long total_ids = 0, max_list = 0;
  grc = rtow::grid_build_phase2(c->grid_scratch, hd.gminf, hd.cellf, hd.n, hd.pad, nullptr, &total_ids, &max_list);
  if (grc) return fail(RTOW_EHIP, "device grid build failed (phase 2, stage %d): %s", grc, hipGetErrorString(hipGetLastError()));
  if (max_list > 255 || total_ids + (unsigned long long)gb.n_large >= (1u << 24)) return RTOW_OK;
  const size_t ncell = (size_t)hd.n[0] * hd.n[1] * hd.n[2];
  for (int k = 0; k < 3; ++k) gimg.n[k] = hd.n[k];
  double scale_small = 0.0;  // (the host builder's rule: rtow_grid.h build_grid_image)
  for (int k = 0; k < 3; ++k)
    scale_small = std::max({scale_small, std::fabs(gb.gmn[k]), std::fabs(gb.gmx[k]), std::fabs(cam.origin[k])});
  const uint32_t fat = rtow::grid_wants_fat_lists(nm, nt, ncell, (size_t)total_ids + (size_t)gb.n_large,
                                                  (size_t)gb.n_large, sph, mov, tri, rec.pmat, rec.mats_bytes, (size_t)total_ids,
                                                  scale_small);
  rtow::layout_grid_image(ncell, (size_t)total_ids + (size_t)gb.n_large, (size_t)gb.n_large, sph, mov, tri, rec.pmat,
                          rec.mats_bytes, gimg, true, fat ? (size_t)total_ids : 0, fat ? fat : 48u);
  if ((rc = c->gblob.ensure(gimg.total_bytes))) return rc;
  unsigned char *gp = (unsigned char *)c->gblob.p;
  unsigned char header[64];
  const uint32_t off_large = (uint32_t)(gimg.off_ids + total_ids * 4);
  rtow::write_grid_header(header, hd, gimg.n_large, off_large, gimg.off_fat, gimg.fat_stride);
  std::memcpy(gimg.header, header, 64);
  HIPCHK(hipMemsetAsync(gp, 0, gimg.total_bytes, nullptr));
  if ((rc = h2d_block(gp, header, 64))) return rc;  // (`header` is on the stack: never the source of an async copy)
  if ((rc = copy_record_sections(gp, {gimg.off_sph, gimg.off_mov, gimg.off_tri, gimg.off_pmat, gimg.off_mats}, c, ns, nm, nt,
                                 (int)rec.pmat.size(), rec.mats_bytes.size())))
    return rc;
  grc = rtow::grid_build_phase3(c->grid_scratch, hd.gminf, hd.cellf, hd.n, hd.pad, total_ids, gp, gimg.off_cells,
                                gimg.off_ids, nullptr, (const double *)c->sph.p, gimg.off_fat,
                                (const double *)c->mov.p, ns, gimg.fat_stride);
  if (grc) return fail(RTOW_EHIP, "device grid build failed (phase 3, stage %d): %s", grc, hipGetErrorString(hipGetLastError()));
  gimg.ok = true;
  return RTOW_OK;
}

// ---- rtow_scene_upload and the lean upload of rtow_render: the stages ---------------------------------------------------

// the record arrays (plus tri16), class-major, through the pinned arena
static int upload_record_arrays(rtow_ctx *c, const rtow::SceneRecords &rec, unsigned need) {
  int rc;
  if ((rc = upload(c->sph, rec.sph)) || (rc = upload(c->sph_r, rec.sph_r)) || (rc = upload(c->mov, rec.mov)) ||
      (rc = upload(c->tri, rec.tri)) || (rc = upload(c->prim_mat, rec.pmat)) || (rc = upload(c->mats, rec.mats_bytes)))
    return rc;
  // the STREAM kernel's copy of the triangle records at a 128-byte stride (rtow_device.h): for the uploads that may be
  // followed by a STREAM render of triangles — everything (rtow_scene_upload) or nothing but the records (a render
  // that asked for the STREAM / reference-tree kernels)
  c->have_tri16 = false;
  const size_t nt = rec.tri.size() / 12;
  if (nt > 0 && (need == kNeedAll || need == 0u)) {
    std::vector<double> tri16(nt * 16, 0.0);
    for (size_t i = 0; i < nt; ++i) std::memcpy(&tri16[i * 16], &rec.tri[i * 12], 12 * sizeof(double));
    if ((rc = upload(c->tri16, tri16))) return rc;
    c->have_tri16 = true;
  }
  return RTOW_OK;
}

// What the tree stage leaves for the stages after it
struct TreeImages {
  rtow::SceneImage img;  // the binary image: offsets and node count (the blob too when the host built it)
  bool leaf_direct = false;
  std::vector<double> tri_img;  // leaf-ordered copies (triangle meshes, host builder)
  std::vector<int32_t> pmat_img;
  rtow::Bvh4Image img4;  // the 4-wide image (.ok false: none; the blob too when the host built it)
  size_t bytes4 = 0;
};

// the trees built in HBM from the record arrays just uploaded; the host only lays out the image sections around them
static int build_tree_images_device(rtow_ctx *c, const rtow_scene_t *s, const rtow::SceneRecords &rec, bool want2, bool want4,
                                    int leaf_max, TreeImages &t) {
  const int ns = s->n_spheres, nm = s->n_moving, nt = s->n_triangles;
  int rc, n_nodes = 0;
  int brc = rtow::lbvh_build((const double *)c->sph.p, (const double *)c->sph_r.p, (const double *)c->mov.p,
                             (const double *)c->tri.p, ns, nm, nt, s->camera.t0, s->camera.t1, s->camera.origin,
                             leaf_max, nullptr, &c->lbvh_scratch, &n_nodes,
                             c->knobs.device_tree == 2   ? -1
                             : c->knobs.device_tree == 0 ? 0
                             : c->knobs.ploc_radius > 0  ? c->knobs.ploc_radius
                                                         : (ns + nm + nt <= 16384 ? 16 : 8));
  if (brc) return fail(RTOW_EHIP, "device BVH build failed (stage %d): %s", brc, hipGetErrorString(hipGetLastError()));
  if (want2) {
    rtow::SceneImage &img = t.img;
    rtow::layout_scene_image(n_nodes, (size_t)(ns + nm + nt), rec.sph, rec.mov, rec.tri, rec.pmat, rec.mats_bytes, img, true);
    if ((rc = c->blob.ensure(img.total_bytes))) return rc;
    // image sections: device-to-device copies of the arrays uploaded above, zeroed node section
    unsigned char *bp = (unsigned char *)c->blob.p;
    HIPCHK(hipMemsetAsync(bp, 0, img.off_sph, nullptr));
    if ((rc = copy_record_sections(bp, {img.off_sph, img.off_mov, img.off_tri, img.off_pmat, img.off_mats}, c, ns, nm, nt,
                                   ns + nm + nt, rec.mats_bytes.size())))
      return rc;
    brc = rtow::lbvh_emit(c->lbvh_scratch, leaf_max, bp, img.off_ids, n_nodes, nullptr);
    if (brc == 4) return fail(RTOW_EINVAL, "internal error: device-built scene image failed validation (BVH links)");
    if (brc) return fail(RTOW_EHIP, "device BVH emit failed (stage %d): %s", brc, hipGetErrorString(hipGetLastError()));
  }
  // triangle meshes: the 4-wide image the BVH4 kernel walks, collapsed from the same radix tree ON THE DEVICE
  // (csrc/rtow_build.hip) — the reference builds its tree inside render()'s timer (src/render.cpp:73-110,141-188);
  // with the device builder nothing of the build runs on the host
  if (!want4 || leaf_max > 4) return RTOW_OK;
  int n4 = 0, depth4 = 0;
  float rb[6];
  brc = rtow::lbvh_bvh4_collapse(c->lbvh_scratch, leaf_max, nullptr, &n4, &depth4, rb);
  if (brc == 4) return fail(RTOW_EINVAL, "internal error: device 4-wide collapse failed validation");
  if (brc != 0 && brc != 5)
    return fail(RTOW_EHIP, "device 4-wide collapse failed (stage %d): %s", brc, hipGetErrorString(hipGetLastError()));
  if (brc == 5) return RTOW_OK;  // (beyond the format's limits — the binary walk takes the scene)
  rtow::Bvh4Image &img4 = t.img4;
  rtow::Bvh4Layout lay = rtow::bvh4_layout((size_t)n4, rtow::kBvh4NodeBytes, (size_t)nt, rec.mats_bytes.size());
  // the same rule as the host builder: binary32 planes when LDS holds the whole image beside the stack,
  // 64-byte nodes with binary16 planes in the mesh's own frame otherwise (rtow_bvh4.h)
  img4.half = lay.total + bvh4_min_stack(c) * 4u * 1024u > kLdsLimit;
  if (img4.half) {
    lay = rtow::bvh4_layout((size_t)n4, rtow::kBvh4HalfNodeBytes, (size_t)nt, rec.mats_bytes.size());
    const double lo[3] = {rb[0], rb[1], rb[2]}, hi[3] = {rb[3], rb[4], rb[5]};
    rtow::bvh4_half_frame(lo, hi, img4.map_c, img4.map_s);
  }
  if ((rc = c->blob4.ensure(lay.total))) return rc;
  unsigned char *b4 = (unsigned char *)c->blob4.p;
  HIPCHK(hipMemsetAsync(b4 + lay.off_pmat, 0, lay.total - lay.off_pmat, nullptr));  // (alignment gaps)
  HIPCHK(hipMemcpyAsync(b4 + lay.off_mats, c->mats.p, rec.mats_bytes.size(), hipMemcpyDeviceToDevice, nullptr));
  brc = rtow::lbvh_bvh4_emit(c->lbvh_scratch, b4, img4.half ? 1 : 0, img4.map_c, img4.map_s, lay.off_tri, lay.off_pmat,
                             (const double *)c->tri.p, (const int32_t *)c->prim_mat.p, nullptr);
  if (brc == 4) return fail(RTOW_EINVAL, "internal error: device-built 4-wide image failed validation");
  if (brc) return fail(RTOW_EHIP, "device 4-wide emit failed (stage %d): %s", brc, hipGetErrorString(hipGetLastError()));
  img4.off_tri = lay.off_tri;
  img4.off_pmat = lay.off_pmat;
  img4.off_mats = lay.off_mats;
  img4.n_nodes = n4;
  img4.depth = depth4;
  img4.ok = true;
  t.bytes4 = lay.total;
  return RTOW_OK;
}

// the host's SAH tree, and both images made from it
static int build_tree_images_host(rtow_ctx *c, const rtow_scene_t *s, const rtow::SceneRecords &rec, bool want2, bool want4,
                                  int leaf_max, bool mesh_tree, TreeImages &t) {
  const int ns = s->n_spheres, nm = s->n_moving, nt = s->n_triangles;
  int rc;
  rtow::HostBvh bvh;
  const double c_trav = c->knobs.bvh_ct >= 0.0 ? c->knobs.bvh_ct : (mesh_tree ? 1.5 : 0.0);
  rtow::build_bvh(rec.sph, rec.sph_r, rec.mov, rec.tri, bvh, leaf_max, c_trav, s->camera.t0, s->camera.t1);
  std::vector<int32_t> prim_order;  // the tree's primitive order before the leaf-order pass renumbers it (for the 4-wide image)
  if (want4 && leaf_max <= 4) prim_order = bvh.prim;
  if (want2) {
    if (ns == 0 && nm == 0 && !c->knobs.no_leaf_order) {
      // Triangle meshes: the image holds the triangle records and their material indices in LEAF order
      // and the id list is the identity, so a leaf test reads its records directly instead of id ->
      // record (one LDS / L2 round trip less per leaf, and leaf neighbours are memory neighbours:
      // +10 % on the 96.8k-triangle mesh, whose image lives in global memory).  `best.prim` is then a
      // leaf slot; shading reads the same permuted sections.  (Host builder only.)
      t.tri_img.resize(rec.tri.size());
      t.pmat_img.resize(rec.pmat.size());
      for (size_t sl = 0; sl < bvh.prim.size(); ++sl) {
        std::memcpy(&t.tri_img[sl * 12], &rec.tri[(size_t)bvh.prim[sl] * 12], 96);
        t.pmat_img[sl] = rec.pmat[bvh.prim[sl]];
      }
      for (size_t sl = 0; sl < bvh.prim.size(); ++sl) bvh.prim[sl] = (int32_t)sl;
      rtow::make_scene_image(bvh, rec.sph, rec.mov, t.tri_img, s->camera.origin, t.img, t.pmat_img, rec.mats_bytes);
      t.leaf_direct = true;
    } else {
      rtow::make_scene_image(bvh, rec.sph, rec.mov, rec.tri, s->camera.origin, t.img, rec.pmat, rec.mats_bytes);
    }
    if (!rtow::validate_scene_image(t.img, ns + nm + nt))
      return fail(RTOW_EINVAL, "internal error: scene image failed validation (BVH links)");
    if ((rc = upload(c->blob, t.img.blob))) return rc;
  }
  // triangle meshes: the 4-wide tree collapsed from the same SAH tree (rtow_bvh4.h; leaves of at most 4 triangles)
  if (!want4 || prim_order.empty()) return RTOW_OK;
  rtow::Bvh4Image &img4 = t.img4;
  bvh.prim = prim_order;
  // an image that LDS cannot hold whole is read from L2 below the top of its tree: 64-byte nodes with
  // binary16 planes (4 loads per node instead of 7; rtow_bvh4.h).  The records alone decide it for a big mesh
  // (no point in building the binary32 image first: 20 ms of the 96.8k-triangle mesh's upload)
  const bool surely_half = (size_t)nt * 100u + bvh4_min_stack(c) * 4u * 1024u > kLdsLimit;
  rtow::make_bvh4_image(bvh, rec.tri, rec.pmat, rec.mats_bytes, s->camera.origin, img4, /*half=*/surely_half);
  if (!surely_half && img4.ok && img4.blob.size() + bvh4_min_stack(c) * 4u * 1024u > kLdsLimit)
    rtow::make_bvh4_image(bvh, rec.tri, rec.pmat, rec.mats_bytes, s->camera.origin, img4, /*half=*/true);
  if (!img4.ok) return RTOW_OK;
  if (!rtow::validate_bvh4_image(img4, (size_t)nt))
    return fail(RTOW_EINVAL, "internal error: 4-wide scene image failed validation");
  if ((rc = upload(c->blob4, img4.blob))) return rc;
  t.bytes4 = img4.blob.size();
  return RTOW_OK;
}

// BVH over the same records, packed with them into one scene image; for a triangle mesh the 4-wide image too
static int build_tree_images(rtow_ctx *c, const rtow_scene_t *s, const rtow::SceneRecords &rec, unsigned need, TreeImages &t) {
  const int ns = s->n_spheres, nm = s->n_moving, nt = s->n_triangles;
  const bool device = c->builder == RTOW_BUILDER_DEVICE_LBVH;
  // host SAH stops splitting by cost (mostly 1-2 primitives per leaf, cap 4); the radix tree has
  // no cost model, so its leaves are capped at 2 (measured: 1 and 2 equal, 4 is 8-17 % slower)
  int leaf_max = device ? 2 : 4;
  // Triangle meshes (the tree the 4-wide image is collapsed from): PAIRS of triangles per leaf — a cost of 1.5
  // primitive tests per level descended makes the SAH stop at two triangles, the cap keeps it from stopping
  // earlier.  Against single-triangle leaves (cost 0, what the builder makes of any cap): suzanne 452 -> 261
  // 4-wide nodes, the whole image now fits LDS with 7 stack entries per lane, 4.06 -> 4.67 Gsamples/s; the
  // 96.8k-triangle mesh 2.00 -> 2.08.  (Cost 1 / cap 4: 4.45 / 2.01; cap 3: 4.49 / 2.01; cost 3 / cap 2: the same
  // tree as 1.5 / 2.)  The binary walk over the same tree loses 3.5 % on suzanne (3.39 -> 3.27): it is the fallback.
  const bool mesh_tree = ns == 0 && nm == 0 && nt > 0 && !device && !c->knobs.no_bvh4;
  if (mesh_tree) leaf_max = 2;
  if (c->knobs.bvh_leaf > 0) leaf_max = std::min(std::max(c->knobs.bvh_leaf, 1), 7);
  const bool want2 = (need & kNeedBvh) != 0;
  const bool want4 = (need & kNeedBvh4) != 0 && ns == 0 && nm == 0 && nt > 0 && !c->knobs.no_bvh4;
  int rc = RTOW_OK;
  if (want2 || want4)
    rc = device ? build_tree_images_device(c, s, rec, want2, want4, leaf_max, t)
                : build_tree_images_host(c, s, rec, want2, want4, leaf_max, mesh_tree, t);
  if (rc == RTOW_OK) bvh4_resident(c, t.img4, t.bytes4);
  return rc;
}

// uniform grid over the small primitives (when the scene suits it): gimg.ok; on_device: the image exists only in HBM
static int build_grid(rtow_ctx *c, const rtow_camera_t &cam, const rtow::SceneRecords &rec, unsigned need,
                      rtow::GridImage &gimg, bool &on_device) {
  // big meshes never take the grid (a triangle spans many cells: 0.4x the BVH):
  // skip the host build, a GRID request then falls back to the BVH
  const bool suits = (int)(rec.tri.size() / 12) <= c->knobs.grid_max_tris;
  on_device = false;
  if (!(need & kNeedGrid) || !suits) return RTOW_OK;  // (not asked for, or a big mesh)
  if (c->builder == RTOW_BUILDER_DEVICE_LBVH) {
    // the same grid, built in HBM (csrc/rtow_build_grid.hip)
    on_device = true;
    return grid_device_build(c, cam, rec, gimg);
  }
  rtow::build_grid_image(rec.sph, rec.sph_r, rec.mov, rec.tri, cam.origin, gimg, c->knobs.grid_cpp, c->knobs.grid_large, cam.t0,
                         cam.t1, rec.pmat, rec.mats_bytes);
  return RTOW_OK;
}

// DevScene: the record arrays and the binary image (bvh4_resident and grid_resident have written their parts)
static void publish_dev_scene(rtow_ctx *c, const rtow_scene_t *s, const TreeImages &t) {
  const rtow::SceneImage &img = t.img;
  c->blob_bytes = (uint32_t)img.total_bytes;
  c->bvh_nodes = img.n_nodes;
  rtow::DevScene &ds = c->ds;
  ds.sph = (const double *)c->sph.p;
  ds.sph_r = (const double *)c->sph_r.p;
  ds.mov = (const double *)c->mov.p;
  ds.tri = (const double *)c->tri.p;
  ds.tri16 = c->have_tri16 ? (const double *)c->tri16.p : nullptr;
  ds.prim_mat = (const int32_t *)c->prim_mat.p;
  ds.mats = (const rtow::DevMaterial *)c->mats.p;
  ds.n_sph = s->n_spheres;
  ds.n_mov = s->n_moving;
  ds.n_tri = s->n_triangles;
  ds.n_mats = s->n_materials;
  ds.blob = (const unsigned char *)c->blob.p;
  ds.blob_bytes = c->blob_bytes;
  ds.off_ids = img.off_ids;
  ds.off_sph = img.off_sph;
  ds.off_mov = img.off_mov;
  ds.off_tri = img.off_tri;
  ds.off_pmat = img.off_pmat;
  ds.off_mats = img.off_mats;
  ds.n_nodes = img.n_nodes;
  ds.leaf_direct = t.leaf_direct ? 1 : 0;
  c->n_prims = s->n_spheres + s->n_moving + s->n_triangles;
}

// the f32 build's images (same trees, binary32 records for the small primitives), derived from the binary64 ones
static int build_f32_images(rtow_ctx *c, const rtow::SceneRecords &rec, const TreeImages &t, const rtow::GridImage &gimg,
                            bool grid_on_device) {
  int rc;
  const bool device_tree = c->builder == RTOW_BUILDER_DEVICE_LBVH;
  Image32 b32;
  make_image32(device_tree ? nullptr : t.img.blob.data(), t.img.off_sph, rec.sph, rec.mov, t.leaf_direct ? t.tri_img : rec.tri,
               t.leaf_direct ? t.pmat_img : rec.pmat, rec.mats_bytes, b32);
  if ((rc = upload(c->blob32, b32.blob))) return rc;
  if (device_tree)  // nodes + ids exist only in HBM
    HIPCHK(hipMemcpy(c->blob32.p, c->blob.p, t.img.off_sph, hipMemcpyDeviceToDevice));
  image32_resident(c->ds32, false, &b32, c->blob32.p, b32.blob.size());
  if (!gimg.ok) {
    image32_resident(c->ds32, true, nullptr, nullptr, 0);
    return RTOW_OK;
  }
  Image32 g32;
  make_image32(grid_on_device ? nullptr : gimg.blob.data(), gimg.off_sph, rec.sph, rec.mov, rec.tri, rec.pmat, rec.mats_bytes, g32);
  if ((rc = upload(c->gblob32, g32.blob))) return rc;
  if (grid_on_device)  // header, cells and ids exist only in HBM
    HIPCHK(hipMemcpy(c->gblob32.p, c->gblob.p, gimg.off_sph, hipMemcpyDeviceToDevice));
  image32_resident(c->ds32, true, &g32, c->gblob32.p, g32.blob.size());
  return RTOW_OK;
}

static int scene_upload(rtow_ctx *c, const rtow_scene_t *s, unsigned need) {
  // validate
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  int rc = validate_scene(s);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  if (!c->arena.p) {
    if (hipHostMalloc((void **)&c->arena.p, 8u << 20, hipHostMallocDefault) == hipSuccess)
      c->arena.cap = 8u << 20;
    else
      c->arena.p = nullptr;  // (uploads then copy synchronously)
  }
  ArenaScope arena_scope(&c->arena);
  if (need & kNeedF32) need |= kNeedBvh | kNeedGrid;  // the binary32 images are derived from the binary64 ones (BVH2, grid)
  // invalidate, host copy, records, record arrays
  c->built = 0;
  c->have_scene = false;
  invalidate_resident(c, Invalidate::Upload);
  const double t_up0 = now_ms();
  if ((rc = host_scene_copy(c, s, /*with_order=*/true))) return rc;
  const rtow::SceneRecords rec = make_scene_records(s);
  if ((rc = upload_record_arrays(c, rec, need))) return rc;
  // trees, grid
  const double t_bvh0 = now_ms();
  TreeImages trees;
  if ((rc = build_tree_images(c, s, rec, need, trees))) return rc;
  const double t_bvh1 = now_ms();
  rtow::GridImage gimg;
  bool grid_on_device = false;
  if ((rc = build_grid(c, s->camera, rec, need, gimg, grid_on_device))) return rc;
  const double t_grid1 = now_ms();
  if (gimg.ok && !grid_on_device && (rc = upload(c->gblob, gimg.blob))) return rc;
  if ((rc = grid_resident(c, gimg, s->n_spheres))) return rc;
  // DevScene, the f32 build's images, camera
  publish_dev_scene(c, s, trees);
  c->ds32 = c->ds;
  if ((need & kNeedF32) && (rc = build_f32_images(c, rec, trees, gimg, grid_on_device))) return rc;
  if ((rc = camera_resident(c, s->camera, (need & kNeedF32) != 0))) return rc;
  // Ordering contract (include/rtow.h): the copies and build kernels above are queued on the null stream without a
  // host wait; a render on ANOTHER stream (a hipStreamNonBlocking stream is not ordered behind the null stream) waits
  // for this event first (render_levels)
  HIPCHK(hipEventRecord(c->upload_ev, nullptr));
  c->built = need;
  c->have_scene = true;
  rtow_build_info_t &bi = c->build_info;
  bi.builder = c->builder;
  bi.bvh_nodes = (int32_t)trees.img.n_nodes;
  bi.bvh_image_bytes = (int32_t)c->blob_bytes;
  bi.grid_image_bytes = (int32_t)c->gblob_bytes;
  bi.bvh_build_ms = t_bvh1 - t_bvh0;
  bi.grid_build_ms = t_grid1 - t_bvh1;
  bi.upload_ms = now_ms() - t_up0;
  return RTOW_OK;
}

namespace rtow {

int validate_scene(const rtow_scene_t *s) {
  if (!s) return fail(RTOW_EINVAL, "scene is NULL");
  if (s->n_spheres < 0 || s->n_moving < 0 || s->n_triangles < 0 || s->n_materials < 0)
    return fail(RTOW_EINVAL, "negative count in scene");
  const long long np = (long long)s->n_spheres + s->n_moving + s->n_triangles;
  if (np == 0) return fail(RTOW_EEMPTY, "scene has no primitives");
  if (s->n_prims != np) return fail(RTOW_EINVAL, "n_prims (%d) != sum of classes (%lld)", s->n_prims, np);
  if (s->n_materials == 0 || !s->materials) return fail(RTOW_EINVAL, "scene has no materials");
  if ((s->n_spheres && (!s->sphere_geom || !s->sphere_mat)) ||
      (s->n_moving && (!s->moving_geom || !s->moving_mat)) ||
      (s->n_triangles && (!s->triangle_geom || !s->triangle_mat)))
    return fail(RTOW_EINVAL, "NULL geometry/material array");
  auto chk = [&](const int32_t *m, int n) {
    for (int i = 0; i < n; ++i)
      if (m[i] < 0 || m[i] >= s->n_materials) return false;
    return true;
  };
  if (!chk(s->sphere_mat, s->n_spheres) || !chk(s->moving_mat, s->n_moving) ||
      !chk(s->triangle_mat, s->n_triangles))
    return fail(RTOW_EINVAL, "material index out of range");
  for (int i = 0; i < s->n_materials; ++i)
    if (s->materials[i].kind < 0 || s->materials[i].kind > 2)
      return fail(RTOW_EINVAL, "material %d has unknown kind %d", i, s->materials[i].kind);
  return RTOW_OK;
}

int impl_scene_upload(rtow_ctx *c, const rtow_scene_t *s) {
  // AUTO knows no config here: the host builder (include/rtow.h), whatever an earlier rtow_render resolved AUTO to
  if (c && c->builder_req == RTOW_BUILDER_AUTO) c->builder = RTOW_BUILDER_HOST_SAH;
  return scene_upload(c, s, kNeedAll);
}

// Upload for ONE render whose config is known: only what its kernel reads (the cover scene through the grid
// kernel needs no BVH image, no 4-wide image and no binary32 images: 0.48 -> 0.15 ms per call).
int upload_for(rtow_ctx *c, const rtow_scene_t *scene, const rtow_config_t *cfg) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  int rc = validate_scene(scene);
  if (rc) return rc;
  const long long np = (long long)scene->n_spheres + scene->n_moving + scene->n_triangles;
  unsigned need;
  const int k = cfg->kernel;
  const bool mesh = scene->n_spheres == 0 && scene->n_moving == 0 && scene->n_triangles > 0 && !c->knobs.no_bvh4;
  if (cfg->precision == RTOW_F32)
    need = kNeedAll;
  else if (k == RTOW_KERNEL_REFTREE || k == RTOW_KERNEL_BRUTE || (k == RTOW_KERNEL_AUTO && np <= 16))
    need = 0u;
  else if ((k == RTOW_KERNEL_AUTO || k == RTOW_KERNEL_GRID) && scene->n_triangles == 0)
    need = kNeedGrid;
  else if (k == RTOW_KERNEL_GRID)
    need = kNeedGrid | kNeedBvh;
  else if (mesh && (k == RTOW_KERNEL_AUTO || k == RTOW_KERNEL_BVH4))
    need = kNeedBvh4;  // the 4-wide image only (the binary image is another 20 ms and 10 MB for the 96.8k-triangle mesh)
  else
    need = kNeedBvh;
  if (c->builder_req == RTOW_BUILDER_AUTO) {
    // AUTO (include/rtow.h): the device builder where it delivers the frame sooner.  Its tree is the host's (binned SAH,
    // csrc/rtow_build.hip pass 3c: the same node and triangle tests per segment), so what decides is the build: a fixed
    // ~1.7 ms of launches plus ~0.055 us per triangle on the device, ~0.15 us per triangle on the host's 16 threads
    // (96,800 triangles: 7 against 12-16 ms) — the device from about 16,000 triangles on, at any sample count.
    const bool device = mesh && need == kNeedBvh4 && scene->n_triangles >= 16384;
    c->builder = device ? RTOW_BUILDER_DEVICE_LBVH : RTOW_BUILDER_HOST_SAH;
  }
  rc = scene_upload(c, scene, need);
  if (rc == RTOW_OK && (need & kNeedGrid) && !(need & kNeedBvh) && !c->have_grid)
    rc = scene_upload(c, scene, need | kNeedBvh);  // the scene does not suit a grid: the walk falls back to the BVH
  if (rc == RTOW_OK && need == kNeedBvh4 && !c->have_bvh4)
    rc = scene_upload(c, scene, kNeedBvh);  // beyond the 4-wide format's limits: the binary walk takes the mesh
  return rc;
}

// Record slot of a leaf-ordered image -> class-order triangle index (which: 1 the host-built mesh BVH image, 2 the 4-wide
// image).  The leaf-ordered images hold exact copies of the class-ordered triangle records, so a slot's triangle is found by
// matching its 96 bytes AND its material word: a query reports a slot's material from the image's own per-slot table
// (point_record, hit records), which follows the builder's permutation, so a slot is paired with a triangle equal in both —
// coincident triangles with different materials (a decal over a wall) keep each its own.  Triangles identical in record
// and material are paired in order: any one of them gives the same hit.  Called on the images as uploaded, while
// c->prim_mat is still the upload's (refit_prepare runs before the refit's records stage).
int match_slots(rtow_ctx *c, int which, std::vector<int32_t> &slot2tri) {
  const int nt = c->ds.n_tri;
  const unsigned char *img = which == 1 ? c->ds.blob + c->ds.off_tri : c->ds.blob4 + c->ds.b4_off_tri;
  const unsigned char *img_mat = which == 1 ? c->ds.blob + c->ds.off_pmat : c->ds.blob4 + c->ds.b4_off_pmat;
  const size_t bytes = (size_t)nt * 96u;
  std::vector<unsigned char> rec_cls(bytes), rec_img(bytes);
  std::vector<int32_t> mat_cls((size_t)nt), mat_img((size_t)nt);
  HIPCHK(hipMemcpy(rec_cls.data(), c->tri.p, bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rec_img.data(), img, bytes, hipMemcpyDeviceToHost));
  if (nt) {
    HIPCHK(hipMemcpy(mat_cls.data(), (const int32_t *)c->prim_mat.p + c->ds.n_sph + c->ds.n_mov, (size_t)nt * 4,
                     hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mat_img.data(), img_mat, (size_t)nt * 4, hipMemcpyDeviceToHost));
  }
  std::vector<int32_t> oc((size_t)nt), oi((size_t)nt);
  for (int i = 0; i < nt; ++i) oc[i] = oi[i] = i;
  auto by_record = [](const std::vector<unsigned char> &r, const std::vector<int32_t> &mat) {
    return [&r, &mat](int32_t a, int32_t b) {
      const int m = std::memcmp(&r[(size_t)a * 96u], &r[(size_t)b * 96u], 96);
      if (m != 0) return m < 0;
      return mat[(size_t)a] != mat[(size_t)b] ? mat[(size_t)a] < mat[(size_t)b] : a < b;
    };
  };
  std::sort(oc.begin(), oc.end(), by_record(rec_cls, mat_cls));
  std::sort(oi.begin(), oi.end(), by_record(rec_img, mat_img));
  slot2tri.assign((size_t)nt, -1);
  for (int k = 0; k < nt; ++k) {
    if (std::memcmp(&rec_cls[(size_t)oc[k] * 96u], &rec_img[(size_t)oi[k] * 96u], 96) != 0 ||
        mat_cls[(size_t)oc[k]] != mat_img[(size_t)oi[k]])
      return fail(RTOW_EINVAL, "internal error: the %s image's triangle records are not those of the scene",
                  which == 1 ? "BVH" : "4-wide");
    slot2tri[(size_t)oi[k]] = oc[k];
  }
  return RTOW_OK;
}

}  // namespace rtow

int rtow_build_info(rtow_ctx *c, rtow_build_info_t *out) {
  if (!c || !out) return fail(RTOW_EINVAL, "NULL argument");
  if (!c->have_scene) return fail(RTOW_EINVAL, "no scene uploaded");
  *out = c->build_info;
  return RTOW_OK;
}

// Diagnostic: copy a resident scene image to the host (0 BVH, 1 grid, 2 BVH of the f32 build,
// 3 grid of the f32 build, 4 the 4-wide BVH, 5 the 48-byte frame record of the 4-wide walk: Bvh4Frame).
// Used by the tests to compare host- and device-built images and to check them against the geometry.
struct Bvh4Frame {   // rtow_debug_image(5): what the 4-wide walk decodes binary16 planes with (world = c + h * is)
  double c[3];       // DevScene::b4_c
  float is[3];       // DevScene::b4_is, as stored
  uint32_t half;     // DevScene::b4_half: 64-byte nodes with binary16 planes
  uint32_t lds_limit;  // DevScene::b4_lds_limit of the resident scene (the launches set their own copy's)
  uint32_t pad_;
};
static_assert(sizeof(Bvh4Frame) == 48, "rtow_debug_image(5) record");

int rtow_debug_image(rtow_ctx *c, int32_t which, void *out, int64_t capacity, int64_t *size_out) {
  if (!c || !size_out) return fail(RTOW_EINVAL, "NULL argument");
  if (!c->have_scene) return fail(RTOW_ENOSCENE, "no scene uploaded");
  const void *src = nullptr;
  int64_t bytes = 0;
  Bvh4Frame frame{};
  switch (which) {
    case 0: src = c->blob.p; bytes = c->ds.blob_bytes; break;
    case 1: src = c->gblob.p; bytes = c->ds.gblob_bytes; break;
    case 2: src = c->blob32.p; bytes = c->ds32.blob_bytes; break;
    case 3: src = c->gblob32.p; bytes = c->ds32.gblob_bytes; break;
    case 4: src = c->blob4.p; bytes = c->have_bvh4 ? c->ds.blob4_bytes : 0; break;
    case 5:
      if (c->have_bvh4) {
        for (int k = 0; k < 3; ++k) {
          frame.c[k] = c->ds.b4_c[k];
          frame.is[k] = c->ds.b4_is[k];
        }
        frame.half = c->ds.b4_half;
        frame.lds_limit = c->ds.b4_lds_limit;
        bytes = (int64_t)sizeof frame;
      }
      break;
    default: return fail(RTOW_EINVAL, "unknown image %d", which);
  }
  *size_out = bytes;
  if (!out) return RTOW_OK;  // size query
  if (capacity < bytes) return fail(RTOW_EINVAL, "buffer too small (%lld < %lld)", (long long)capacity, (long long)bytes);
  if (which == 5) {
    if (bytes) std::memcpy(out, &frame, sizeof frame);
    return RTOW_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  if (bytes) HIPCHK(hipMemcpy(out, src, (size_t)bytes, hipMemcpyDeviceToHost));
  return RTOW_OK;
}

// ---- in-place refit (rtow_scene_refit) -------------------------------------------------------------------------------
// The same shape as the resident scene: counts and insertion order (checked before anything is written).
static int refit_check_shape(const rtow_ctx *c, const rtow_scene_t *s) {
  if (s->n_spheres != c->ds.n_sph || s->n_moving != c->ds.n_mov || s->n_triangles != c->ds.n_tri || s->n_prims != c->n_prims ||
      s->n_materials != c->ds.n_mats)
    return fail(RTOW_EINVAL, "rtow_scene_refit: the scene's counts (%d spheres, %d moving, %d triangles, %d materials) are not "
                "the resident scene's (%d, %d, %d, %d): call rtow_scene_upload", s->n_spheres, s->n_moving, s->n_triangles,
                s->n_materials, c->ds.n_sph, c->ds.n_mov, c->ds.n_tri, c->ds.n_mats);
  const rtow_ctx::HostSceneCopy &h = c->host_scene;
  const bool order = s->prim_kind && s->prim_index;
  if (order != h.have_order ||
      (order && (std::memcmp(s->prim_kind, h.pk.data(), (size_t)s->n_prims * 4) != 0 ||
                 std::memcmp(s->prim_index, h.pi.data(), (size_t)s->n_prims * 4) != 0)))
    return fail(RTOW_EINVAL, "rtow_scene_refit: prim_kind / prim_index differ from the resident scene's insertion order");
  return RTOW_OK;
}

// What the first refit after an upload derives from the images as built, before they are overwritten: the slot maps of
// the leaf-ordered images, the parent links of both trees, and the area sum of the binary BVH for the uploaded geometry.
static int refit_prepare(rtow_ctx *c) {
  rtow_ctx::Refit &r = c->rf;
  const rtow::DevScene &ds = c->ds;
  const int ns = ds.n_sph, nm = ds.n_mov, nt = ds.n_tri, np = c->n_prims;
  int rc;
  const bool bvh2 = (c->built & kNeedBvh) != 0;
  r.slot2tri[0].clear();
  r.slot2tri[1].clear();
  if (bvh2 && ds.leaf_direct) {
    if ((rc = match_slots(c, 1, r.slot2tri[0])) || (rc = r.map2.ensure((size_t)nt * 4))) return rc;
    HIPCHK(hipMemcpy(r.map2.p, r.slot2tri[0].data(), (size_t)nt * 4, hipMemcpyHostToDevice));
  }
  if (c->have_bvh4) {
    if ((rc = match_slots(c, 2, r.slot2tri[1])) || (rc = r.map4.ensure((size_t)nt * 4))) return rc;
    HIPCHK(hipMemcpy(r.map4.p, r.slot2tri[1].data(), (size_t)nt * 4, hipMemcpyHostToDevice));
  }
  if ((rc = r.area.ensure(8 * sizeof(double))) || (rc = r.pbox.ensure((size_t)np * 48))) return rc;
  if (bvh2) {
    const int n = ds.n_nodes;
    if ((rc = r.par2.ensure((size_t)n * 4)) || (rc = r.flags.ensure((size_t)n * 4)) || (rc = r.nbox2.ensure((size_t)n * 48)) ||
        (rc = r.partials.ensure(((size_t)n + 255) / 256 * 8)))
      return rc;
    if (rtow::refit_bvh2_links(ds.blob, n, (int32_t *)r.par2.p, nullptr))
      return fail(RTOW_EHIP, "refit link pass failed: %s", hipGetErrorString(hipGetLastError()));
    // the upload's geometry: its records and shutter are still resident
    if (rtow::refit_prim_boxes(ds.sph, ds.sph_r, ds.mov, ds.tri, ns, nm, nt, c->cam.t0, c->cam.t1, (double *)r.pbox.p, nullptr) ||
        rtow::refit_bvh2(const_cast<unsigned char *>(ds.blob), n, ds.off_ids, np,
                         ds.leaf_direct ? (const int32_t *)r.map2.p : nullptr, ns + nm,
                         (const double *)r.pbox.p, (const int32_t *)r.par2.p, (uint32_t *)r.flags.p, (double *)r.nbox2.p,
                         (double *)r.partials.p, /*emit=*/0, c->cam.origin, (double *)r.area.p, nullptr))
      return fail(RTOW_EHIP, "refit area pass failed: %s", hipGetErrorString(hipGetLastError()));
  }
  if (c->have_bvh4) {
    const int n4 = c->build_info.bvh4_nodes;
    const uint32_t nb = ds.b4_half ? rtow::kBvh4HalfNodeBytes : rtow::kBvh4NodeBytes, co = ds.b4_half ? 48u : 96u;
    if ((rc = r.par4.ensure((size_t)n4 * 4)) || (rc = r.need4.ensure((size_t)n4 * 4)) ||
        (rc = r.flags.ensure((size_t)std::max(n4, ds.n_nodes) * 4)) || (rc = r.nbox4.ensure((size_t)n4 * 48)) ||
        (rc = r.sbox4.ensure((size_t)n4 * 192)))
      return rc;
    if (rtow::refit_bvh4_links(ds.blob4, n4, nb, co, (int32_t *)r.par4.p, (int32_t *)r.need4.p, nullptr))
      return fail(RTOW_EHIP, "refit 4-wide link pass failed: %s", hipGetErrorString(hipGetLastError()));
  }
  r.ready = true;
  return RTOW_OK;
}

// ---- rtow_scene_refit: the stages ---------------------------------------------------------------------------------------

// raw geometry, material indices and records through the pinned arena; the derived records and boxes on the device
static int refit_records_stage(rtow_ctx *c, const rtow_scene_t *s, const rtow::SceneRecords &rec) {
  rtow_ctx::Refit &r = c->rf;
  const int ns = c->ds.n_sph, nm = c->ds.n_mov, nt = c->ds.n_tri, np = c->n_prims;
  int rc;
  if ((rc = r.g_sph.ensure((size_t)ns * 32 + 8)) || (rc = r.g_mov.ensure((size_t)nm * 64 + 8)) ||
      (rc = r.g_tri.ensure((size_t)nt * 72 + 8)))
    return rc;
  if ((ns && (rc = h2d_block(r.g_sph.p, s->sphere_geom, (size_t)ns * 32))) ||
      (nm && (rc = h2d_block(r.g_mov.p, s->moving_geom, (size_t)nm * 64))) ||
      (nt && (rc = h2d_block(r.g_tri.p, s->triangle_geom, (size_t)nt * 72))) ||
      (rc = h2d_block(c->prim_mat.p, rec.pmat.data(), (size_t)np * 4)) ||
      (rc = h2d_block(c->mats.p, rec.mats_bytes.data(), rec.mats_bytes.size())))
    return rc;
  auto *sph = (double *)c->sph.p, *sph_r = (double *)c->sph_r.p, *mov = (double *)c->mov.p, *tri = (double *)c->tri.p;
  if (rtow::refit_records((const double *)r.g_sph.p, (const double *)r.g_mov.p, (const double *)r.g_tri.p, ns, nm, nt, sph,
                          sph_r, mov, tri, c->have_tri16 ? (double *)c->tri16.p : nullptr, nullptr))
    return fail(RTOW_EHIP, "refit record pass failed: %s", hipGetErrorString(hipGetLastError()));
  if (((c->built & kNeedBvh) || c->have_bvh4) &&
      rtow::refit_prim_boxes(sph, sph_r, mov, tri, ns, nm, nt, s->camera.t0, s->camera.t1, (double *)r.pbox.p, nullptr))
    return fail(RTOW_EHIP, "refit box pass failed: %s", hipGetErrorString(hipGetLastError()));
  return RTOW_OK;
}

// binary BVH: records, boxes, planes (and the f32 build's copy of it)
static int refit_bvh2_images(rtow_ctx *c, const rtow_camera_t &cam, size_t mats_n) {
  rtow_ctx::Refit &r = c->rf;
  const rtow::DevScene &ds = c->ds;
  const int ns = ds.n_sph, nm = ds.n_mov, nt = ds.n_tri, np = c->n_prims;
  const auto *sph = (const double *)c->sph.p, *mov = (const double *)c->mov.p, *tri = (const double *)c->tri.p;
  const auto *pmat_tri = (const int32_t *)c->prim_mat.p + ns + nm;
  const int32_t *map2 = ds.leaf_direct ? (const int32_t *)r.map2.p : nullptr;
  int rc;
  unsigned char *b = (unsigned char *)c->blob.p;
  // (a leaf-ordered image: the triangle records and their material indices go through the slot map)
  if (map2 && rtow::refit_tri_section(nt, tri, pmat_tri, map2, b, ds.off_tri, ds.off_pmat, 0, nullptr))
    return fail(RTOW_EHIP, "refit record scatter failed: %s", hipGetErrorString(hipGetLastError()));
  const RecordOffsets all{ds.off_sph, ds.off_mov, ds.off_tri, ds.off_pmat, ds.off_mats};
  if ((rc = copy_record_sections(b, map2 ? RecordOffsets{kSkip, kSkip, kSkip, kSkip, ds.off_mats} : all, c, ns, nm, nt, np, mats_n)))
    return rc;
  if (rtow::refit_bvh2(b, ds.n_nodes, ds.off_ids, np, map2, ns + nm, (const double *)r.pbox.p, (const int32_t *)r.par2.p,
                       (uint32_t *)r.flags.p, (double *)r.nbox2.p, (double *)r.partials.p, /*emit=*/1, cam.origin,
                       (double *)r.area.p + 1, nullptr))
    return fail(RTOW_EHIP, "refit BVH pass failed: %s", hipGetErrorString(hipGetLastError()));
  if (!(c->built & kNeedF32)) return RTOW_OK;
  // the same layout as uploaded: nodes and ids, then the records
  const rtow::DevScene &d32 = c->ds32;
  unsigned char *b32 = (unsigned char *)c->blob32.p;
  HIPCHK(d2d(b32, b, ds.off_sph));
  if ((rc = copy_record_sections(b32, {d32.off_sph, d32.off_mov, kSkip, map2 ? kSkip : d32.off_pmat, d32.off_mats}, c, ns, nm, nt,
                                 np, mats_n)))
    return rc;
  if (rtow::refit_tri_section(nt, tri, pmat_tri, map2, b32, d32.off_tri, map2 ? d32.off_pmat : ~0u, 1, nullptr) ||
      rtow::refit_spheres32(ns, nm, sph, mov, b32, d32.off_sph32, d32.off_mov32, nullptr))
    return fail(RTOW_EHIP, "refit f32 record scatter failed: %s", hipGetErrorString(hipGetLastError()));
  return RTOW_OK;
}

// 4-wide BVH: records in leaf order, boxes, planes in a frame from the new root box
static int refit_bvh4_image(rtow_ctx *c, const rtow_camera_t &cam, size_t mats_n) {
  rtow_ctx::Refit &r = c->rf;
  const rtow::DevScene &ds = c->ds;
  const int ns = ds.n_sph, nm = ds.n_mov, nt = ds.n_tri;
  unsigned char *b4 = (unsigned char *)c->blob4.p;
  const int n4 = c->build_info.bvh4_nodes;
  const uint32_t nb = ds.b4_half ? rtow::kBvh4HalfNodeBytes : rtow::kBvh4NodeBytes, co = ds.b4_half ? 48u : 96u;
  double *frame_dev = (double *)r.area.p + 2;
  if (rtow::refit_tri_section(nt, (const double *)c->tri.p, (const int32_t *)c->prim_mat.p + ns + nm, (const int32_t *)r.map4.p,
                              b4, ds.b4_off_tri, ds.b4_off_pmat, 0, nullptr) ||
      rtow::refit_bvh4(b4, n4, nb, co, (int)ds.b4_half, nt, (const int32_t *)r.map4.p, ns + nm, (const double *)r.pbox.p,
                       (const int32_t *)r.par4.p, (const int32_t *)r.need4.p, (uint32_t *)r.flags.p, (double *)r.nbox4.p,
                       (double *)r.sbox4.p, cam.origin, frame_dev, nullptr))
    return fail(RTOW_EHIP, "refit 4-wide pass failed: %s", hipGetErrorString(hipGetLastError()));
  HIPCHK(d2d(b4 + ds.b4_off_mats, c->mats.p, mats_n));
  if (ds.b4_half) {  // the frame is a launch parameter: 48 bytes back
    double frame[6];
    HIPCHK(hipMemcpy(frame, frame_dev, sizeof frame, hipMemcpyDeviceToHost));
    bvh4_set_frame(c, frame, frame + 3);
  }
  return RTOW_OK;
}

// the grid cannot be refit: rebuilt on the device, present exactly when a fresh upload would build it (and the f32
// build's copy of it)
static int refit_grid_images(rtow_ctx *c, const rtow_scene_t *s, rtow::SceneRecords &rec) {
  const int ns = c->ds.n_sph, nm = c->ds.n_mov, nt = c->ds.n_tri, np = c->n_prims;
  const size_t mats_n = rec.mats_bytes.size();
  int rc;
  rtow::GridImage gimg;
  if (nt <= c->knobs.grid_max_tris) {
    rtow::sphere_records(s->sphere_geom, ns, rec.sph, rec.sph_r);  // (the fat-list format reads the spheres' r*r)
    rec.mov.resize((size_t)nm * 8);                                // (read for their sizes only)
    rec.tri.resize((size_t)nt * 12);
    if ((rc = grid_device_build(c, s->camera, rec, gimg))) return rc;
  }
  if ((rc = grid_resident(c, gimg, ns))) return rc;
  if (!(c->built & kNeedF32)) return RTOW_OK;
  if (!gimg.ok) {
    image32_resident(c->ds32, true, nullptr, nullptr, 0);
    return RTOW_OK;
  }
  Image32 g32;
  const size_t total = layout_image32(gimg.off_sph, ns, nm, nt, np, mats_n, g32);
  if ((rc = c->gblob32.ensure(total))) return rc;
  unsigned char *g = (unsigned char *)c->gblob32.p;
  HIPCHK(hipMemsetAsync(g, 0, total, nullptr));
  HIPCHK(d2d(g, c->gblob.p, gimg.off_sph));  // header, cells and ids
  if ((rc = copy_record_sections(g, {g32.off_sph, g32.off_mov, kSkip, g32.off_pmat, g32.off_mats}, c, ns, nm, nt, np, mats_n)))
    return rc;
  if (rtow::refit_tri_section(nt, (const double *)c->tri.p, nullptr, nullptr, g, g32.off_tri, ~0u, 1, nullptr) ||
      rtow::refit_spheres32(ns, nm, (const double *)c->sph.p, (const double *)c->mov.p, g, g32.off_sph32, g32.off_mov32, nullptr))
    return fail(RTOW_EHIP, "refit f32 grid records failed: %s", hipGetErrorString(hipGetLastError()));
  image32_resident(c->ds32, true, &g32, g, total);
  return RTOW_OK;
}

namespace rtow {
int impl_scene_refit(rtow_ctx *c, const rtow_scene_t *s) {
  // validate
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  int rc = validate_scene(s);
  if (rc) return rc;
  if (!c->have_scene) return fail(RTOW_ENOSCENE, "no scene uploaded");
  if ((rc = refit_check_shape(c, s))) return rc;
  const double t_call = now_ms();
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());  // (earlier work may still read the images)
  rtow_ctx::Refit &r = c->rf;
  if (!r.ev[0])
    for (hipEvent_t &e : r.ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(r.ev[0], nullptr));
  c->have_scene = false;  // (until every image is consistent again: a failure below leaves no scene)
  ArenaScope arena_scope(&c->arena);
  if (!r.ready && (rc = refit_prepare(c))) return rc;
  // records, then every image that is resident
  SceneRecords rec;  // (material indices and materials; the spheres' records where the grid is rebuilt)
  scene_materials(s, rec);
  if ((rc = refit_records_stage(c, s, rec))) return rc;
  if ((c->built & kNeedBvh) && (rc = refit_bvh2_images(c, s->camera, rec.mats_bytes.size()))) return rc;
  if (c->have_bvh4 && (rc = refit_bvh4_image(c, s->camera, rec.mats_bytes.size()))) return rc;
  if ((c->built & kNeedGrid) && (rc = refit_grid_images(c, s, rec))) return rc;
  // camera, bookkeeping
  if ((rc = camera_resident(c, s->camera, (c->built & kNeedF32) != 0))) return rc;
  if ((rc = host_scene_copy(c, s, /*with_order=*/false))) return rc;
  invalidate_resident(c, Invalidate::Refit);
  HIPCHK(hipEventRecord(r.ev[1], nullptr));
  HIPCHK(hipEventRecord(c->upload_ev, nullptr));  // ordering contract of rtow_scene_upload
  c->have_scene = true;
  r.refits++;
  r.refit_ms = now_ms() - t_call;
  return RTOW_OK;
}
}  // namespace rtow

int rtow_refit_info(rtow_ctx *c, rtow_refit_info_t *out) {
  if (!c || !out) return fail(RTOW_EINVAL, "NULL argument");
  if (!c->have_scene) return fail(RTOW_ENOSCENE, "no scene uploaded");
  std::memset(out, 0, sizeof *out);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  const rtow_ctx::Refit &r = c->rf;
  out->refits = r.refits;
  out->grid_resident = c->have_grid ? 1 : 0;
  out->refit_ms = r.refit_ms;
  out->bvh_area_ratio = (c->built & kNeedBvh) ? 1.0 : 0.0;
  if (r.refits > 0) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, r.ev[0], r.ev[1]));
    out->device_ms = ms;
    if (c->built & kNeedBvh) {
      double a[2];
      HIPCHK(hipMemcpy(a, r.area.p, sizeof a, hipMemcpyDeviceToHost));
      out->bvh_area_ratio = a[0] > 0.0 ? a[1] / a[0] : 1.0;  // (a tree without inner nodes cannot degrade)
    }
  }
  return RTOW_OK;
}
