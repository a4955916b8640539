// rtow_ctx.h — the context behind include/rtow.h, for the three host translation units of the C ABI: rtow_scene.cpp
// (what makes a scene resident: upload, refit, the diagnostics that read the images back), rtow_capi.cpp (the context
// itself and everything that renders the resident scene) and rtow_queries.cpp (every query over it).  Host code only: no
// .hip file includes this.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtow.h"
#include "rtow_bvh.h"
#include "rtow_bvh4.h"
#include "rtow_device.h"
#include "rtow_grid.h"
#include "rtow_reftree.h"

namespace rtow {
// the thread's error message (rtow_last_error) and the code to return: defined in rtow_capi.cpp
int set_last_error(int code, const char *fmt, ...);
template <class... A>
inline int fail(int code, const char *fmt, A... a) {
  return set_last_error(code, fmt, a...);
}
}  // namespace rtow
using rtow::fail;

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(RTOW_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// No C++ exception crosses the C ABI (include/rtow.h): the entry points that allocate or start threads run
// their bodies through this.
template <class F>
int guarded(const char *what, F &&f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc &) {
    return fail(RTOW_ENOMEM, "%s: out of host memory", what);
  } catch (const std::exception &e) {
    return fail(RTOW_EINVAL, "%s: %s", what, e.what());
  } catch (...) {
    return fail(RTOW_EINVAL, "%s: unknown C++ exception", what);
  }
}

constexpr unsigned kLdsLimit = 160u * 1024u;
constexpr int kEventRing = 256;
constexpr int kBlock = 256;  // STREAM kernel workgroup

namespace rtow {

struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  int ensure(size_t need) {
    if (need <= bytes) return RTOW_OK;
    if (p) {
      HIPCHK(hipFree(p));
      p = nullptr;
      bytes = 0;
    }
    size_t want = need + need / 8 + 256;
    HIPCHK(hipMalloc(&p, want));
    bytes = want;
    return RTOW_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// Host-to-device copies of a scene upload go through one pinned staging arena and are queued on the null
// stream without a host wait each (a dozen small synchronous copies were 0.2 ms of a cover-scene upload); the
// arena is rewound at the start of the next upload, behind that upload's device synchronisation.  What does
// not fit (a big mesh's images) is copied synchronously from pageable memory as before.
struct PinnedArena {
  unsigned char *p = nullptr;
  size_t cap = 0, used = 0;
};
// A host block to a device address inside an upload: through the arena (the source may be a stack buffer: an
// asynchronous copy must not read it after this returns), synchronously when it does not fit or outside an upload.
int h2d_block(void *dst, const void *src, size_t n);

template <class T>
int upload(DevBuf &b, const std::vector<T> &v) {
  const size_t n = v.size() * sizeof(T);
  if (int rc = b.ensure(n ? n : sizeof(T))) return rc;
  return n ? h2d_block(b.p, v.data(), n) : RTOW_OK;
}

inline double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

}  // namespace rtow
using rtow::DevBuf;
using rtow::PinnedArena;
using rtow::h2d_block;
using rtow::now_ms;
using rtow::upload;

// Experiment knobs (RTOW_* environment variables), read ONCE at rtow_ctx_create: nothing on the
// render path touches the environment.
struct Knobs {
  int bvh_leaf = 0;               // RTOW_BVH_LEAF: leaf size cap of the BVH builders (0 = default)
  double bvh_ct = -1.0;           // RTOW_BVH_CT: SAH cost of descending one level (< 0: 0, meshes 1.5)
  bool no_leaf_order = false;     // RTOW_NO_LEAF_ORDER
  double grid_cpp = 1.0;          // RTOW_GRID_CPP: grid cells per primitive (C2 0.5 / 0.75 / 1 / 1.25 / 1.5 / 2 / 2.5:
                                  // 11.01 / 11.03 / 11.18 / 10.72 / 10.99 / 10.98 / 10.85 Gsamples/s; moving 9.47 / 9.53 / 9.45 /
                                  // 9.14 / 8.99 / 8.83 / 7.64; 3-D clouds are indifferent, scripts/bench_cloud.py)
  double grid_large = 4.0;        // RTOW_GRID_LARGE: diagonal ratio that makes a primitive "large"
  int grid_max_tris = 8192;       // RTOW_GRID_MAX_TRIS
  unsigned long long partials_cap = 8ull << 30;  // RTOW_PARTIALS_MAX_MB
  int bvh_block = 0;              // RTOW_BVH_BLOCK: 256 / 512 / 1024 (0 = automatic)
  int blocks_per_cu = 0;          // RTOW_BLOCKS_PER_CU (0 = occupancy query)
  bool no_tiles = false;          // RTOW_NO_TILES
  int sky_eighths = 1;            // RTOW_SKY_EIGHTHS
  bool stamps = false;            // RTOW_STAMPS: diagnostic region-stamp build
  bool bvh4_no_aux = false;       // RTOW_BVH4_NO_AUX: materials / material indices stay in L2 when only the top of the tree is staged
  bool no_bvh4 = false;           // RTOW_NO_BVH4: triangle meshes keep the binary threaded walk
  // Scheduling of the trip kernels (measured on one MI355X; 0 / "off" switches a measure off):
  int fetch_votes = 0;            // RTOW_FETCH_VOTES: lanes that must need a work item before the fetch block runs
                                  // (0 = per kernel: 4, BVH4 2 — 2 / 4 / 8: C4 4.01 / 3.99 / 3.89, C5 1.98 / 1.96 / 1.92, C2 10.72 / 10.73 / 10.71)
  int leaf_votes = 0;             // RTOW_LEAF_VOTES: lanes that must hold a queued cell / leaf before a leaf phase
                                  //   (0 = per kernel: GRID 16, BVH4 28)
  int walk_cap = -1, walk_max_open = 0;  // RTOW_WALK_CAP=cap,max_open | off: resumable walk (-1 = per kernel:
                                         //   GRID 3,16; BVH4 4,24 with every node in LDS, 4,32 otherwise)
  bool bvh4_sm = false;           // RTOW_BVH4_SM: the state-machine form of the BVH4 kernel (rtow_trace_sm4.h)
  int sm4_votes[3] = {8, 16, 16};  // RTOW_SM4_VOTES=restart,scatter,leaf: quorum of the state machine's blocks
  int bvh4_stack_k = 0;           // RTOW_BVH4_STACK_K: image staged whole if this many stack entries per lane still fit
                                  //   (default 8), else the entries per lane beside the staged top of the tree (default 24)
  int sched_chunk = 10;           // RTOW_SCHED_CHUNK: fast builds: samples per work item aimed at (0 = one item per stream and
                                  //   pixel, like the strict build).  5 / 10 / 20 / 25: 10.88 / 11.18 / 10.22 / 9.55 Gsamples/s on C2
  int sched_chunk_mesh = 16;      //   ... for a scene of triangles only (its walks are longer and resumable: fewer, longer items;
                                  //   4 / 8 / 16 / 32 samples: 4.60 / 4.64 / 4.69 / 4.68 Gsamples/s on C4, 2.29 / 2.30 / 2.32 / 2.32 on C5)
  int ploc_radius = -1;           // RTOW_PLOC_RADIUS: device builder: search radius of the PLOC pass (csrc/rtow_build.hip, round 5);
                                  //   0 = Karras' radix tree (rounds 1-4); -1 = default: 16 up to 16,384 primitives, 8 above
  int device_tree = 2;            // RTOW_DEVICE_TREE=radix|ploc|sah: how the device builder makes its binary tree (0 / 1 / 2);
                                  //   sah = binned surface-area heuristic, top-down, level by level (pass 3c): the default
  bool stream_scalar = false;     // RTOW_STREAM_SCALAR: the STREAM kernel's triangle loop through scalar loads at every size (A/B
                                  //   against the LDS-tiled loop; rounds 1-5a)
  bool no_spec = false;           // RTOW_NO_SPEC: always the generic GRID kernel (A/B against the scene-class specialisations)
  bool no_flat = false;           // RTOW_NO_FLAT: the scene-class kernels keep the 3D walk on a grid with one layer in y (A/B and
                                  //   tests against the two-axis walk, kSpecFlatY)
  bool count_always = false;      // RTOW_COUNT_ALWAYS: a render that returns no statistics launches the counting trace kernel all
                                  //   the same (A/B of the two instantiations in one library)
  bool tile_order = true;         // RTOW_TILE_ORDER=0: the queue keeps the row order alone (one segment); default: the tiles through
                                  //   which no camera ray can reach a primitive are traced last (tile_classify)
  int empty_levels = 3;           // RTOW_EMPTY_LEVELS: levels of a tile one atomic buys in the queue's empty-tile segment (1..16)
  int tail_bound = 0;             // RTOW_TAIL_BOUND (tests only): trips of the end-of-launch protocol before a wave gives up
                                  //   its samples (0 = the structural bound); a small value forces the RTOW_EHIP path
  int radiance_blocks = 0;        // RTOW_RADIANCE_BLOCKS (tests only): cap on the workgroups of a radiance query (0 = none), so
                                  //   that a small batch makes every lane take many rays
  int guides_blocks = 0;          // RTOW_GUIDES_BLOCKS (tests only): the same cap for rtow_guides*: every lane takes many pixels
  void read() {
    auto geti = [](const char *n, int d) { const char *e = std::getenv(n); return e ? std::atoi(e) : d; };
    auto getd = [](const char *n, double d) { const char *e = std::getenv(n); return e ? std::atof(e) : d; };
    bvh_leaf = geti("RTOW_BVH_LEAF", 0);
    bvh_ct = getd("RTOW_BVH_CT", -1.0);
    no_leaf_order = std::getenv("RTOW_NO_LEAF_ORDER") != nullptr;
    grid_cpp = getd("RTOW_GRID_CPP", 1.0);
    grid_large = getd("RTOW_GRID_LARGE", 4.0);
    grid_max_tris = geti("RTOW_GRID_MAX_TRIS", 8192);
    if (const char *e = std::getenv("RTOW_PARTIALS_MAX_MB")) partials_cap = (unsigned long long)std::atoll(e) << 20;
    bvh_block = geti("RTOW_BVH_BLOCK", 0);
    if (bvh_block != 256 && bvh_block != 512 && bvh_block != 1024) bvh_block = 0;
    blocks_per_cu = geti("RTOW_BLOCKS_PER_CU", 0);
    if (blocks_per_cu < 1 || blocks_per_cu > 16) blocks_per_cu = 0;
    no_tiles = std::getenv("RTOW_NO_TILES") != nullptr;
    sky_eighths = std::min(std::max(geti("RTOW_SKY_EIGHTHS", 1), 0), 8);
    stamps = std::getenv("RTOW_STAMPS") != nullptr;
    no_bvh4 = std::getenv("RTOW_NO_BVH4") != nullptr;
    bvh4_no_aux = std::getenv("RTOW_BVH4_NO_AUX") != nullptr;
    fetch_votes = std::min(std::max(geti("RTOW_FETCH_VOTES", 0), 0), 64);
    leaf_votes = std::min(std::max(geti("RTOW_LEAF_VOTES", 0), 0), 64);
    bvh4_sm = std::getenv("RTOW_BVH4_SM") != nullptr;
    if (const char *e = std::getenv("RTOW_WALK_CAP")) {
      int a = 0, b = 0;
      if (std::sscanf(e, "%d,%d", &a, &b) == 2 && a > 0 && b > 0) {
        walk_cap = a;
        walk_max_open = std::min(b, 64);
      } else {
        walk_cap = 0;  // "off"
      }
    }
    if (const char *e = std::getenv("RTOW_SM4_VOTES")) {
      int a = 0, b = 0, d = 0;
      if (std::sscanf(e, "%d,%d,%d", &a, &b, &d) == 3) {
        sm4_votes[0] = std::min(std::max(a, 1), 64);
        sm4_votes[1] = std::min(std::max(b, 1), 64);
        sm4_votes[2] = std::min(std::max(d, 1), 64);
      }
    }
    bvh4_stack_k = std::min(std::max(geti("RTOW_BVH4_STACK_K", 0), 0), 64);
    sched_chunk = std::min(std::max(geti("RTOW_SCHED_CHUNK", 10), 0), 4096);
    sched_chunk_mesh = std::min(std::max(geti("RTOW_SCHED_CHUNK_MESH", 16), 0), 4096);
    tail_bound = std::max(geti("RTOW_TAIL_BOUND", 0), 0);
    radiance_blocks = std::max(geti("RTOW_RADIANCE_BLOCKS", 0), 0);
    guides_blocks = std::max(geti("RTOW_GUIDES_BLOCKS", 0), 0);
    tile_order = geti("RTOW_TILE_ORDER", 1) != 0;
    empty_levels = std::min(std::max(geti("RTOW_EMPTY_LEVELS", 3), 1), 16);
    no_spec = std::getenv("RTOW_NO_SPEC") != nullptr;
    no_flat = std::getenv("RTOW_NO_FLAT") != nullptr;
    count_always = geti("RTOW_COUNT_ALWAYS", 0) != 0;
    stream_scalar = std::getenv("RTOW_STREAM_SCALAR") != nullptr;
    if (const char *e = std::getenv("RTOW_PLOC_RADIUS")) ploc_radius = std::min(std::max(std::atoi(e), 0), 64);
    if (const char *e = std::getenv("RTOW_DEVICE_TREE"))
      device_tree = std::strcmp(e, "radix") == 0 ? 0 : (std::strcmp(e, "ploc") == 0 ? 1 : 2);
    if (ploc_radius >= 0 && !std::getenv("RTOW_DEVICE_TREE")) device_tree = ploc_radius == 0 ? 0 : 1;  // (the radius alone selects PLOC / radix)
  }
};

// what a scene upload builds besides the record arrays: rtow_scene_upload builds everything (the scene stays
// resident for any later render); rtow_render / rtow_render_rgb8 know their config and build what its kernel reads
// kNeedBvh: the binary threaded image (BVH kernel); kNeedBvh4: the 4-wide image of a triangle mesh (BVH4 kernel) — a
// render that walks the one does not pay for the other (the 96.8k-triangle mesh: 20 ms of host work and 10 MB of
// upload less per rtow_render call)
constexpr unsigned kNeedBvh = 1u, kNeedGrid = 2u, kNeedF32 = 4u, kNeedBvh4 = 8u, kNeedAll = 15u;

struct rtow_ctx {
  int device = 0;
  Knobs knobs;
  int num_cus = 0;
  bool have_scene = false;
  rtow::DevScene ds{};
  rtow::DevCamera cam{};
  int n_prims = 0;
  // scene buffers
  DevBuf sph, sph_r, mov, tri, tri16, prim_mat, mats, blob, cam_dev, gblob;
  DevBuf blob4;                        // 4-wide BVH image (triangle meshes)
  bool have_bvh4 = false;
  bool have_tri16 = false;             // the STREAM kernel's 128-byte-stride triangle records are resident
  int bvh4_depth = 0;
  DevBuf blob32, gblob32, cam32_dev;  // the f32 build's scene images and camera
  rtow::DevScene ds32{};               // ds with the f32 images' pointers and offsets
  uint32_t gblob_bytes = 0;
  uint32_t grid_fat_stride = 0;  // bytes per fat cell-list entry of the resident grid image (0: plain id lists)
  int32_t grid_ny = 0;           // n[1] of the resident grid image's header (0: no grid); 1 selects the two-axis walk
  GridWalkConsts grid_walk{};    // the walk's constants from that header (rtow_walk_consts.h): TraceParams::walk
  int64_t last_spec = -1;        // TraceParams::spec of the last trace launch (rtow_debug_last_spec; -1: none yet)
  int last_counted = -1;         // whether that launch's kernel counted statistics (rtow_debug_last_counted; -1: none yet)
  bool have_grid = false;
  uint32_t blob_bytes = 0;
  long long bvh_nodes = 0;
  int builder = RTOW_BUILDER_HOST_SAH;      // the builder of the upload in progress / of the resident images
  int builder_req = RTOW_BUILDER_AUTO;      // what the caller asked for (rtow_ctx_set_builder, RTOW_BUILDER)
  void *lbvh_scratch = nullptr;  // device builder's buffers, kept across uploads
  void *grid_scratch = nullptr;
  rtow_build_info_t build_info{};
  // RTOW_KERNEL_REFTREE: the reference's own tree is built on first use from a host copy of the scene as uploaded
  struct HostSceneCopy {
    std::vector<double> sg, mg, tg;
    std::vector<int32_t> pk, pi;
    bool have_order = false;
    rtow_camera_t cam{};
  } host_scene;
  // Queue order of the 64-pixel tiles (tile_queue_table): device table, queue position of a tile -> tile, made by the
  // first render that needs it and kept while what it depends on stays: the resident scene (scene_gen counts uploads
  // and refits), the image size, this rank's strips, the tile shape and the ordering knobs.
  DevBuf tile_table;
  long long tile_key[10] = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t tile_empty = 0;       // tiles of the table's empty segment
  long long scene_gen = 0;
  DevBuf rtree;
  bool have_rtree = false;
  PinnedArena arena;     // staging of the scene uploads
  unsigned built = 0;    // kNeed* bits of what the resident scene holds (rtow_render uploads only what its kernel reads)
  // workspace
  DevBuf partials, stack, counters, spill;
  DevBuf out, out8;  // rtow_render / rtow_render_rgb8: device-side output of the host-buffer entry points
  // rtow_render_rgb8: the reduce kernel of the next single-launch render writes bytes here instead of sums
  unsigned char *fuse_rgb8 = nullptr;
  double fuse_spp = 0.0;
  bool fuse_used = false;
  DevBuf counters_init;  // what the 48 counters look like before a launch (one D2D copy instead of three memsets)
  // Samples given up at the end-of-launch bound (rtow_trace_body.h): a device word no launch resets, mirrored into
  // pinned memory behind every render; every entry point that waits for the device checks it (check_dropped)
  DevBuf dropped;
  unsigned long long *h_dropped = nullptr;
  hipEvent_t upload_ev = nullptr;  // recorded on the null stream behind the last copy / build kernel of a scene upload
  // launch shape per [precision][kernel-1]: blocks per CU (0 = not queried yet)
  int occ[3][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
  // profiling ring: event pairs around each trace-kernel launch since the last collect
  hipEvent_t ev[kEventRing][2] = {};
  int ev_count = 0;
  hipEvent_t call_ev[2] = {};
  // pinned host mirror of the counters for stats
  unsigned long long *h_counters = nullptr;
  // ray queries (rtow_intersect*, rtow_occluded*): counters, events, spill and staging of their own (a query never
  // touches the render's workspace, profile ring or dropped-sample word); the walk-id -> insertion-index tables are built
  // at the first closest-hit query that needs them after an upload (query_map)
  DevBuf q_counters, q_spill, q_rays, q_hits, q_occ, q_map[3];
  DevBuf q_stack, q_ids, q_rgb;  // rtow_radiance*: the strict build's path stack (sized per launch), the host form's staging
  DevBuf q_status;               // rtow_path_step: the host form's status words (its rays step in place in q_rays, its
                                 // attenuations and hits go through q_rgb and q_hits)
  DevBuf q_guides;               // rtow_guides: the host form's staging (rtow_camera_rays stages in q_rays / q_ids)
  DevBuf q_khits, q_kcounts;     // rtow_first_hits, rtow_nearest: the host forms' staging (their inputs go through q_rays)
  DevBuf q_ambient, q_ambient_rays;  // rtow_ambient: the host form's records and, when the caller asks for the sampled rays,
                                     // n x samples of them (its points and ids go through q_rays / q_ids)
  bool q_map_ok[3] = {false, false, false};
  hipEvent_t q_ev[4] = {};
  unsigned long long *h_qcounters = nullptr;
  // in-place refits (rtow_scene_refit, csrc/rtow_refit.hip).  What the first refit after an upload derives from the
  // images as built (before anything is overwritten) is kept until the next upload: the record slot -> triangle maps of
  // the leaf-ordered images, the parent links of both trees, the area sum of the binary BVH as uploaded.
  struct Refit {
    bool ready = false;                // the per-upload state below is derived
    std::vector<int32_t> slot2tri[2];  // [0] BVH image when ds.leaf_direct, [1] the 4-wide image (class-order triangle index)
    DevBuf map2, map4, par2, par4, need4, flags, nbox2, nbox4, sbox4, pbox, partials;
    DevBuf area;                       // [0] area sum of the upload's geometry, [1] of the last refit's; [2..7] 4-wide frame
    DevBuf g_sph, g_mov, g_tri;        // raw geometry, staged
    int refits = 0;
    double refit_ms = 0.0;
    hipEvent_t ev[2] = {};
  } rf;
};

// BVH4: stack entries per lane (4 B x 1024 lanes each) an image staged whole must leave room for (RTOW_BVH4_STACK_K)
// (round 5: 6, was 8 — suzanne's host tree walks at the same rate with 8, 7 and 6 entries per lane in LDS, and two more
// entry levels are 8 KB = 64 nodes of room for a mesh near the limit: the device-built suzanne tree, 276 nodes against
// the host's 261, is staged whole with 7)
inline uint32_t bvh4_min_stack(const rtow_ctx *c) { return c->knobs.bvh4_stack_k > 0 ? (uint32_t)c->knobs.bvh4_stack_k : 6u; }

// Launch shape of a strategy on the resident scene (shared by the render and the queries): workgroup size, LDS
// bytes and the DevScene fields that go with them (STREAM tiles; BVH4: what is staged, the stack's place and depth).
struct LaunchShape {
  rtow::DevScene scene;
  int block = 0;
  unsigned lds_bytes = 0;
  int stack_bound = 0;  // BVH4: traversal stack entries a lane may need (3 x depth + 1)
  bool image_kernel = false;
};

namespace rtow {
// the device builders' scratch, kept across uploads (csrc/rtow_build.hip, rtow_build_grid.hip): freed with the context
void lbvh_release(void *handle);
void grid_build_release(void *handle);
// ---- rtow_scene.cpp, for rtow_capi.cpp --------------------------------------------------------------------------------
int validate_scene(const rtow_scene_t *s);
int impl_scene_upload(rtow_ctx *c, const rtow_scene_t *s);
// Upload for ONE render whose config is known: only what its kernel reads
int upload_for(rtow_ctx *c, const rtow_scene_t *scene, const rtow_config_t *cfg);
int impl_scene_refit(rtow_ctx *c, const rtow_scene_t *s);
// Record slot of a leaf-ordered image -> class-order triangle index (which: 1 the host-built mesh BVH image, 2 the 4-wide image)
int match_slots(rtow_ctx *c, int which, std::vector<int32_t> &slot2tri);
// ---- rtow_capi.cpp, for rtow_queries.cpp ------------------------------------------------------------------------------
int validate_cfg(const rtow_config_t *cfg);
// The strategy a request resolves to, with the render's fallbacks and residency rules (shared by the render and the
// ray queries); the first RTOW_KERNEL_REFTREE request builds the reference's tree.
int resolve_kernel(rtow_ctx *c, int precision, int requested, int *out);
// The fallbacks and residency rules of a chosen strategy.  stream_records: BRUTE reads the STREAM kernel's triangle
// records (the render and the ray queries; the point queries read the class records every upload keeps).
int resident_kernel(rtow_ctx *c, int precision, int kernel, bool stream_records, int *out);
int launch_shape(rtow_ctx *c, int kernel, bool f32, LaunchShape &s);
}  // namespace rtow
using rtow::launch_shape;
using rtow::resident_kernel;
using rtow::resolve_kernel;
using rtow::validate_cfg;
using rtow::impl_scene_refit;
using rtow::impl_scene_upload;
using rtow::match_slots;
using rtow::upload_for;
using rtow::validate_scene;
