// rtow_capi.cpp — the C-ABI shim of include/rtow.h over the HIP kernels.
//
// One context = one HIP device.  The context owns the flattened scene in HBM,
// the workspace (per-stream partial images, per-lane path stack, counters) and a
// ring of event pairs that time every trace-kernel launch without a host sync.
// There is no CPU fallback: without a usable HIP device every entry point fails
// with RTOW_ENODEV / RTOW_EHIP.
//
// This file creates the context and renders the resident scene; what makes a scene resident (upload, refit, the
// diagnostics that read the images back) is rtow_scene.cpp, and every query over it is rtow_queries.cpp.  rtow_ctx.h is
// what the three share.

#include "rtow_ctx.h"

namespace {
thread_local std::string g_err;
}  // namespace
namespace rtow {
// for the other translation units of the library (rtow_queries.cpp, rtow_multi.cpp): same thread-local message
int set_last_error(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace rtow
namespace {

constexpr int kStreamTileMin = 64;  // STREAM kernel: from this many triangles on they are streamed through LDS tiles (below:
                                    //   scalar loads — the kernel's real use, scenes of <= 16 primitives)
constexpr int kBvhBlock = 512;   // BVH kernel workgroup (one LDS scene image per workgroup)

// magic/shift for fastdiv(): libdivide's branch-free u32 scheme
// q = (((n - t) >> 1) + t) >> shift with t = mulhi(n, magic)
rtow::FastDiv make_fastdiv(uint32_t d) {
  rtow::FastDiv f{0u, 0u};
  if (d <= 1) {  // identity: flagged with shift = 255
    f.shift = 255u;
    return f;
  }
  uint32_t fl = 31u - (uint32_t)__builtin_clz(d);
  if ((d & (d - 1)) == 0) {  // power of two: t = 0 would give n>>1>>(fl-1)
    f.magic = 0u;
    f.shift = fl - 1u;
    return f;
  }
  const uint64_t two = (uint64_t)1 << (32 + fl);
  uint64_t m = two / d;
  const uint64_t rem = two - m * d;
  // round up, doubled (the 33-bit magic's top bit is implicit in the (n-t)>>1 + t step)
  m = m * 2;
  const uint64_t twice_rem = rem * 2;
  if (twice_rem >= d || twice_rem < rem) m += 1;
  f.magic = (uint32_t)(m + 1);
  f.shift = fl;
  return f;
}

}  // namespace

extern "C" {

int rtow_abi_version(void) { return RTOW_ABI_VERSION; }

const char *rtow_last_error(void) { return g_err.c_str(); }

static int impl_ctx_create(int device_id, rtow_ctx **out) {
  if (!out) return fail(RTOW_EINVAL, "rtow_ctx_create: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(RTOW_ENODEV, "no HIP device (%s)", e == hipSuccess ? "count=0" : hipGetErrorString(e));
  if (device_id < 0 || device_id >= n) return fail(RTOW_ENODEV, "device %d out of range [0,%d)", device_id, n);
  HIPCHK(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_id));
  rtow_ctx *c = new rtow_ctx();
  c->device = device_id;
  c->num_cus = prop.multiProcessorCount;
  c->knobs.read();
  if (const char *e = std::getenv("RTOW_BUILDER"))
    c->builder_req = std::strcmp(e, "device") == 0 ? RTOW_BUILDER_DEVICE_LBVH
                     : std::strcmp(e, "auto") == 0 ? RTOW_BUILDER_AUTO : RTOW_BUILDER_HOST_SAH;
  c->builder = c->builder_req == RTOW_BUILDER_DEVICE_LBVH ? RTOW_BUILDER_DEVICE_LBVH : RTOW_BUILDER_HOST_SAH;
  // every failure below releases what was created so far (rtow_ctx_destroy skips null handles)
  hipError_t he = hipSuccess;
  for (int i = 0; i < kEventRing && he == hipSuccess; ++i)
    for (int k = 0; k < 2 && he == hipSuccess; ++k) he = hipEventCreate(&c->ev[i][k]);
  for (int k = 0; k < 2 && he == hipSuccess; ++k) he = hipEventCreate(&c->call_ev[k]);
  if (he == hipSuccess)
    he = hipHostMalloc((void **)&c->h_counters, 48 * sizeof(unsigned long long), hipHostMallocDefault);
  if (he == hipSuccess) he = hipHostMalloc((void **)&c->h_dropped, sizeof(unsigned long long), hipHostMallocDefault);
  if (he == hipSuccess) {
    *c->h_dropped = 0ull;
    he = hipEventCreateWithFlags(&c->upload_ev, hipEventDisableTiming);
  }
  if (he == hipSuccess && c->dropped.ensure(sizeof(unsigned long long)) != RTOW_OK) he = hipErrorOutOfMemory;
  if (he == hipSuccess) he = hipMemset(c->dropped.p, 0, sizeof(unsigned long long));
  if (he != hipSuccess) {
    rtow_ctx_destroy(c);
    return fail(RTOW_EHIP, "rtow_ctx_create: %s", hipGetErrorString(he));
  }
  *out = c;
  return RTOW_OK;
}

void rtow_ctx_destroy(rtow_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  for (DevBuf *b : {&c->sph, &c->sph_r, &c->mov, &c->tri, &c->tri16, &c->prim_mat, &c->mats, &c->blob, &c->cam_dev, &c->gblob,
                    &c->blob32, &c->gblob32, &c->cam32_dev, &c->blob4,
                    &c->partials, &c->stack, &c->counters, &c->spill, &c->out, &c->out8, &c->rtree, &c->counters_init,
                    &c->dropped, &c->q_counters, &c->q_spill, &c->q_rays, &c->q_hits, &c->q_occ, &c->q_map[0], &c->q_map[1],
                    &c->q_map[2], &c->q_stack, &c->q_ids, &c->q_rgb, &c->q_status, &c->q_guides, &c->q_khits, &c->q_kcounts,
                    &c->q_ambient, &c->q_ambient_rays,
                    &c->rf.map2, &c->rf.map4, &c->rf.par2, &c->rf.par4, &c->rf.need4, &c->rf.flags,
                    &c->rf.nbox2, &c->rf.nbox4, &c->rf.sbox4, &c->rf.pbox, &c->rf.partials, &c->rf.area, &c->rf.g_sph,
                    &c->rf.g_mov, &c->rf.g_tri, &c->tile_table})
    b->release();
  for (hipEvent_t e : c->rf.ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->q_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->h_qcounters) (void)hipHostFree(c->h_qcounters);
  if (c->h_dropped) (void)hipHostFree(c->h_dropped);
  if (c->upload_ev) (void)hipEventDestroy(c->upload_ev);
  if (c->arena.p) (void)hipHostFree(c->arena.p);
  for (int i = 0; i < kEventRing; ++i)
    for (int k = 0; k < 2; ++k)
      if (c->ev[i][k]) (void)hipEventDestroy(c->ev[i][k]);
  for (int k = 0; k < 2; ++k)
    if (c->call_ev[k]) (void)hipEventDestroy(c->call_ev[k]);
  if (c->h_counters) (void)hipHostFree(c->h_counters);
  rtow::lbvh_release(c->lbvh_scratch);
  rtow::grid_build_release(c->grid_scratch);
  // nothing of this context is pending in the runtime when the caller goes on (often: to exit())
  (void)hipDeviceSynchronize();
  delete c;
}

extern "C++" int rtow::validate_cfg(const rtow_config_t *cfg) {
  if (!cfg) return fail(RTOW_EINVAL, "config is NULL");
  if (cfg->image_width <= 0 || cfg->image_height <= 0)
    return fail(RTOW_EINVAL, "image size %dx%d", cfg->image_width, cfg->image_height);
  if (cfg->nstreams <= 0) return fail(RTOW_EINVAL, "nstreams must be >= 1");
  if (cfg->samples_per_pixel < 0 || cfg->max_child_rays < 0)
    return fail(RTOW_EINVAL, "negative samples_per_pixel / max_child_rays");
  if (cfg->nranks <= 0 || cfg->rank < 0 || cfg->rank >= cfg->nranks)
    return fail(RTOW_EINVAL, "rank %d of %d", cfg->rank, cfg->nranks);
  if (cfg->tile_rows <= 0) return fail(RTOW_EINVAL, "tile_rows must be >= 1");
  if (cfg->precision != RTOW_F64_STRICT && cfg->precision != RTOW_F64_FAST && cfg->precision != RTOW_F32)
    return fail(RTOW_EINVAL, "unknown precision %d", cfg->precision);
  if (cfg->kernel < RTOW_KERNEL_AUTO || cfg->kernel > RTOW_KERNEL_REFTREE)
    return fail(RTOW_EINVAL, "unknown kernel %d", cfg->kernel);
  if ((long long)cfg->image_width * cfg->image_height > 0x7fffffffLL)
    return fail(RTOW_EINVAL, "image too large");
  if (cfg->stream_first < 0 || cfg->stream_count < 0 ||
      (cfg->stream_count > 0 && cfg->stream_first + cfg->stream_count > cfg->nstreams) ||
      (cfg->stream_count == 0 && cfg->stream_first != 0))
    return fail(RTOW_EINVAL, "stream range [%d, %d+%d) outside [0, %d)", cfg->stream_first, cfg->stream_first,
                cfg->stream_count, cfg->nstreams);
  return RTOW_OK;
}

int rtow_ctx_set_builder(rtow_ctx *c, int32_t builder) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  if (builder != RTOW_BUILDER_HOST_SAH && builder != RTOW_BUILDER_DEVICE_LBVH && builder != RTOW_BUILDER_AUTO)
    return fail(RTOW_EINVAL, "unknown builder %d", builder);
  c->builder_req = builder;
  c->builder = builder == RTOW_BUILDER_DEVICE_LBVH ? RTOW_BUILDER_DEVICE_LBVH : RTOW_BUILDER_HOST_SAH;  // (AUTO without a config: host)
  return RTOW_OK;
}

int rtow_local_rows(const rtow_config_t *cfg) {
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  int rows = 0;
  for (int i = 0; i < cfg->image_height; ++i)
    if ((i / cfg->tile_rows) % cfg->nranks == cfg->rank) ++rows;
  return rows;
}

int rtow_local_row_list(const rtow_config_t *cfg, int32_t *rows_out, int32_t capacity) {
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  if (!rows_out && capacity > 0) return fail(RTOW_EINVAL, "rows_out is NULL");
  int n = 0;
  for (int i = 0; i < cfg->image_height; ++i)
    if ((i / cfg->tile_rows) % cfg->nranks == cfg->rank) {
      if (n < capacity) rows_out[n] = i;
      ++n;
    }
  return n;
}

// Levels: what one work item per pixel covers.  Strict build: a level is a stream, spp / nstreams samples summed
// in sample order, the partial images added in stream order — the reference's own decomposition
// (src/render.cpp:169-185), bit for bit.  Fast builds (tolerance builds: FMA contraction already re-associates):
// the SAME samples, cut into levels of a length that does not depend on nstreams — the divisor of the sample
// range nearest RTOW_SCHED_CHUNK (10, the measured optimum of the item length) — so Config::nthreads keeps its
// arithmetic meaning (which samples exist: spp / nthreads * nthreads) without setting the size of a work item: a
// drop-in caller with the reference's default of 4 threads (25 or 125 samples per stream) runs the items the
// bench runs.  The sum of a pixel is then the fixed-order sum of its level sums; the image is a pure function
// of (scene, config, seed) and of nothing else.
// (the item length aimed at depends on the class of the resident scene, not on anything else)
static int sched_chunk_for(const rtow_ctx *c) {
  const bool mesh = c->have_scene && c->ds.n_tri > 0 && c->ds.n_sph == 0 && c->ds.n_mov == 0;
  return mesh ? c->knobs.sched_chunk_mesh : c->knobs.sched_chunk;
}
struct LevelPlan {
  int spt;             // samples per level
  int first;           // index of the first level when the levels are the config's streams (strict build)
  int count;           // levels
  long long base;      // sample index of the first sample of level 0: level k covers [base + k * spt, ...)
  int last;            // samples of the LAST level (= spt, or spt <= last < 2 spt when the schedule is ragged)
  long long samples() const { return count > 0 ? (long long)(count - 1) * spt + last : 0; }
};
static LevelPlan level_plan(const rtow_config_t *cfg, int chunk) {
  const int spt = cfg->samples_per_pixel / cfg->nstreams;  // src/render.cpp:174
  const int streams_now = cfg->stream_count > 0 ? cfg->stream_count : cfg->nstreams;
  LevelPlan p{spt, cfg->stream_first, streams_now, (long long)cfg->stream_first * spt, spt};
  if (cfg->precision == RTOW_F64_STRICT || chunk <= 0 || spt <= 0) return p;
  // a level length d must divide the first sample index and the number of samples: any divisor of their gcd
  const long long s0 = (long long)cfg->stream_first * spt, total = (long long)streams_now * spt;
  long long g = total, r = s0;
  while (r) {
    const long long t = g % r;
    g = r;
    r = t;
  }
  long long best = 1;
  double best_err = 1e300;
  for (long long d = 1; d * d <= g; ++d) {
    if (g % d) continue;
    for (long long e : {d, g / d}) {
      const double err = std::fabs(std::log((double)e / (double)chunk));
      if (err < best_err - 1e-12 || (std::fabs(err - best_err) <= 1e-12 && e < best)) {
        best_err = err;
        best = e;
      }
    }
  }
  if (2 * best < chunk || best > 2LL * chunk) {
    // No divisor within a factor of two of the aimed-at length (a prime sample count: 101 would be 101 levels of
    // one sample — 101 work items and 101 partial images per pixel — or one level of 101).  Ragged schedule
    // instead: levels of `chunk` samples from the first sample on, the remainder added to the LAST level
    // (chunk <= last < 2 chunk; a range shorter than a chunk is one level).  Still a pure function of the config.
    const long long n = std::max<long long>(total / chunk, 1);
    if (n > 0x7fffffffLL) return p;
    p.spt = n > 1 ? chunk : (int)total;
    p.count = (int)n;
    p.last = (int)(total - (n - 1) * (long long)p.spt);
    p.base = s0;
    p.first = 0;
    return p;
  }
  if (total / best > 0x7fffffffLL || best > 0x7fffffffLL) return p;
  p.spt = (int)best;
  p.first = (int)(s0 / best);
  p.count = (int)(total / best);
  p.last = p.spt;
  p.base = s0;
  return p;
}

// (diagnostic / tests) the levels a render of `cfg` is cut into: pairs (first sample, count).  ctx may be NULL.
static int impl_debug_schedule(rtow_ctx *c, const rtow_config_t *cfg, uint32_t *out, int32_t capacity_pairs) {
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  Knobs defaults;  // ctx NULL: the defaults of a new context (pure host arithmetic, usable without a GPU)
  if (!c) defaults.read();
  const LevelPlan p = level_plan(cfg, c ? sched_chunk_for(c) : defaults.sched_chunk);
  for (int i = 0; i < p.count && i < capacity_pairs && out; ++i) {
    out[2 * i] = (uint32_t)(p.base + (long long)i * p.spt);
    out[2 * i + 1] = (uint32_t)(i + 1 == p.count ? p.last : p.spt);
  }
  return p.count;
}

// 64-pixel tiles of the queue order: 8x8, 16x4 or 32x2 — the tallest that divides the strip height, this rank's
// rows and the image width (a tile never straddles two strips); 0, 0 = plain row-major order
static void tile_shape(const rtow_config_t *cfg, int rows, uint32_t &th, uint32_t &tw) {
  th = tw = 0;
  for (uint32_t h : {3u, 2u, 1u}) {
    const uint32_t hh = 1u << h, ww = 64u >> h;
    if (cfg->tile_rows % hh == 0 && rows % (int)hh == 0 && cfg->image_width % (int)ww == 0) {
      th = h;
      tw = 6u - h;
      return;
    }
  }
}

// ---- queue order of the tiles ------------------------------------------------------------------------------------
// Which of this rank's 64-pixel tiles are EMPTY: no ray the camera can generate through any of their pixels — the whole
// jitter square of every pixel, the whole lens disk, for a moving sphere the whole shutter interval — can reach any
// primitive.  Every sample of such a tile is exactly one segment (the sky), so the work is cheap, uniform and cannot
// start a long path: the queue ends on it (tile_queue_table).  A hint only: it decides when a tile is traced, never
// what is rendered, and errs to "not empty" — a camera frame that is not the reference's (horizontal along u, vertical
// along v, the viewport straight ahead), a primitive around the lens: nothing is empty.
//   * A primitive is its bounding sphere (c, r): a sphere itself, the ball swept by a moving sphere between the
//     shutter's ends (centre c0 + t (c1 - c0), t in [t0, t1]), the ball around a triangle's box centre through its vertices.
//   * The lens is folded into the radius.  A ray from the lens point o' (|o' - o| <= lens) through the viewport point
//     P is, at the parameter s where it has depth z = s fd, the pinhole ray o -> P displaced by (o' - o)(1 - s): by at
//     most lens for z <= 2 fd and lens (z / fd - 1) beyond.  The ray enters the sphere at a depth z_max or less (see
//     below), so if the lens ray meets the sphere, the pinhole ray through the same viewport point meets the sphere
//     of radius R = r + lens max(1, z_max / fd - 1).  From here on only pinhole rays and inflated spheres.
//   * A tile is the cone around the direction through its centre that holds the directions through all of its
//     jittered pixel positions: columns [j0, j0 + tw] / (W - 1), rows [H - i0 - th, H - i0] / (H - 1) of the viewport,
//     half-angle asin(half diagonal / distance of the centre).  It can see the sphere when the angle between the two
//     axes is at most asin(R / |c - o|) + that half-angle.  Per sphere the test runs over the tiles of its screen
//     rectangle only (the tangents from the eye to its outline in the camera's two axis planes), so the cost is a
//     few dozen operations per sphere and tile it may touch.  Radii and half-angles carry a relative slack of 1e-6:
//     far above the rounding of this arithmetic and of the binary32 build's rays, far below a pixel.
static void tile_classify(const rtow_ctx::HostSceneCopy &h, const rtow_config_t *cfg, uint32_t th, uint32_t tw, int rows,
                          std::vector<unsigned char> &empty) {
  const uint32_t tpr = (uint32_t)cfg->image_width >> tw, ntr = (uint32_t)rows >> th, nt = tpr * ntr;
  empty.assign(nt, 0);
  const rtow_camera_t &cam = h.cam;
  const int W = cfg->image_width, H = cfg->image_height;
  if (W < 2 || H < 2 || nt == 0) return;
  auto dot3 = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  const double lenH = std::sqrt(dot3(cam.horizontal, cam.horizontal)), lenV = std::sqrt(dot3(cam.vertical, cam.vertical));
  double mid[3];
  for (int k = 0; k < 3; ++k) mid[k] = cam.lower_left_corner[k] + 0.5 * cam.horizontal[k] + 0.5 * cam.vertical[k] - cam.origin[k];
  const double fd = -dot3(mid, cam.w);  // the viewport lies fd along -w
  const double lens = std::fabs(cam.lens_radius);
  if (!(lenH > 0.0 && lenV > 0.0 && fd > 0.0) || !std::isfinite(lenH + lenV + fd + lens)) return;
  {  // the frame the rectangles below assume
    const double tol = 1e-9;
    bool ok = std::fabs(dot3(cam.u, cam.u) - 1.0) < tol && std::fabs(dot3(cam.v, cam.v) - 1.0) < tol &&
              std::fabs(dot3(cam.w, cam.w) - 1.0) < tol && std::fabs(dot3(cam.u, cam.v)) < tol &&
              std::fabs(dot3(cam.u, cam.w)) < tol && std::fabs(dot3(cam.v, cam.w)) < tol;
    ok = ok && std::fabs(dot3(cam.horizontal, cam.u) - lenH) < tol * lenH && std::fabs(dot3(cam.vertical, cam.v) - lenV) < tol * lenV;
    ok = ok && std::fabs(dot3(mid, cam.u)) < tol * fd && std::fabs(dot3(mid, cam.v)) < tol * fd;
    if (!ok) return;
  }
  std::vector<int32_t> row_list((size_t)rows);
  rtow_local_row_list(cfg, row_list.data(), rows);
  const double wm = (double)(W - 1), hm = (double)(H - 1);
  const double tile_w = (double)(1u << tw), tile_h = (double)(1u << th);
  // per tile row / column: the viewport interval it covers; per tile: unit axis and sine / cosine of the half-angle
  std::vector<double> v_lo(ntr), v_hi(ntr), axis((size_t)nt * 3), sin_b(nt), cos_b(nt);
  const double half_diag = 0.5 * std::sqrt(tile_w * tile_w * lenH * lenH / (wm * wm) + tile_h * tile_h * lenV * lenV / (hm * hm));
  for (uint32_t tr = 0; tr < ntr; ++tr) {
    const double i0 = (double)row_list[(size_t)tr << th];  // (a tile never straddles two strips: its rows are consecutive)
    v_lo[tr] = ((double)H - i0 - tile_h) / hm;
    v_hi[tr] = ((double)H - i0) / hm;
    for (uint32_t tc = 0; tc < tpr; ++tc) {
      const double sc = ((double)tc + 0.5) * tile_w / wm, vc = 0.5 * (v_lo[tr] + v_hi[tr]);
      double d[3];
      for (int k = 0; k < 3; ++k) d[k] = cam.lower_left_corner[k] + sc * cam.horizontal[k] + vc * cam.vertical[k] - cam.origin[k];
      const double dl = std::sqrt(dot3(d, d));
      const size_t t = (size_t)tr * tpr + tc;
      for (int k = 0; k < 3; ++k) axis[3 * t + k] = d[k] / dl;
      const double sb = std::min(half_diag / dl * (1.0 + 1e-6) + 1e-9, 1.0);
      sin_b[t] = sb;
      cos_b[t] = std::sqrt(1.0 - sb * sb);
    }
  }
  std::vector<unsigned char> seen(nt, 0);
  bool all = false;
  // tangent slopes x / z from the eye to the disc (p, z; R) of one axis plane, as viewport coordinates
  auto extent = [](double p, double z, double R, double scale, double &lo, double &hi) {
    lo = -1e300;
    hi = 1e300;
    if (!(z > R)) return;  // the disc reaches the lens plane: every coordinate
    const double q = std::sqrt(std::max(p * p + z * z - R * R, 0.0));
    lo = 0.5 + (p * q - R * z) / (z * q + p * R) * scale;
    hi = 0.5 + (p * q + R * z) / (z * q - p * R) * scale;
  };
  auto mark = [&](const double *cc, double r) {
    if (all) return;
    if (!std::isfinite(cc[0] + cc[1] + cc[2] + r)) {
      all = true;
      return;
    }
    double rel[3];
    for (int k = 0; k < 3; ++k) rel[k] = cc[k] - cam.origin[k];
    const double px = dot3(rel, cam.u), py = dot3(rel, cam.v), pz = -dot3(rel, cam.w);
    r = std::fabs(r);
    const double dist = std::sqrt(dot3(rel, rel));
    if (!(dist - lens > r)) {  // the lens reaches into the sphere: everything
      all = true;
      return;
    }
    // depth of the point where a lens ray enters the sphere: at most the far side, and at most the tangent length
    // from the lens point (entry x exit = the power of the point, entry <= exit) — what keeps the ground in bounds
    const double z_max = std::min(pz + r, std::sqrt((dist + lens) * (dist + lens) - r * r));
    double R = r + lens * std::max(1.0, z_max / fd - 1.0);
    R = R * (1.0 + 1e-6) + 1e-9;
    if (pz + R <= 0.0) return;  // wholly behind the lens plane: every camera ray runs forward
    if (!(dist > R)) {  // the eye is inside the inflated sphere: everything
      all = true;
      return;
    }
    double s0, s1, t0, t1;
    extent(px, pz, R, fd / lenH, s0, s1);
    extent(py, pz, R, fd / lenV, t0, t1);
    const double c0 = std::floor(s0 * wm / tile_w) - 1.0, c1 = std::floor(s1 * wm / tile_w) + 1.0;
    if (c1 < 0.0 || c0 > (double)(tpr - 1u)) return;
    const uint32_t ca = (uint32_t)std::max(c0, 0.0), cb = (uint32_t)std::min(c1, (double)(tpr - 1u));
    const double pad = tile_h / hm;  // (one tile of margin, as for the columns: the cone test decides)
    const double sa = R / dist, csa = std::sqrt(1.0 - sa * sa);
    const double ax[3] = {rel[0] / dist, rel[1] / dist, rel[2] / dist};
    for (uint32_t tr = 0; tr < ntr; ++tr) {
      if (v_hi[tr] + pad < t0 || v_lo[tr] - pad > t1) continue;
      for (uint32_t tc = ca; tc <= cb; ++tc) {
        const size_t t = (size_t)tr * tpr + tc;
        if (seen[t]) continue;
        // angle between the axes <= alpha + beta (both below a right angle)
        const double cos_reach = csa * cos_b[t] - sa * sin_b[t];
        if (dot3(&axis[3 * t], ax) >= cos_reach) seen[t] = 1;
      }
    }
  };
  for (size_t i = 0; i < h.sg.size() / 4; ++i) mark(&h.sg[4 * i], h.sg[4 * i + 3]);
  for (size_t i = 0; i < h.mg.size() / 8; ++i) {
    const double *m = &h.mg[8 * i];  // c0 xyz, c1 xyz, r: centre c0 + t (c1 - c0) for t in the shutter interval
    double a[3], b[3], mc[3], dd = 0.0;
    for (int k = 0; k < 3; ++k) {
      a[k] = m[k] + cam.t0 * (m[3 + k] - m[k]);
      b[k] = m[k] + cam.t1 * (m[3 + k] - m[k]);
      mc[k] = 0.5 * (a[k] + b[k]);
      dd += (b[k] - a[k]) * (b[k] - a[k]);
    }
    mark(mc, std::fabs(m[6]) + 0.5 * std::sqrt(dd));
  }
  for (size_t i = 0; i < h.tg.size() / 9; ++i) {
    const double *g = &h.tg[9 * i];
    double mc[3], rr = 0.0;
    for (int k = 0; k < 3; ++k)
      mc[k] = 0.5 * (std::min(g[k], std::min(g[3 + k], g[6 + k])) + std::max(g[k], std::max(g[3 + k], g[6 + k])));
    for (int q = 0; q < 3; ++q) {
      double d2 = 0.0;
      for (int k = 0; k < 3; ++k) d2 += (g[3 * q + k] - mc[k]) * (g[3 * q + k] - mc[k]);
      rr = std::max(rr, d2);
    }
    mark(mc, std::sqrt(rr));
  }
  if (all) return;
  for (uint32_t t = 0; t < nt; ++t) empty[t] = !seen[t];
}

// table[queue position of a tile] = tile (row-major over this rank's tile rows).  The queue is consumed from its far
// end, so position 0 runs LAST.  Two segments: the empty tiles (tile_classify) at positions [0, n_empty), everything
// else above them; inside each the row order that was the whole order before — the rows below the top band top-down
// first (the horizon rows of an outdoor scene, its costliest), the top band (sky_rows tile rows) last — so a scene
// with no empty tile, or `ordered` false (RTOW_TILE_ORDER=0), runs exactly as it did.
static uint32_t tile_queue_table(const std::vector<unsigned char> &empty, bool ordered, uint32_t tpr, uint32_t ntr,
                                 uint32_t sky_rows, std::vector<uint32_t> &table) {
  const uint32_t nt = tpr * ntr;
  table.resize(nt);
  uint32_t n_empty = 0;
  if (ordered)
    for (uint32_t t = 0; t < nt; ++t) n_empty += empty[t] ? 1u : 0u;
  uint32_t pe = 0, pf = n_empty;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t trq = t / tpr, tc = t - trq * tpr;
    const uint32_t tr = trq >= sky_rows ? sky_rows + (ntr - 1u - trq) : trq;
    const uint32_t tile = tr * tpr + tc;
    if (ordered && empty[tile])
      table[pe++] = tile;
    else
      table[pf++] = tile;
  }
  return n_empty;
}

static int render_levels(rtow_ctx *c, const rtow_config_t *cfg, void *d_rgb_sums, void *hip_stream,
                         rtow_stats_t *stats, const LevelPlan &plan, int lvl_first, int lvl_count, int accumulate);

// Samples given up at the end-of-launch bound are an ERROR, never a darker image: the kernels count them in a device
// word no launch resets.  Entry points that wait for the device anyway read it: `mirrored` = the word was copied to
// c->h_dropped by a copy queued behind the render on a stream the caller has since waited for; otherwise it is read
// with a blocking copy (the launches in question must have completed).
static int check_dropped(rtow_ctx *c, bool mirrored) {
  unsigned long long v = 0ull;
  if (mirrored)
    v = *c->h_dropped;
  else
    HIPCHK(hipMemcpy(&v, c->dropped.p, sizeof v, hipMemcpyDeviceToHost));
  if (v == 0ull) return RTOW_OK;
  *c->h_dropped = 0ull;
  HIPCHK(hipMemset(c->dropped.p, 0, sizeof v));
  return fail(RTOW_EHIP, "trace kernel: end-of-launch bound reached, %llu lanes gave up their samples", v);
}
static int mirror_dropped(rtow_ctx *c, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(c->h_dropped, c->dropped.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  return RTOW_OK;
}

static int impl_render_device(rtow_ctx *c, const rtow_config_t *cfg, void *d_rgb_sums, void *hip_stream,
                       rtow_stats_t *stats) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  if (!c->have_scene) return fail(RTOW_ENOSCENE, "no scene uploaded");
  if (!d_rgb_sums) return fail(RTOW_EINVAL, "d_rgb_sums is NULL");
  HIPCHK(hipSetDevice(c->device));

  const int rows = rtow_local_rows(cfg);
  const int spt = cfg->samples_per_pixel / cfg->nstreams;  // src/render.cpp:174
  const unsigned long long npix = (unsigned long long)rows * cfg->image_width;
  const int streams_now = cfg->stream_count > 0 ? cfg->stream_count : cfg->nstreams;
  if ((unsigned long long)spt * (unsigned long long)(cfg->stream_first + streams_now) > 0xffffffffULL)
    return fail(RTOW_EINVAL, "sample index beyond 32 bits");
  const LevelPlan plan = level_plan(cfg, sched_chunk_for(c));
  const int n_levels = plan.count;
  // Large sample counts: the per-level partial sums (24 B per pixel and level) are bounded by tracing the
  // levels in ranges that accumulate onto d_rgb_sums — bit-identical to one launch (the reduce kernel adds
  // level sums in level order either way).
  unsigned long long max_levels = (unsigned long long)n_levels;
  if (npix > 0) {
    max_levels = c->knobs.partials_cap / (npix * 24ull);
    if (0xfffffff0ULL / npix < max_levels) max_levels = 0xfffffff0ULL / npix;  // 32-bit item index
    if (max_levels < 1) max_levels = 1;
  }
  if ((unsigned long long)n_levels <= max_levels || spt == 0 || npix == 0)
    return render_levels(c, cfg, d_rgb_sums, hip_stream, stats, plan, 0, n_levels, cfg->accumulate);
  rtow_stats_t total;
  std::memset(&total, 0, sizeof total);
  for (int done = 0; done < n_levels;) {
    const int now = (int)std::min<unsigned long long>(max_levels, (unsigned long long)(n_levels - done));
    rtow_stats_t st1;
    rc = render_levels(c, cfg, d_rgb_sums, hip_stream, stats ? &st1 : nullptr, plan, done, now,
                       (done > 0 || cfg->accumulate) ? 1 : 0);
    if (rc) return rc;
    if (stats) {
      total.samples += st1.samples;
      total.segments += st1.segments;
      total.prim_tests += st1.prim_tests;
      total.node_tests += st1.node_tests;
      total.kernel_ms += st1.kernel_ms;
      total.total_ms += st1.total_ms;
      total.local_rows = st1.local_rows;
      total.kernel_used = st1.kernel_used;
    }
    done += now;
  }
  if (stats) *stats = total;
  return RTOW_OK;
}

// The strategy RTOW_KERNEL_AUTO stands for in a render of the resident scene (and in the ray queries).
static int auto_kernel(const rtow_ctx *c, int precision) {
  // AUTO: a handful of primitives is cheaper to stream than to walk; sphere scenes walk the
  // grid (measured 1.3x the BVH on the cover scene); triangle meshes walk the BVH (a triangle
  // spans many cells and its test is 3.5x a sphere's, so duplicates are expensive: 0.4x)
  const bool bvh4_ok = c->have_bvh4 && precision != RTOW_F32;  // triangle mesh, host builder, binary64 build
  return c->n_prims <= 16 ? RTOW_KERNEL_BRUTE
         : (c->have_grid && c->ds.n_tri == 0) ? RTOW_KERNEL_GRID
         : bvh4_ok ? RTOW_KERNEL_BVH4 : RTOW_KERNEL_BVH;
}

// The strategy a request resolves to, with the render's fallbacks and residency rules (shared by the render and the
// ray queries); the first RTOW_KERNEL_REFTREE request builds the reference's tree.
extern "C++" int rtow::resolve_kernel(rtow_ctx *c, int precision, int requested, int *out) {
  return resident_kernel(c, precision, requested == RTOW_KERNEL_AUTO ? auto_kernel(c, precision) : requested, true, out);
}

// The fallbacks and residency rules of a chosen strategy.  stream_records: BRUTE reads the STREAM kernel's triangle
// records (the render and the ray queries; the point query reads the class records every upload keeps).
extern "C++" int rtow::resident_kernel(rtow_ctx *c, int precision, int kernel, bool stream_records, int *out) {
  const bool strict = precision == RTOW_F64_STRICT;
  const bool f32 = precision == RTOW_F32;
  const bool bvh4_ok = c->have_bvh4 && !f32;  // triangle mesh, host builder, binary64 build
  if (kernel == RTOW_KERNEL_GRID && !c->have_grid) kernel = RTOW_KERNEL_BVH;  // scene not suited to a grid
  if (kernel == RTOW_KERNEL_BRUTE && stream_records && c->ds.n_tri > 0 && !c->have_tri16)
    return fail(RTOW_ENOSCENE, "the resident scene was uploaded for another kernel (the STREAM kernel's triangle records are "
                               "missing): call rtow_scene_upload");
  if (kernel == RTOW_KERNEL_BVH4 && !bvh4_ok) kernel = RTOW_KERNEL_BVH;
  if ((kernel == RTOW_KERNEL_BVH && !(c->built & kNeedBvh)) || (f32 && !(c->built & kNeedF32)))
    return fail(RTOW_ENOSCENE, "the resident scene was uploaded by rtow_render for another kernel / precision: "
                               "call rtow_scene_upload before rtow_render_device");
  if (kernel == RTOW_KERNEL_REFTREE) {
    // the reference's own tree and box test: an exactness mode, so it exists in the strict build only
    if (!strict) return fail(RTOW_EINVAL, "RTOW_KERNEL_REFTREE needs precision RTOW_F64_STRICT");
    if (!c->have_rtree) {
      rtow_scene_t hs;
      std::memset(&hs, 0, sizeof hs);
      const rtow_ctx::HostSceneCopy &h = c->host_scene;
      hs.n_spheres = c->ds.n_sph;
      hs.n_moving = c->ds.n_mov;
      hs.n_triangles = c->ds.n_tri;
      hs.n_prims = c->n_prims;
      hs.sphere_geom = h.sg.data();
      hs.moving_geom = h.mg.data();
      hs.triangle_geom = h.tg.data();
      hs.prim_kind = h.have_order ? h.pk.data() : nullptr;
      hs.prim_index = h.have_order ? h.pi.data() : nullptr;
      rtow::RefTree rt;
      const double t0 = now_ms();
      rtow::build_reftree(&hs, rt);
      if (!rt.ok) return fail(RTOW_EINVAL, "reference tree: depth %d exceeds the kernel's stack", rt.depth);
      if (int rc = upload(c->rtree, rt.blob)) return rc;
      c->ds.rtree = (const unsigned char *)c->rtree.p;
      c->ds.rt_off_ids = rt.off_ids;
      c->have_rtree = true;
      c->build_info.ref_tree_nodes = rt.n_nodes;
      c->build_info.ref_tree_stupid_volume = rt.stupid_volume;
      c->build_info.ref_tree_build_ms = now_ms() - t0;
    }
  }
  *out = kernel;
  return RTOW_OK;
}

// Launch shape of a strategy on the resident scene (LaunchShape, rtow_ctx.h; shared by the render and the queries).
extern "C++" int rtow::launch_shape(rtow_ctx *c, int kernel, bool f32, LaunchShape &s) {
  s.scene = f32 ? c->ds32 : c->ds;
  rtow::DevScene &scene = s.scene;
  int &block = s.block;
  block = (kernel >= RTOW_KERNEL_BVH && kernel <= RTOW_KERNEL_BVH4) ? kBvhBlock : kBlock;
  const bool image_kernel = s.image_kernel = kernel >= RTOW_KERNEL_BVH && kernel <= RTOW_KERNEL_BVH4;
  if (image_kernel && c->knobs.bvh_block) block = c->knobs.bvh_block;  // experiment knob
  // the scene image goes to LDS when one copy per workgroup fits (160 KiB per CU)
  const uint32_t image_bytes = kernel == RTOW_KERNEL_GRID ? scene.gblob_bytes : scene.blob_bytes;
  // an image too big for two workgroups per CU: ONE 1024-lane workgroup (16 waves, the same 4 per SIMD)
  // instead of one 512-lane workgroup (2 per SIMD)
  if (image_kernel && block == kBvhBlock && image_bytes <= kLdsLimit && 2u * image_bytes > kLdsLimit &&
      !c->knobs.bvh_block)
    block = 1024;
  unsigned &lds_bytes = s.lds_bytes;
  lds_bytes = (image_kernel && image_bytes <= kLdsLimit) ? image_bytes : 0u;
  scene.stream_tile_lds = 0u;
  if (kernel == RTOW_KERNEL_BRUTE && scene.n_tri >= kStreamTileMin && !c->knobs.stream_scalar) {
    // the tiled triangle loop of the STREAM kernel (csrc/rtow_trace_hit.h): two 3 KB tiles of LDS per wave
    scene.stream_tile_lds = 2u * 32u * 96u;
    lds_bytes = (unsigned)(block / 64) * scene.stream_tile_lds;
  }
  int &stack_bound = s.stack_bound;
  stack_bound = 0;
  if (kernel == RTOW_KERNEL_BVH4) {
    // One 1024-lane workgroup per CU.  LDS = [image, or the top of its tree][stack: K entries x 4 B per lane].
    // A small mesh is staged whole and the stack takes what is left (at least 8 entries per lane);
    // a big one gets 24 stack entries per lane and as many breadth-first nodes as fit beside them.
    block = 1024;
    const uint32_t per_entry = 4u * (uint32_t)block;
    stack_bound = 3 * c->bvh4_depth + 1;
    uint32_t K, staged, aux_src = scene.blob4_bytes, aux_bytes = 0u;
    const uint32_t min_k = bvh4_min_stack(c);
    const uint32_t node_bytes = scene.b4_half ? rtow::kBvh4HalfNodeBytes : rtow::kBvh4NodeBytes;
    if (!scene.b4_half && scene.blob4_bytes + min_k * per_entry <= kLdsLimit) {
      staged = scene.blob4_bytes;
      K = std::min<uint32_t>((kLdsLimit - staged) / per_entry, 32u);
      if (c->knobs.bvh4_stack_k > 0) K = std::min<uint32_t>(K, (uint32_t)c->knobs.bvh4_stack_k);  // (experiments: fewer)
    } else if (!scene.b4_half) {
      return fail(RTOW_EINVAL, "internal error: a 4-wide image with binary32 nodes must fit LDS whole");
    } else {
      // (stack entries 6 / 8 / 10 / 12 / 16 / 24 on the 96.8k-triangle mesh: 2.07 / 2.12 / 2.12 / 2.11 / 2.10 / 2.10
      // Gsamples/s — what the stack does not need holds 128-byte nodes)
      K = c->knobs.bvh4_stack_k > 0 ? std::min<uint32_t>((uint32_t)c->knobs.bvh4_stack_k, 32u) : 10u;
      // the end of the image goes to LDS as well when it is small: materials + material indices, or the
      // materials alone (shading reads index -> material after every hit: two dependent L2 round trips otherwise)
      const uint32_t aux_max = c->knobs.bvh4_no_aux ? 0u : 16u * 1024u;
      if (scene.blob4_bytes - scene.b4_off_pmat <= aux_max)
        aux_src = scene.b4_off_pmat;
      else if (scene.blob4_bytes - scene.b4_off_mats <= aux_max)
        aux_src = scene.b4_off_mats;
      aux_bytes = scene.blob4_bytes - aux_src;
      staged = std::min<uint32_t>((kLdsLimit - K * per_entry - aux_bytes) / node_bytes * node_bytes, scene.b4_off_tri);
    }
    K = std::min<uint32_t>(K, (uint32_t)stack_bound);
    scene.b4_lds_limit = staged;
    scene.b4_aux_src = aux_src;
    scene.b4_aux_lds = (staged + 15u) / 16u * 16u;
    scene.b4_stack_base = (scene.b4_aux_lds + aux_bytes + 15u) / 16u * 16u;
    scene.b4_stack_k = K;
    lds_bytes = scene.b4_stack_base + K * per_entry;
  }
  return RTOW_OK;
}

// One launch: levels [lvl_first, lvl_first + lvl_count) of the plan.
static int render_levels(rtow_ctx *c, const rtow_config_t *cfg, void *d_rgb_sums, void *hip_stream,
                         rtow_stats_t *stats, const LevelPlan &plan, int lvl_first, int lvl_count, int accumulate) {
  int rc;
  hipStream_t st = (hipStream_t)hip_stream;
  const int rows = rtow_local_rows(cfg);
  const unsigned long long npix = (unsigned long long)rows * cfg->image_width;
  const int streams_now = lvl_count;  // levels of this launch
  const int spt = plan.spt;
  const int spt_last = lvl_first + lvl_count == plan.count ? plan.last : plan.spt;  // (a ragged schedule ends on a longer level)
  const unsigned long long n_items = npix * (unsigned long long)streams_now;
  if (n_items > 0xfffffff0ULL) return fail(RTOW_EINVAL, "too many work items (%llu)", n_items);
  int kernel = 0;
  if ((rc = resolve_kernel(c, cfg->precision, cfg->kernel, &kernel))) return rc;
  const bool strict = cfg->precision == RTOW_F64_STRICT;
  const bool f32 = cfg->precision == RTOW_F32;
  LaunchShape shape;
  if ((rc = launch_shape(c, kernel, f32, shape))) return rc;
  rtow::DevScene &scene = shape.scene;
  const int block = shape.block;
  const unsigned lds_bytes = shape.lds_bytes;
  const int stack_bound = shape.stack_bound;
  const bool image_kernel = shape.image_kernel;

  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->local_rows = rows;
    stats->kernel_used = kernel;
  }
  if (npix == 0) return RTOW_OK;
  if (spt == 0) {
    // fewer samples than streams: zero effective samples (src/render.cpp:174), black sums
    if (!accumulate) HIPCHK(hipMemsetAsync(d_rgb_sums, 0, (size_t)npix * 3 * sizeof(double), st));
    if (stats) HIPCHK(hipStreamSynchronize(st));
    return RTOW_OK;
  }

  // grid: as many 256-lane blocks as stay resident, but no more than there are items
  int &occ = c->occ[strict ? 0 : (f32 ? 2 : 1)][kernel - 1];
  if (kernel == RTOW_KERNEL_BVH4) occ = 0;  // its LDS footprint depends on the scene: query every time (cheap)
  if (occ <= 0) {
    occ = strict ? rtow::trace_occupancy_strict(kernel, block, lds_bytes)
          : f32  ? rtow::trace_occupancy_f32(kernel, block, lds_bytes)
                 : rtow::trace_occupancy_fast(kernel, block, lds_bytes);
    if (occ <= 0) return fail(RTOW_EHIP, "occupancy query failed (kernel %d, %u B of LDS)", kernel, lds_bytes);
    if (occ > 8) occ = 8;
    if (c->knobs.blocks_per_cu) occ = c->knobs.blocks_per_cu;  // experiment knob
  }
  long long grid = (long long)c->num_cus * occ;
  const long long need_blocks = (long long)((n_items + block - 1) / block);
  if (grid > need_blocks) grid = need_blocks;
  if (grid < 1) grid = 1;
  const unsigned long long n_lanes = (unsigned long long)grid * block;

  const size_t depth_slots = (size_t)(cfg->max_child_rays > 0 ? cfg->max_child_rays : 1);
  if ((rc = c->partials.ensure((size_t)n_items * 3 * sizeof(double))) ||
      (rc = c->stack.ensure(strict ? depth_slots * (size_t)n_lanes * sizeof(uint32_t) : 4)) ||  // strict build only
      (rc = c->counters.ensure(48 * sizeof(unsigned long long))))
    return rc;
  if (kernel == RTOW_KERNEL_BVH4) {
    const int extra = std::max(stack_bound - (int)scene.b4_stack_k, 0);
    if ((rc = c->spill.ensure(std::max<size_t>((size_t)extra * (size_t)n_lanes * sizeof(uint32_t), 16)))) return rc;
  }

#ifdef RTOW_TAILSTAT  // (experiment build, scripts/tailstat.py; sphere scenes only: the BVH4 kernel needs its spill array itself)
  if (kernel == RTOW_KERNEL_BVH4) return fail(RTOW_EINVAL, "RTOW_TAILSTAT builds do not run the BVH4 kernel");
  if ((rc = c->spill.ensure(std::max<size_t>((size_t)n_lanes, 16)))) return rc;  // 8 words of 8 bytes per wave
#endif
  rtow::TraceParams P;
  std::memset(&P, 0, sizeof P);
  P.sc = scene;
  P.cam = (const rtow::DevCamera *)c->cam_dev.p;
  P.cam32 = (const float *)c->cam32_dev.p;
  P.W = cfg->image_width;
  P.H = cfg->image_height;
  P.spt = spt;
  P.nstreams = streams_now;
  P.stream_first = plan.first + lvl_first;
  P.sample_base = (uint32_t)(plan.base + (long long)lvl_first * spt);
  P.spt_last = spt_last;
  {
    // structural bound of the end-of-launch protocol (rtow_trace_body.h): x64 because a stopped-and-resumed walk
    // spreads one segment over several trips
    const unsigned long long b = 64ull * (4096ull + 8ull * (unsigned long long)(cfg->max_child_rays + 2) *
                                                        (unsigned long long)(std::max(spt, spt_last) + 1));
    P.tail_bound = c->knobs.tail_bound > 0 ? (uint32_t)c->knobs.tail_bound : (uint32_t)std::min<unsigned long long>(b, 0xfffffff0ull);
  }
  P.dropped = (unsigned long long *)c->dropped.p;
  P.inv_wm1 = 1.0 / (double)(cfg->image_width - 1);  // (W = 1: inf, and the fast build's u = 0 * inf is NaN like the
  P.inv_hm1 = 1.0 / (double)(cfg->image_height - 1);  //  strict build's 0 / 0 — the reference divides by zero there too)
  P.max_child_rays = cfg->max_child_rays;
  P.rank = cfg->rank;
  P.nranks = cfg->nranks;
  P.tile_rows = cfg->tile_rows;
  P.local_rows = rows;
  P.seed_lo = (uint32_t)cfg->seed;
  P.seed_hi = (uint32_t)(cfg->seed >> 32);
  P.n_items = (uint32_t)n_items;
  P.n_lanes = (uint32_t)n_lanes;
  P.npix_local = (uint32_t)npix;
  P.div_npix = make_fastdiv((uint32_t)npix);
  P.div_w = make_fastdiv((uint32_t)cfg->image_width);
  P.div_tile = make_fastdiv((uint32_t)cfg->tile_rows);
  P.div_ns = make_fastdiv((uint32_t)streams_now);
  // tile the pixel order when the geometry allows it (a tile never straddles two strips)
  uint32_t th = 0, tw = 0;
  if (!c->knobs.no_tiles) tile_shape(cfg, rows, th, tw);
  P.tile_h_log2 = th;
  P.tile_w_log2 = tw;
  P.div_tpr_n = th ? (uint32_t)cfg->image_width >> tw : 1u;
  P.div_tpr = make_fastdiv(P.div_tpr_n);
  P.n_tile_rows = th ? (uint32_t)rows >> th : 1u;
  P.tile_table = nullptr;
  P.n_items_first = P.n_items;
  P.empty_batch = 64u;
  if (th) {
    // the top eighth of the image is traced last (RTOW_SKY_EIGHTHS: 0..8), and behind it the tiles that see nothing
    const uint32_t sky_rows = P.n_tile_rows * (uint32_t)c->knobs.sky_eighths / 8u;
    const long long key[10] = {1, c->scene_gen, cfg->image_width, cfg->image_height, cfg->rank, cfg->nranks, cfg->tile_rows,
                               (long long)th, (long long)sky_rows, c->knobs.tile_order ? 1 : 0};
    if (std::memcmp(key, c->tile_key, sizeof key) != 0) {  // (repeated renders of a resident scene reuse the table)
      std::vector<unsigned char> empty;
      std::vector<uint32_t> table;
      if (c->knobs.tile_order) tile_classify(c->host_scene, cfg, th, tw, rows, empty);
      c->tile_empty = tile_queue_table(empty, c->knobs.tile_order, P.div_tpr_n, P.n_tile_rows, sky_rows, table);
      if ((rc = c->tile_table.ensure(table.size() * sizeof(uint32_t)))) return rc;
      c->tile_key[0] = -1;
      HIPCHK(hipStreamSynchronize(st));  // (an earlier launch on this stream may still read the old table)
      HIPCHK(hipMemcpy(c->tile_table.p, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      std::memcpy(c->tile_key, key, sizeof key);
    }
    P.tile_table = (const uint32_t *)c->tile_table.p;
    P.n_items_first = P.n_items - c->tile_empty * 64u * (uint32_t)streams_now;
    P.empty_batch = 64u * (uint32_t)c->knobs.empty_levels;
  }
  P.partials = (double *)c->partials.p;
  P.stack = (uint32_t *)c->stack.p;
  P.spill = (uint32_t *)c->spill.p;
  // scene-class specialisation of the GRID kernel (rtow_device.h): static spheres with 48-byte fat lists, or static +
  // moving spheres with 80-byte ones, image in LDS, binary64 builds
  P.spec = rtow::kSpecGeneric;
  if (kernel == RTOW_KERNEL_GRID && lds_bytes > 0 && !f32 && !c->knobs.no_spec && scene.n_tri == 0) {
    if (scene.n_mov == 0 && c->grid_fat_stride == 48u) P.spec = rtow::kSpecStaticSpheres;
    if (scene.n_mov > 0 && c->grid_fat_stride == 80u) P.spec = rtow::kSpecMovingSpheres;
    // ... and on top of either class, a grid with one layer of cells in y (both cover scenes): the two-axis walk.  From
    // the header of the image that is resident NOW (every upload and refit, host- or device-built, sets grid_ny)
    if (P.spec != rtow::kSpecGeneric && c->grid_ny == 1 && !c->knobs.no_flat) P.spec |= rtow::kSpecFlatY;
  }
  P.walk = c->grid_walk;  // (read by the class kernels only; made with grid_ny, from the same header)
  P.b4_trips = c->knobs.bvh4_sm ? 0u : 1u;
  {
    const bool b4 = kernel == RTOW_KERNEL_BVH4;
    // every node in LDS (a small mesh, whether or not its triangles are staged too): a walk may stop once 24
    // lanes are left in it; nodes read from L2 (big mesh): 32 — the longer step hides more of the latency
    // (suzanne 16 / 20 / 24 / 28 / 32 / 40: 3.65 / 3.82 / 3.88 / 3.86 / 3.79 / 3.63 Gsamples/s; 96.8k mesh
    // 1.64 / 1.81 / 1.89 / 1.94 / 1.97 / 1.95)
    const bool b4_nodes_resident = b4 && scene.b4_lds_limit >= scene.b4_off_tri;
    int cap = c->knobs.walk_cap, open = c->knobs.walk_max_open;
    if (cap < 0) {
      cap = b4 ? 4 : 3;
      open = b4 ? (b4_nodes_resident ? 24 : 32) : 16;
    }
    // GRID: a resumed lane re-enters one cell BEHIND the cell it stopped at (rtow_trace_grid.h), and up to
    // two cell crossings can share one ray parameter (a ray through a cell corner), so fewer than 3 steps
    // per trip would not guarantee progress (cap 1 is a livelock).  BVH4 resumes exactly where it stopped.
    if (cap > 0 && !b4) cap = std::max(cap, 3);
    P.walk_cap = cap > 0 ? (uint32_t)cap : 0xffffffffu;
    P.walk_max_open = (uint32_t)open;
    P.leaf_votes = (uint32_t)(c->knobs.leaf_votes > 0 ? c->knobs.leaf_votes : (b4 ? 28 : 16));
  }
  P.fetch_votes = (uint32_t)(c->knobs.fetch_votes > 0 ? c->knobs.fetch_votes : (kernel == RTOW_KERNEL_BVH4 ? 2 : 4));
  P.sm4_restart = (uint32_t)c->knobs.sm4_votes[0];
  P.sm4_scatter = (uint32_t)c->knobs.sm4_votes[1];
  P.sm4_leaf = (uint32_t)c->knobs.sm4_votes[2];
  P.counters = (unsigned long long *)c->counters.p;
  P.t_origin = P.counters + 16;

  if (st != nullptr) HIPCHK(hipStreamWaitEvent(st, c->upload_ev, 0));  // the scene upload was queued on the null stream
  if (stats) HIPCHK(hipEventRecord(c->call_ev[0], st));
  if (!c->counters_init.p) {  // zeros, except the two minima of the diagnostic build ([5] min end, [16] t_origin)
    std::vector<unsigned long long> init(48, 0ull);
    init[5] = init[16] = ~0ull;
    if ((rc = c->counters_init.ensure(48 * sizeof(unsigned long long)))) return rc;
    HIPCHK(hipMemcpy(c->counters_init.p, init.data(), 48 * sizeof(unsigned long long), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpyAsync(c->counters.p, c->counters_init.p, 48 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
  const int slot = c->ev_count < kEventRing ? c->ev_count : -1;
  if (slot >= 0) HIPCHK(hipEventRecord(c->ev[slot][0], st));
  int launch_kernel = kernel;
  if (image_kernel && lds_bytes > 0 && c->knobs.stamps) launch_kernel = kernel + 16;  // diagnostic
  // counters[1..3] are read below only for a caller that takes statistics: every other launch runs the instantiation
  // without them where the kernel has one (rtow_trace_body.h, COUNT; RTOW_COUNT_ALWAYS keeps the counting one)
  const bool want_count = stats != nullptr || c->knobs.count_always;
  bool counted = true;
  int lrc = strict ? rtow::launch_trace_strict(P, launch_kernel, (int)grid, block, lds_bytes, st, want_count, &counted)
            : f32  ? rtow::launch_trace_f32(P, launch_kernel, (int)grid, block, lds_bytes, st, want_count, &counted)
                   : rtow::launch_trace_fast(P, launch_kernel, (int)grid, block, lds_bytes, st, want_count, &counted);
#ifdef RTOW_TAILSTAT
  if (const char *path = std::getenv("RTOW_TAILSTAT_OUT")) {
    HIPCHK(hipStreamSynchronize(st));
    std::vector<unsigned long long> ts((size_t)n_lanes / 64 * 8);
    HIPCHK(hipMemcpy(ts.data(), c->spill.p, ts.size() * 8, hipMemcpyDeviceToHost));
    if (FILE *f = std::fopen(path, "wb")) {
      std::fwrite(ts.data(), 8, ts.size(), f);
      std::fclose(f);
    }
  }
#endif
  if (lrc != 0) return fail(RTOW_EHIP, "trace kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
  c->last_spec = (int64_t)P.spec;
  c->last_counted = counted ? 1 : 0;
  if (slot >= 0) {
    HIPCHK(hipEventRecord(c->ev[slot][1], st));
    c->ev_count++;
  }
  rtow::ReduceParams R;
  R.partials = P.partials;
  R.out = (double *)d_rgb_sums;
  R.npix3 = (uint32_t)(npix * 3);
  R.nstreams = streams_now;
  R.accumulate = accumulate;
  R.W = (uint32_t)cfg->image_width;
  R.tile_w_log2 = tw;
  R.tile_h_log2 = th;
  R.tiles_per_row = P.div_tpr_n;
  R.rgb8 = nullptr;
  R.spp = 0.0;
  if (c->fuse_rgb8 && lvl_first == 0 && lvl_count == plan.count && !accumulate) {  // the whole render in this launch
    R.rgb8 = c->fuse_rgb8;
    R.spp = c->fuse_spp;
    c->fuse_used = true;
  }
  lrc = rtow::launch_reduce(R, st);
  if (lrc != 0) return fail(RTOW_EHIP, "reduce kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));

  if (stats) {
    HIPCHK(hipEventRecord(c->call_ev[1], st));
    HIPCHK(hipMemcpyAsync(c->h_counters, c->counters.p, 48 * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (c->h_counters[47] != 0ull) {  // the structural bound of the end-of-launch protocol fired (never observed)
      (void)check_dropped(c, false);    // (clears the sticky word: this call reports the error)
      return fail(RTOW_EHIP, "trace kernel: end-of-launch bound reached, %llu lanes gave up their samples",
                  c->h_counters[47]);
    }
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->call_ev[0], c->call_ev[1]));
    stats->total_ms = ms;
    if (slot >= 0) {
      HIPCHK(hipEventElapsedTime(&ms, c->ev[slot][0], c->ev[slot][1]));
      stats->kernel_ms = ms;
    }
    stats->samples = npix * ((unsigned long long)spt * (unsigned long long)(streams_now - 1) + (unsigned long long)spt_last);
    stats->segments = c->h_counters[1];
    if (kernel == RTOW_KERNEL_BRUTE) {
      stats->prim_tests = stats->segments * (unsigned long long)c->n_prims;
      stats->node_tests = 0;
    } else {
      stats->prim_tests = c->h_counters[2];
      stats->node_tests = c->h_counters[3];
    }
  }
  return RTOW_OK;
}

// Diagnostic: the 16 device counters of the last launch (work queue, segments, prim
// tests, node tests, ... region cycle sums of the RTOW_STAMPS build at [8..12]).
int rtow_debug_counters(rtow_ctx *c, unsigned long long *out48) {
  if (!c || !out48) return fail(RTOW_EINVAL, "NULL argument");
  if (!c->counters.p) return fail(RTOW_ENOSCENE, "no launch yet");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out48, c->counters.p, 48 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return RTOW_OK;
}

// Diagnostic: TraceParams::spec of the last trace launch (rtow_device.h kSpec*): which instantiation of the GRID kernel ran.
int rtow_debug_last_spec(rtow_ctx *c, uint32_t *out_spec) {
  if (!c || !out_spec) return fail(RTOW_EINVAL, "NULL argument");
  if (c->last_spec < 0) return fail(RTOW_ENOSCENE, "no launch yet");
  *out_spec = (uint32_t)c->last_spec;
  return RTOW_OK;
}

// Diagnostic: whether that launch's kernel was a counting instantiation (rtow_trace_body.h, COUNT).
int rtow_debug_last_counted(rtow_ctx *c, uint32_t *out_counted) {
  if (!c || !out_counted) return fail(RTOW_EINVAL, "NULL argument");
  if (c->last_counted < 0) return fail(RTOW_ENOSCENE, "no launch yet");
  *out_counted = (uint32_t)c->last_counted;
  return RTOW_OK;
}

// Diagnostic: the GRID walk's constants block as the last upload or refit derived it (TraceParams::walk).
int rtow_debug_walk_consts(rtow_ctx *c, void *out, int32_t capacity_bytes, int32_t *out_bytes) {
  if (!c || !out_bytes || capacity_bytes < 0 || (!out && capacity_bytes > 0)) return fail(RTOW_EINVAL, "NULL argument");
  if (!c->have_scene) return fail(RTOW_ENOSCENE, "no scene uploaded");
  *out_bytes = (int32_t)sizeof c->grid_walk;
  if (capacity_bytes > 0) std::memcpy(out, &c->grid_walk, std::min<size_t>((size_t)capacity_bytes, sizeof c->grid_walk));
  return RTOW_OK;
}

// write_color as a device epilogue: 8-bit RGB from the radiance sums.
int rtow_tonemap_device(rtow_ctx *c, const void *d_rgb_sums, int64_t n_values, int32_t spp_effective,
                        void *d_rgb8, void *hip_stream) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  if (!d_rgb_sums || !d_rgb8) return fail(RTOW_EINVAL, "NULL device pointer");
  if (n_values < 0 || n_values > 0xffffffffLL) return fail(RTOW_EINVAL, "n_values out of range");
  if (spp_effective <= 0) return fail(RTOW_EINVAL, "spp_effective must be positive");
  HIPCHK(hipSetDevice(c->device));
  int lrc = rtow::launch_tonemap((const double *)d_rgb_sums, (unsigned char *)d_rgb8, (uint32_t)n_values,
                                 (double)spp_effective, hip_stream);
  if (lrc != 0) return fail(RTOW_EHIP, "tonemap launch failed: %s", hipGetErrorString((hipError_t)lrc));
  return RTOW_OK;
}

int rtow_profile_collect(rtow_ctx *c, double *kernel_ms_sum, int32_t *launches) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  HIPCHK(hipSetDevice(c->device));
  double sum = 0.0;
  for (int i = 0; i < c->ev_count; ++i) {
    HIPCHK(hipEventSynchronize(c->ev[i][1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[i][0], c->ev[i][1]));
    sum += ms;
  }
  if (kernel_ms_sum) *kernel_ms_sum = sum;
  if (launches) *launches = c->ev_count;
  const bool waited = c->ev_count > 0;
  c->ev_count = 0;
  // the asynchronous entry point (rtow_render_device without stats) reports dropped samples here: every launch
  // of the ring has completed
  return waited ? check_dropped(c, false) : RTOW_OK;
}

static int impl_render(rtow_ctx *c, const rtow_scene_t *scene, const rtow_config_t *cfg, double *rgb_sums_host,
                rtow_stats_t *stats) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  if (!rgb_sums_host) return fail(RTOW_EINVAL, "rgb_sums_host is NULL");
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  if ((rc = upload_for(c, scene, cfg))) return rc;
  const int rows = rtow_local_rows(cfg);
  const size_t bytes = (size_t)rows * cfg->image_width * 3 * sizeof(double);
  if (bytes == 0) {
    if (stats) {
      std::memset(stats, 0, sizeof *stats);
    }
    return RTOW_OK;
  }
  if ((rc = c->out.ensure(bytes))) return rc;  // kept across calls
  void *d_out = c->out.p;
  if (cfg->accumulate)  // continue from the caller's sums
    HIPCHK(hipMemcpy(d_out, rgb_sums_host, bytes, hipMemcpyHostToDevice));
  rc = rtow_render_device(c, cfg, d_out, nullptr, stats);  // (no stats: no host wait before the copy below)
  if (rc != RTOW_OK) return rc;
  if ((rc = mirror_dropped(c, nullptr))) return rc;
  HIPCHK(hipMemcpy(rgb_sums_host, d_out, bytes, hipMemcpyDeviceToHost));
  return check_dropped(c, true);  // never RTOW_OK with samples dropped, with or without `stats`
}

// This rank's rows as 8-bit RGB on the DEVICE: render + write_color (fused into the reduce kernel when the render is
// one launch), asynchronous on `hip_stream` like rtow_render_device.  The f64 sums live in the context's workspace.
static int impl_render_device_rgb8(rtow_ctx *c, const rtow_config_t *cfg, void *d_rgb8, void *hip_stream,
                                   rtow_stats_t *stats) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  if (!d_rgb8) return fail(RTOW_EINVAL, "d_rgb8 is NULL");
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  const int spp_eff = cfg->samples_per_pixel / cfg->nstreams * cfg->nstreams;  // src/render.cpp:185
  if (spp_eff <= 0) return fail(RTOW_EINVAL, "no effective samples (samples_per_pixel < nstreams)");
  if (cfg->accumulate) return fail(RTOW_EINVAL, "the rgb8 entry points own their sums: accumulate must be 0");
  const int rows = rtow_local_rows(cfg);
  const size_t n = (size_t)rows * cfg->image_width * 3;
  if (n == 0) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    return RTOW_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  if ((rc = c->out.ensure(n * sizeof(double)))) return rc;  // kept across calls
  c->fuse_rgb8 = (unsigned char *)d_rgb8;  // write_color inside the reduce kernel when the render is one launch
  c->fuse_spp = (double)spp_eff;
  c->fuse_used = false;
  rc = impl_render_device(c, cfg, c->out.p, hip_stream, stats);
  c->fuse_rgb8 = nullptr;
  if (rc == RTOW_OK && !c->fuse_used) rc = rtow_tonemap_device(c, c->out.p, (int64_t)n, spp_eff, d_rgb8, hip_stream);
  return rc;
}

// upload + render + device write_color + copy 8-bit RGB to the host: the whole output path of
// the reference's render() with 3 bytes per pixel over PCIe instead of 24.
static int impl_render_rgb8(rtow_ctx *c, const rtow_scene_t *scene, const rtow_config_t *cfg, unsigned char *rgb8_host,
                     rtow_stats_t *stats) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  if (!rgb8_host) return fail(RTOW_EINVAL, "rgb8_host is NULL");
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  if (cfg->samples_per_pixel / cfg->nstreams <= 0) return fail(RTOW_EINVAL, "no effective samples (samples_per_pixel < nstreams)");
  if (cfg->accumulate) return fail(RTOW_EINVAL, "rtow_render_rgb8 owns its sums: accumulate must be 0");
  if ((rc = upload_for(c, scene, cfg))) return rc;
  const int rows = rtow_local_rows(cfg);
  const size_t n = (size_t)rows * cfg->image_width * 3;
  if (n == 0) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    return RTOW_OK;
  }
  if ((rc = c->out8.ensure(n))) return rc;  // kept across calls
  if ((rc = impl_render_device_rgb8(c, cfg, c->out8.p, nullptr, stats))) return rc;
  // (a pinned landing buffer + host memcpy measured slower than the runtime's own staged copy for these 2.9 MB:
  // 8.67 vs 8.55 ms per call)
  if ((rc = mirror_dropped(c, nullptr))) return rc;
  HIPCHK(hipMemcpy(rgb8_host, c->out8.p, n, hipMemcpyDeviceToHost));
  return check_dropped(c, true);  // never RTOW_OK with samples dropped, with or without `stats`
}

// ---- the guarded entry points (see guarded() above) ----
int rtow_ctx_create(int device_id, rtow_ctx **out) {
  return guarded("rtow_ctx_create", [&] { return impl_ctx_create(device_id, out); });
}
int rtow_scene_upload(rtow_ctx *c, const rtow_scene_t *s) {
  return guarded("rtow_scene_upload", [&] { return impl_scene_upload(c, s); });
}
int rtow_render_device(rtow_ctx *c, const rtow_config_t *cfg, void *d_rgb_sums, void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_render_device", [&] { return impl_render_device(c, cfg, d_rgb_sums, hip_stream, stats); });
}
int rtow_render(rtow_ctx *c, const rtow_scene_t *scene, const rtow_config_t *cfg, double *rgb_sums_host,
                rtow_stats_t *stats) {
  return guarded("rtow_render", [&] { return impl_render(c, scene, cfg, rgb_sums_host, stats); });
}
int rtow_render_rgb8(rtow_ctx *c, const rtow_scene_t *scene, const rtow_config_t *cfg, unsigned char *rgb8_host,
                     rtow_stats_t *stats) {
  return guarded("rtow_render_rgb8", [&] { return impl_render_rgb8(c, scene, cfg, rgb8_host, stats); });
}
int rtow_render_device_rgb8(rtow_ctx *c, const rtow_config_t *cfg, void *d_rgb8, void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_render_device_rgb8", [&] { return impl_render_device_rgb8(c, cfg, d_rgb8, hip_stream, stats); });
}
int rtow_scene_refit(rtow_ctx *c, const rtow_scene_t *s) {
  return guarded("rtow_scene_refit", [&] { return impl_scene_refit(c, s); });
}
// (diagnostic / tests; pure host arithmetic, usable without a GPU) the queue order of the tiles of a render of `cfg` of
// `scene` by a context with the default knobs (include/rtow.h)
int rtow_debug_tile_order(const rtow_scene_t *scene, const rtow_config_t *cfg, uint32_t *table_out, unsigned char *empty_out,
                          int32_t capacity, int32_t *n_empty, int32_t *tile_w_log2, int32_t *tile_h_log2) {
  return guarded("rtow_debug_tile_order", [&]() -> int {
    int rc = validate_scene(scene);
    if (rc) return rc;
    if ((rc = validate_cfg(cfg))) return rc;
    Knobs knobs;
    knobs.read();
    rtow_ctx::HostSceneCopy h;
    h.sg.assign(scene->sphere_geom, scene->sphere_geom + 4 * (size_t)scene->n_spheres);
    h.mg.assign(scene->moving_geom, scene->moving_geom + 8 * (size_t)scene->n_moving);
    h.tg.assign(scene->triangle_geom, scene->triangle_geom + 9 * (size_t)scene->n_triangles);
    h.cam = scene->camera;
    const int rows = rtow_local_rows(cfg);
    uint32_t th = 0, tw = 0;
    if (!knobs.no_tiles) tile_shape(cfg, rows, th, tw);
    if (tile_w_log2) *tile_w_log2 = (int32_t)tw;
    if (tile_h_log2) *tile_h_log2 = (int32_t)th;
    if (n_empty) *n_empty = 0;
    if (!th) return 0;
    const uint32_t tpr = (uint32_t)cfg->image_width >> tw, ntr = (uint32_t)rows >> th;
    std::vector<unsigned char> empty;
    std::vector<uint32_t> table;
    if (knobs.tile_order) tile_classify(h, cfg, th, tw, rows, empty);
    const uint32_t ne = tile_queue_table(empty, knobs.tile_order, tpr, ntr, ntr * (uint32_t)knobs.sky_eighths / 8u, table);
    if (n_empty) *n_empty = (int32_t)ne;
    for (size_t i = 0; i < table.size() && (int32_t)i < capacity; ++i) {
      if (table_out) table_out[i] = table[i];
      if (empty_out) empty_out[i] = knobs.tile_order ? empty[i] : 0;
    }
    return (int)table.size();
  });
}
int rtow_debug_schedule(rtow_ctx *c, const rtow_config_t *cfg, uint32_t *out, int32_t capacity_pairs) {
  return guarded("rtow_debug_schedule", [&] { return impl_debug_schedule(c, cfg, out, capacity_pairs); });
}

}  // extern "C"

namespace rtow {
// for rtow_multi.cpp: the sticky dropped-samples word of a context, read after its stream has been waited for
int ctx_check_dropped(rtow_ctx *c) { return c ? check_dropped(c, false) : RTOW_OK; }
int ctx_mirror_dropped(rtow_ctx *c, void *stream) { return c ? mirror_dropped(c, (hipStream_t)stream) : RTOW_OK; }
int ctx_check_dropped_mirrored(rtow_ctx *c) {
  if (!c) return RTOW_OK;
  if (*c->h_dropped != 0ull) HIPCHK(hipSetDevice(c->device));  // (the error path resets the device word)
  return check_dropped(c, true);
}
}  // namespace rtow

