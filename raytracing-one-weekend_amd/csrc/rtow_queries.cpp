// rtow_queries.cpp — every query over the resident scene: rtow_intersect*, rtow_occluded*, rtow_closest_point*,
// rtow_first_hits*, rtow_nearest*, rtow_radiance*, rtow_path_step*, rtow_ambient*, rtow_sweep*, rtow_overlap* and the camera stage (rtow_camera_rays*, rtow_guides*).
//
// One host path serves them all.  A QueryKind row says what tells an entry-point pair apart — its buffers, its strategy
// resolver, its launchers — and query_device / query_host are the two entry forms of every row; the camera stage, whose
// batch comes from a config instead of a count, has front ends of its own over the same checks, staging and launch.
// A new query is one row here and one kernel header ("Adding a query").
//
// What the render side shares with this file (the strategy and residency rules, the launch shape) is declared in
// rtow_ctx.h and defined in rtow_capi.cpp.

#include "rtow_ctx.h"

namespace rtow {
// csrc/rtow_<family>_{strict,fast}.hip (rtow_query.h, rtow_occlude.h, rtow_pointq.h, rtow_first_hits.h, rtow_nearest.h,
// rtow_radiance.h, rtow_step.h, rtow_guides.h, rtow_ambient.h, rtow_sweep.h, rtow_overlap.h): every family exports one launcher and one occupancy function per build
using QueryLaunchFn = int(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block, unsigned lds_bytes,
                          void *stream);
using QueryOccupancyFn = int(int kernel, int block, unsigned lds_bytes, int *vgprs);
QueryLaunchFn launch_query_strict, launch_query_fast, launch_occlude_strict, launch_occlude_fast, launch_pointq_strict,
    launch_pointq_fast, launch_first_hits_strict, launch_first_hits_fast, launch_nearest_strict, launch_nearest_fast,
    launch_radiance_strict, launch_radiance_fast, launch_step_strict, launch_step_fast, launch_guides_strict,
    launch_guides_fast, launch_camera_rays_strict, launch_camera_rays_fast, launch_ambient_strict, launch_ambient_fast,
    launch_sweep_strict, launch_sweep_fast, launch_overlap_strict, launch_overlap_fast;
QueryOccupancyFn query_occupancy_strict, query_occupancy_fast, occlude_occupancy_strict, occlude_occupancy_fast,
    pointq_occupancy_strict, pointq_occupancy_fast, first_hits_occupancy_strict, first_hits_occupancy_fast,
    nearest_occupancy_strict, nearest_occupancy_fast, radiance_occupancy_strict, radiance_occupancy_fast,
    step_occupancy_strict, step_occupancy_fast, guides_occupancy_strict, guides_occupancy_fast, ambient_occupancy_strict,
    ambient_occupancy_fast, sweep_occupancy_strict, sweep_occupancy_fast, overlap_occupancy_strict, overlap_occupancy_fast;
}  // namespace rtow

namespace {

constexpr int64_t kMaxQueryRays = (1ll << 31) - 64;  // include/rtow.h

// Walk-order primitive id -> insertion index (the uploaded scene's prim_kind / prim_index order; class-major order when
// the scene came without one).  which: 0 class-major ids (STREAM, GRID, REFTREE walks and a device-built BVH image),
// 1 the record slots of a host-built mesh BVH image (ds.leaf_direct), 2 the record slots of the 4-wide image (match_slots).
// Built on the host at the first query that needs the table after an upload or a refit; both drop them.
int query_map(rtow_ctx *c, int which, const int32_t **out) {
  if (c->q_map_ok[which]) {
    *out = (const int32_t *)c->q_map[which].p;
    return RTOW_OK;
  }
  const int ns = c->ds.n_sph, nm = c->ds.n_mov, nt = c->ds.n_tri, np = c->n_prims;
  const rtow_ctx::HostSceneCopy &h = c->host_scene;
  std::vector<int32_t> cls2ins((size_t)np);
  for (int i = 0; i < np; ++i) cls2ins[i] = i;
  if (h.have_order)
    for (int i = 0; i < np; ++i) {
      const int k = h.pk[i];
      const int base = k == RTOW_PRIM_SPHERE ? 0 : (k == RTOW_PRIM_MOVING_SPHERE ? ns : ns + nm);
      cls2ins[(size_t)base + h.pi[i]] = i;
    }
  std::vector<int32_t> table;
  if (which == 0) {
    table.swap(cls2ins);
  } else {
    // after a refit the records have moved: the maps its first call derived from the images as uploaded
    std::vector<int32_t> matched;
    if (!c->rf.ready)
      if (int rc = match_slots(c, which, matched)) return rc;
    const std::vector<int32_t> &slot2tri = c->rf.ready ? c->rf.slot2tri[which - 1] : matched;
    table.assign((size_t)nt, -1);
    for (int k = 0; k < nt; ++k) table[(size_t)k] = cls2ins[(size_t)ns + nm + slot2tri[(size_t)k]];
  }
  DevBuf &b = c->q_map[which];
  if (int rc = b.ensure(std::max<size_t>(table.size() * sizeof(int32_t), 4))) return rc;
  if (!table.empty()) HIPCHK(hipMemcpy(b.p, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  c->q_map_ok[which] = true;
  *out = (const int32_t *)b.p;
  return RTOW_OK;
}

// The table the hits of `kernel`'s walk need: the 4-wide image's record slots, a leaf-ordered binary image's, or class-major ids
int query_map_for(rtow_ctx *c, int kernel, const int32_t **out) {
  return query_map(c, kernel == RTOW_KERNEL_BVH4 ? 2 : (kernel == RTOW_KERNEL_BVH && c->ds.leaf_direct ? 1 : 0), out);
}

// ---- what tells the queries apart: one QueryKind row per entry-point pair ----------------------------------------------
constexpr int kMaxQueryBufs = 6;

// One buffer argument, in the entry point's argument order (the order of the alignment checks).
struct QueryBuf {
  const char *name;          // the word of the error texts
  bool required;             // NULL is refused when there is anything to do
  unsigned align;            // alignment required of the device buffer
  size_t item_bytes;         // record size (include/rtow.h)
  bool per_k;                // k (max_hits; the ambient query: samples) records per query instead of one
  bool out;                  // the host form copies it back (otherwise: in)
  DevBuf rtow_ctx::*stage;   // the host form's device buffer; two buffers of one size may share one (a step in place)
  void *rtow::QueryArgs::*arg;  // where the launcher finds it; nullptr: the input, QueryArgs::in
};

// What one call brings: the entry points' arguments, buffers in the row's order.
struct QueryCall {
  int32_t precision, kernel;
  int64_t n;
  int32_t k;           // k / max_hits (rows with k_max); the ambient query: params->samples (checked by its own hook)
  const void *params;  // rtow_radiance_params_t / rtow_step_params_t / rtow_ambient_params_t (rows with has_params)
  void *buf[kMaxQueryBufs];
  void *stream;
  rtow_stats_t *stats;
};

enum class Walk { kNone, kRay, kPoint };  // how the strategy is resolved: not at all, resolve_kernel, resolve_point_kernel

struct QueryKind {
  const char *count = nullptr;  // the word for n in the error texts
  int n_bufs = 0;
  QueryBuf bufs[kMaxQueryBufs] = {};
  Walk walk = Walk::kRay;
  bool mapped = false;           // hit records name primitives by insertion index: needs query_map (when hits are asked for)
  bool map_always = false;       // ... and so does the query itself (the overlap query's min_prim): query_map in every call
  bool brute_no_lds = false;     // its BRUTE walk reads the class-major arrays: launched without LDS
  bool brute_tests_all = false;  // its STREAM walk tests every primitive uncounted: prim_tests = n * n_prims
  const char *k_name = nullptr;  // nullptr: no k; else "k" / "max_hits", in [1, k_max]
  int32_t k_max = 0;
  bool k_first = false;          // k is checked before n (else behind it)
  bool has_params = false;       // NULL params are refused right behind ctx (device form)
  bool check_sizes_staging = false;  // the host form, too, refuses NULL params and runs `check` before it stages anything:
                                     // the row's params size a buffer (the ambient query's ray export)
  int Knobs::*block_cap = nullptr;            // nullptr, or the test knob that caps the workgroups
  rtow::QueryLaunchFn *launch[2] = {};        // [0] strict, [1] fast
  rtow::QueryOccupancyFn *occupancy[2] = {};  // nullptr: a kernel that walks nothing, 8 workgroups per CU
  // what is truly per family (each may be nullptr): the checks behind the alignments; what the kernel reads beyond the
  // walks' fields (the seed and stack of TraceParams, the scalars of QueryArgs); the stats beyond query_launch's
  int (*check)(const QueryCall &call) = nullptr;
  int64_t (*grid_items)(const QueryCall &call) = nullptr;  // what the grid is sized for when that is not n
  int (*fill)(rtow_ctx *c, const QueryCall &call, bool strict, rtow::TraceParams &P, rtow::QueryArgs &a) = nullptr;
  void (*epilogue)(const rtow_ctx *c, const QueryCall &call, rtow_stats_t *stats) = nullptr;
};

using rtow::QueryArgs;
#define RTOW_LAUNCHERS(family)                                                  \
  .launch = {rtow::launch_##family##_strict, rtow::launch_##family##_fast},     \
  .occupancy = {rtow::family##_occupancy_strict, rtow::family##_occupancy_fast}

// closest hit
const QueryKind kIntersect = {
    .count = "n_rays", .n_bufs = 2,
    .bufs = {{"ray", true, 16, sizeof(rtow_ray_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"hit", true, 8, sizeof(rtow_hit_t), false, true, &rtow_ctx::q_hits, &QueryArgs::hits}},
    .walk = Walk::kRay, .mapped = true, .brute_tests_all = true, RTOW_LAUNCHERS(query)};
// any hit: the closest-hit query's contract without its hit records (so no query_map: nothing to translate)
const QueryKind kOccluded = {
    .count = "n_rays", .n_bufs = 2,
    .bufs = {{"ray", true, 16, sizeof(rtow_ray_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"result", true, 1, 1, false, true, &rtow_ctx::q_occ, &QueryArgs::result}},
    .walk = Walk::kRay, RTOW_LAUNCHERS(occlude)};
// closest point: the closest-hit query's contract with the point walks (BRUTE stages no triangle tiles)
const QueryKind kClosestPoint = {
    .count = "n", .n_bufs = 2,
    .bufs = {{"query", true, 16, sizeof(rtow_point_query_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"hit", true, 16, sizeof(rtow_point_hit_t), false, true, &rtow_ctx::q_hits, &QueryArgs::hits}},
    .walk = Walk::kPoint, .mapped = true, .brute_no_lds = true, RTOW_LAUNCHERS(pointq)};
// first k hits (csrc/rtow_first_hits.h): max_hits records and one count per ray.  REFTREE is refused (the reference's
// tree misses hits by design: no multi-hit meaning).  BRUTE counts the tests it ran.
const QueryKind kFirstHits = {
    .count = "n_rays", .n_bufs = 3,
    .bufs = {{"ray", true, 16, sizeof(rtow_ray_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"hit", true, 8, sizeof(rtow_hit_t), true, true, &rtow_ctx::q_khits, &QueryArgs::hits},
             {"count", false, 4, sizeof(int32_t), false, true, &rtow_ctx::q_kcounts, &QueryArgs::counts}},
    .walk = Walk::kRay, .mapped = true, .brute_no_lds = true, .k_name = "max_hits", .k_max = RTOW_MAX_HITS,
    RTOW_LAUNCHERS(first_hits),
    .check = [](const QueryCall &call) {
      return call.kernel == RTOW_KERNEL_REFTREE
                 ? fail(RTOW_EINVAL, "first-hits queries: RTOW_KERNEL_REFTREE has no multi-hit meaning") : RTOW_OK;
    }};
// k nearest (csrc/rtow_nearest.h): k records and one count per point; k is checked before anything else is looked at
const QueryKind kNearest = {
    .count = "n", .n_bufs = 3,
    .bufs = {{"query", true, 16, sizeof(rtow_point_query_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"hit", true, 16, sizeof(rtow_point_hit_t), true, true, &rtow_ctx::q_khits, &QueryArgs::hits},
             {"count", false, 4, sizeof(int32_t), false, true, &rtow_ctx::q_kcounts, &QueryArgs::counts}},
    .walk = Walk::kPoint, .mapped = true, .brute_no_lds = true, .k_name = "k", .k_max = RTOW_MAX_NEAREST, .k_first = true,
    RTOW_LAUNCHERS(nearest)};
// radiance (csrc/rtow_radiance.h): whole paths.  Beyond the walks' fields they need the Philox key, the depth and — strict
// build — a path stack of their own, [bounce][lane] material indices, sized for this launch's lanes.
const QueryKind kRadiance = {
    .count = "n_rays", .n_bufs = 3,
    .bufs = {{"ray", true, 16, sizeof(rtow_ray_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"ids", false, 8, 8, false, false, &rtow_ctx::q_ids, &QueryArgs::ids},
             {"result", true, 8, 24, false, true, &rtow_ctx::q_rgb, &QueryArgs::result}},
    .walk = Walk::kRay, .has_params = true, .block_cap = &Knobs::radiance_blocks, RTOW_LAUNCHERS(radiance),
    .check = [](const QueryCall &call) {
      const auto *prm = (const rtow_radiance_params_t *)call.params;
      if (prm->samples_per_ray < 1) return fail(RTOW_EINVAL, "samples_per_ray %d < 1", prm->samples_per_ray);
      if (prm->max_child_rays < 0) return fail(RTOW_EINVAL, "max_child_rays %d < 0", prm->max_child_rays);
      return (int)RTOW_OK;
    },
    .fill = [](rtow_ctx *c, const QueryCall &call, bool strict, rtow::TraceParams &P, QueryArgs &a) {
      const auto *prm = (const rtow_radiance_params_t *)call.params;
      P.seed_lo = (uint32_t)(prm->seed & 0xffffffffu);
      P.seed_hi = (uint32_t)(prm->seed >> 32);
      P.max_child_rays = prm->max_child_rays;
      a.samples = prm->samples_per_ray;
      a.sample_first = prm->sample_first;
      if (!strict) return (int)RTOW_OK;
      const size_t words = (size_t)prm->max_child_rays * (size_t)P.n_lanes;
      const int rc = c->q_stack.ensure(std::max<size_t>(words * sizeof(uint32_t), 16));
      P.stack = (uint32_t *)c->q_stack.p;
      return rc;
    },
    .epilogue = [](const rtow_ctx *c, const QueryCall &call, rtow_stats_t *stats) {
      stats->samples = (uint64_t)call.n * (uint64_t)((const rtow_radiance_params_t *)call.params)->samples_per_ray;
      stats->segments = c->h_qcounters[2];
    }};
// path step (csrc/rtow_step.h): one segment per ray, traced and scattered.  The host form steps the rays in place in
// q_rays; its attenuations go through the radiance query's q_rgb.  BRUTE reports n * n_prims tests, as rtow_intersect does.
const QueryKind kStep = {
    .count = "n_rays", .n_bufs = 6,
    .bufs = {{"ray", true, 16, sizeof(rtow_ray_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"ids", false, 8, 8, false, false, &rtow_ctx::q_ids, &QueryArgs::ids},
             {"next-ray", true, 16, sizeof(rtow_ray_t), false, true, &rtow_ctx::q_rays, &QueryArgs::next},
             {"attenuation", true, 8, 24, false, true, &rtow_ctx::q_rgb, &QueryArgs::atten},
             {"status", true, 4, sizeof(int32_t), false, true, &rtow_ctx::q_status, &QueryArgs::status},
             {"hit", false, 8, sizeof(rtow_hit_t), false, true, &rtow_ctx::q_hits, &QueryArgs::hits}},
    .walk = Walk::kRay, .mapped = true, .brute_tests_all = true, .has_params = true, RTOW_LAUNCHERS(step),
    .check = [](const QueryCall &call) {
      const int32_t bounce = ((const rtow_step_params_t *)call.params)->bounce;
      return bounce < 0 ? fail(RTOW_EINVAL, "bounce %d < 0", bounce) : RTOW_OK;
    },
    .fill = [](rtow_ctx *, const QueryCall &call, bool, rtow::TraceParams &P, QueryArgs &a) {
      const auto *prm = (const rtow_step_params_t *)call.params;
      P.seed_lo = (uint32_t)(prm->seed & 0xffffffffu);
      P.seed_hi = (uint32_t)(prm->seed >> 32);
      a.request = 1u + (uint32_t)prm->bounce;
      a.sample_first = prm->sample_first;
      return (int)RTOW_OK;
    }};
// ambient (csrc/rtow_ambient.h): `samples` any-hit walks per surface point, drawn in the kernel; one record per point and,
// on request, the `samples` rays it walked.  The samples size that export, so the hook below runs before the host form
// stages; QueryCall::k carries them to the staging (buf_bytes).
const QueryKind kAmbient = {
    .count = "n", .n_bufs = 4,
    .bufs = {{"point", true, 16, sizeof(rtow_surface_point_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"ids", false, 8, 8, false, false, &rtow_ctx::q_ids, &QueryArgs::ids},
             {"result", true, 16, sizeof(rtow_ambient_t), false, true, &rtow_ctx::q_ambient, &QueryArgs::result},
             {"ray", false, 16, sizeof(rtow_ray_t), true, true, &rtow_ctx::q_ambient_rays, &QueryArgs::rays_out}},
    .walk = Walk::kRay, .has_params = true, .check_sizes_staging = true, RTOW_LAUNCHERS(ambient),
    .check = [](const QueryCall &call) {
      const int32_t samples = ((const rtow_ambient_params_t *)call.params)->samples;
      if (samples < 1 || samples > RTOW_MAX_AMBIENT_SAMPLES)
        return fail(RTOW_EINVAL, "samples %d outside [1, %d]", samples, RTOW_MAX_AMBIENT_SAMPLES);
      if (call.buf[3] && call.n * (int64_t)samples > kMaxQueryRays)
        return fail(RTOW_EINVAL, "n * samples = %lld rays to export, beyond 2^31 - 64", (long long)(call.n * (int64_t)samples));
      return (int)RTOW_OK;
    },
    // a wave's 64 points are 64 x samples walks: from 16 samples on, one wave's step is a workgroup's worth of work, and
    // the kernel numbers its waves across the workgroups
    .grid_items = [](const QueryCall &call) {
      return call.n * (int64_t)std::min(((const rtow_ambient_params_t *)call.params)->samples, 16);
    },
    .fill = [](rtow_ctx *, const QueryCall &call, bool, rtow::TraceParams &P, QueryArgs &a) {
      const auto *prm = (const rtow_ambient_params_t *)call.params;
      P.seed_lo = (uint32_t)(prm->seed & 0xffffffffu);
      P.seed_hi = (uint32_t)(prm->seed >> 32);
      a.samples = prm->samples;
      a.sample_first = prm->sample_first;
      return (int)RTOW_OK;
    },
    .epilogue = [](const rtow_ctx *, const QueryCall &call, rtow_stats_t *stats) {
      stats->samples = stats->segments = (uint64_t)call.n * (uint64_t)((const rtow_ambient_params_t *)call.params)->samples;
    }};
static_assert(sizeof(rtow_surface_point_t) == 64 && sizeof(rtow_ambient_t) == 64 && sizeof(rtow_ambient_params_t) == 16,
              "the ambient query's records: four 16-byte loads, four 16-byte stores");
// swept sphere (csrc/rtow_sweep.h): the closest-point query's contract with the sweep walks; one 80-byte record in and out
const QueryKind kSweep = {
    .count = "n", .n_bufs = 2,
    .bufs = {{"query", true, 16, sizeof(rtow_sweep_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"hit", true, 16, sizeof(rtow_sweep_hit_t), false, true, &rtow_ctx::q_hits, &QueryArgs::hits}},
    .walk = Walk::kPoint, .mapped = true, .brute_no_lds = true, RTOW_LAUNCHERS(sweep)};
static_assert(sizeof(rtow_sweep_t) == 80 && sizeof(rtow_sweep_hit_t) == 80,
              "the sweep query's records: five 16-byte loads, five 16-byte stores");
// box overlap (csrc/rtow_overlap.h): one count and max_ids insertion indices per box; max_ids is checked where k nearest
// checks k.  The ids travel as QueryArgs::hits; min_prim compares insertion indices, so the map is made for a call
// without ids too.
const QueryKind kOverlap = {
    .count = "n", .n_bufs = 3,
    .bufs = {{"query", true, 16, sizeof(rtow_box_query_t), false, false, &rtow_ctx::q_rays, nullptr},
             {"count", true, 4, sizeof(int32_t), false, true, &rtow_ctx::q_kcounts, &QueryArgs::counts},
             {"ids", false, 4, sizeof(int32_t), true, true, &rtow_ctx::q_khits, &QueryArgs::hits}},
    .walk = Walk::kPoint, .mapped = true, .map_always = true, .brute_no_lds = true, .k_name = "max_ids",
    .k_max = RTOW_MAX_OVERLAP_IDS, .k_first = true, RTOW_LAUNCHERS(overlap)};
static_assert(sizeof(rtow_box_query_t) == 64 && offsetof(rtow_box_query_t, time) == 48 && offsetof(rtow_box_query_t, min_prim) == 56,
              "the overlap query's record: four 16-byte loads");
// the camera stage (csrc/rtow_guides.h): the primaries of the resident camera — a kernel that reads the camera alone —
// and the first-hit guide buffers
const QueryKind kCameraRays = {
    .n_bufs = 2,
    .bufs = {{"ray", true, 16, sizeof(rtow_ray_t), false, true, &rtow_ctx::q_rays, &QueryArgs::result},
             {"ids", false, 8, 8, false, true, &rtow_ctx::q_ids, &QueryArgs::ids}},
    .walk = Walk::kNone, .launch = {rtow::launch_camera_rays_strict, rtow::launch_camera_rays_fast}};
const QueryKind kGuides = {
    .n_bufs = 1,
    .bufs = {{"guide", true, 16, sizeof(rtow_guide_t), false, true, &rtow_ctx::q_guides, &QueryArgs::result}},
    .walk = Walk::kRay, .block_cap = &Knobs::guides_blocks, RTOW_LAUNCHERS(guides)};
static_assert(sizeof(rtow_guide_t) == 64, "rtow_guide_t is four 16-byte stores");
#undef RTOW_LAUNCHERS

// ---- the checks ---------------------------------------------------------------------------------------------------------
// ctx aside, the first checks of both forms: the range of n, and of k before or behind it
int check_counts(const QueryKind &k, const QueryCall &call) {
  for (const bool first : {true, false}) {
    if (k.k_name && k.k_first == first && (call.k < 1 || call.k > k.k_max))
      return fail(RTOW_EINVAL, "%s %d outside [1, %d]", k.k_name, call.k, k.k_max);
    if (first && (call.n < 0 || call.n > kMaxQueryRays))
      return fail(RTOW_EINVAL, "%s %lld outside [0, 2^31 - 64]", k.count, (long long)call.n);
  }
  return RTOW_OK;
}

// A required buffer that is NULL with something to do ("NULL ray, next-ray, attenuation or status buffer"); then, for
// device buffers (what = "buffer"; host arrays: "array"), the alignments in argument order.
int check_buffers(const QueryKind &k, void *const *buf, int64_t n, const char *what, bool device) {
  int required = 0, missing = 0;
  for (int i = 0; i < k.n_bufs; ++i) {
    required += k.bufs[i].required ? 1 : 0;
    missing += k.bufs[i].required && !buf[i] ? 1 : 0;
  }
  if (n > 0 && missing) {
    std::string names;  // the required buffers: "a", "a or b", "a, b or c"
    for (int i = 0, left = required; i < k.n_bufs; ++i) {
      if (!k.bufs[i].required) continue;
      names += std::string(k.bufs[i].name) + (--left > 1 ? ", " : left == 1 ? " or " : "");
    }
    return fail(RTOW_EINVAL, "NULL %s %s", names.c_str(), what);
  }
  for (int i = 0; device && i < k.n_bufs; ++i)
    if (((uintptr_t)buf[i] & (k.bufs[i].align - 1u)) != 0u)
      return fail(RTOW_EINVAL, "%s %s must be %u-byte aligned", k.bufs[i].name, what, k.bufs[i].align);
  return RTOW_OK;
}

// ---- the launch ---------------------------------------------------------------------------------------------------------
// query_begin: the argument checks after the buffers', the strategy (the render's resolution and residency rules), the
// launch shape, the stats header.  query_launch: the grid from the kernel's occupancy, the BVH4 spill, the walk fields, and
// the launch between events on the caller's stream (ordered behind the last upload); with stats, the counters and times.
constexpr size_t kQueryCounters = 4;  // [0] primitive tests, [1] node tests; the radiance query: [2] segments, [3] queue head
struct QueryRun {
  int kernel = 0;
  bool strict = false;
  LaunchShape shape;
  unsigned lds = 0;   // LDS bytes of the launch: the shape's, or none (QueryKind::brute_no_lds)
  int block_cap = 0;  // > 0: at most this many workgroups (QueryKind::block_cap)
};
// The point query's strategy: AUTO takes the best resident tree (BVH4, else BVH, else BRUTE: it never fails on a resident
// scene); GRID has no point walk and is answered by the binary BVH; then the render's fallbacks and residency rules.
int resolve_point_kernel(rtow_ctx *c, int precision, int requested, int *out) {
  int kernel = requested;
  if (kernel == RTOW_KERNEL_REFTREE) return fail(RTOW_EINVAL, "point queries: RTOW_KERNEL_REFTREE has no point walk");
  if (kernel == RTOW_KERNEL_AUTO)
    kernel = c->have_bvh4 ? RTOW_KERNEL_BVH4 : (c->built & kNeedBvh) ? RTOW_KERNEL_BVH : RTOW_KERNEL_BRUTE;
  if (kernel == RTOW_KERNEL_GRID) kernel = RTOW_KERNEL_BVH;
  return resident_kernel(c, precision, kernel, false, out);
}

// Walk::kNone (rtow_camera_rays*): the request is checked but no strategy is resolved — q.kernel stays 0, and a lean
// upload, which built one strategy's structures only, is as good as a full one
int query_begin(rtow_ctx *c, const QueryKind &k, int32_t precision, int32_t kernel_req, rtow_stats_t *stats, QueryRun &q) {
  if (precision == RTOW_F32) return fail(RTOW_EINVAL, "ray queries: RTOW_F32 is not supported (binary64 builds only)");
  if (precision != RTOW_F64_STRICT && precision != RTOW_F64_FAST) return fail(RTOW_EINVAL, "unknown precision %d", precision);
  if (kernel_req < RTOW_KERNEL_AUTO || kernel_req > RTOW_KERNEL_REFTREE) return fail(RTOW_EINVAL, "unknown kernel %d", kernel_req);
  if (!c->have_scene) return fail(RTOW_ENOSCENE, "no scene uploaded");
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if (k.walk == Walk::kNone) {
    q.kernel = 0;
    q.shape.block = kBlock;
  } else {
    if ((rc = k.walk == Walk::kPoint ? resolve_point_kernel(c, precision, kernel_req, &q.kernel)
                                     : resolve_kernel(c, precision, kernel_req, &q.kernel)))
      return rc;
    if ((rc = launch_shape(c, q.kernel, false, q.shape))) return rc;
  }
  q.strict = precision == RTOW_F64_STRICT;
  q.lds = k.brute_no_lds && q.kernel == RTOW_KERNEL_BRUTE ? 0u : q.shape.lds_bytes;
  q.block_cap = k.block_cap ? c->knobs.*k.block_cap : 0;
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->kernel_used = q.kernel;
  }
  return RTOW_OK;
}

// n_items: what the grid is sized for; a: the launcher's arguments but the counters; fill(P, a): what the family's kernel
// reads beyond the walks' fields, made before anything is enqueued (an RTOW_* code)
template <class Fill>
int query_launch(rtow_ctx *c, const QueryKind &k, const QueryRun &q, QueryArgs a, int64_t n_items, void *hip_stream,
                 rtow_stats_t *stats, Fill &&fill) {
  const int kernel = q.kernel, build = q.strict ? 0 : 1;
  const int block = q.shape.block;
  int occ = k.occupancy[build] ? k.occupancy[build](kernel, block, q.lds, nullptr) : 8;
  if (occ <= 0) return fail(RTOW_EHIP, "query occupancy failed (kernel %d, %u B of LDS)", kernel, q.shape.lds_bytes);
  occ = std::min(occ, 8);
  long long grid = (long long)c->num_cus * occ;
  const long long need_blocks = (n_items + block - 1) / block;
  grid = std::max(std::min(grid, need_blocks), 1ll);
  if (q.block_cap > 0) grid = std::min(grid, (long long)q.block_cap);
  const unsigned long long n_lanes = (unsigned long long)grid * block;
  int rc;
  if ((rc = c->q_counters.ensure(kQueryCounters * sizeof(unsigned long long)))) return rc;
  if (kernel == RTOW_KERNEL_BVH4) {
    const int extra = std::max(q.shape.stack_bound - (int)q.shape.scene.b4_stack_k, 0);
    if ((rc = c->q_spill.ensure(std::max<size_t>((size_t)extra * (size_t)n_lanes * sizeof(uint32_t), 16)))) return rc;
  }
  rtow::TraceParams P;
  std::memset(&P, 0, sizeof P);
  P.sc = q.shape.scene;
  P.n_lanes = (uint32_t)n_lanes;
  P.spill = (uint32_t *)c->q_spill.p;
  // every walk runs to completion (cap 0xffffffff); the leaf-phase quorum is the render's
  const bool b4 = kernel == RTOW_KERNEL_BVH4;
  P.walk_cap = 0xffffffffu;
  P.walk_max_open = 64u;
  P.leaf_votes = (uint32_t)(c->knobs.leaf_votes > 0 ? c->knobs.leaf_votes : (b4 ? 28 : 16));
  if ((rc = fill(P, a))) return rc;

  hipStream_t st = (hipStream_t)hip_stream;
  if (stats && !c->q_ev[0]) {
    for (hipEvent_t &e : c->q_ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipHostMalloc((void **)&c->h_qcounters, kQueryCounters * sizeof(unsigned long long), hipHostMallocDefault));
  }
  if (st != nullptr) HIPCHK(hipStreamWaitEvent(st, c->upload_ev, 0));  // the scene upload was queued on the null stream
  if (stats) HIPCHK(hipEventRecord(c->q_ev[0], st));
  HIPCHK(hipMemsetAsync(c->q_counters.p, 0, kQueryCounters * sizeof(unsigned long long), st));
  if (stats) HIPCHK(hipEventRecord(c->q_ev[1], st));
  a.counters = (unsigned long long *)c->q_counters.p;
  const int lrc = k.launch[build](P, a, kernel, (int)grid, block, q.lds, hip_stream);
  if (lrc != 0) return fail(RTOW_EHIP, "query kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
  if (stats) {
    HIPCHK(hipEventRecord(c->q_ev[2], st));
    HIPCHK(hipMemcpyAsync(c->h_qcounters, a.counters, kQueryCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->q_ev[3], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->q_ev[1], c->q_ev[2]));
    stats->kernel_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, c->q_ev[0], c->q_ev[3]));
    stats->total_ms = ms;
    stats->segments = (uint64_t)n_items;
    stats->prim_tests = c->h_qcounters[0];
    stats->node_tests = kernel == RTOW_KERNEL_BRUTE ? 0u : c->h_qcounters[1];
    if (k.brute_tests_all && kernel == RTOW_KERNEL_BRUTE) stats->prim_tests = (uint64_t)n_items * (uint64_t)c->n_prims;
  }
  return RTOW_OK;
}

// the row's buffers as the launcher's arguments
QueryArgs query_args(const QueryKind &k, void *const *buf) {
  QueryArgs a;
  for (int i = 0; i < k.n_bufs; ++i)
    if (k.bufs[i].arg) a.*k.bufs[i].arg = buf[i];
    else a.in = buf[i];
  return a;
}

// ---- the host forms' staging: a row's buffers through the context's q_* members ------------------------------------------
size_t buf_bytes(const QueryBuf &b, int64_t n, int32_t k) { return (size_t)n * (b.per_k ? (size_t)k : 1u) * b.item_bytes; }

// Device buffers for the arrays that were given (an optional array that was not stays NULL), the inputs copied in.
int stage_in(rtow_ctx *c, const QueryKind &k, void *const *host, int64_t n, int32_t kk, void **dev) {
  for (int i = 0; i < k.n_bufs; ++i) {
    DevBuf &d = c->*k.bufs[i].stage;
    if (host[i])
      if (int rc = d.ensure(buf_bytes(k.bufs[i], n, kk))) return rc;
    dev[i] = host[i] ? d.p : nullptr;
  }
  for (int i = 0; i < k.n_bufs; ++i)
    if (host[i] && !k.bufs[i].out) HIPCHK(hipMemcpy(dev[i], host[i], buf_bytes(k.bufs[i], n, kk), hipMemcpyHostToDevice));
  return RTOW_OK;
}
int stage_out(const QueryKind &k, void *const *host, int64_t n, int32_t kk, void *const *dev) {
  for (int i = 0; i < k.n_bufs; ++i)
    if (host[i] && k.bufs[i].out) HIPCHK(hipMemcpy(host[i], dev[i], buf_bytes(k.bufs[i], n, kk), hipMemcpyDeviceToHost));
  return RTOW_OK;
}

// ---- the two entry forms of every row ------------------------------------------------------------------------------------
int query_device(rtow_ctx *c, const QueryKind &k, const QueryCall &call) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  if (k.has_params && !call.params) return fail(RTOW_EINVAL, "params is NULL");
  int rc;
  if ((rc = check_counts(k, call)) || (rc = check_buffers(k, call.buf, call.n, "buffer", true))) return rc;
  if (k.check && (rc = k.check(call))) return rc;
  QueryRun q;
  if ((rc = query_begin(c, k, call.precision, call.kernel, call.stats, q))) return rc;
  if (call.n == 0) return RTOW_OK;

  QueryArgs a = query_args(k, call.buf);
  a.n = (uint32_t)call.n;
  a.k = call.k;
  if (k.mapped && (a.hits || k.map_always) && (rc = query_map_for(c, q.kernel, &a.map))) return rc;
  const int64_t n_items = k.grid_items ? k.grid_items(call) : call.n;
  rc = query_launch(c, k, q, a, n_items, call.stream, call.stats, [&](rtow::TraceParams &P, QueryArgs &args) {
    return k.fill ? k.fill(c, call, q.strict, P, args) : (int)RTOW_OK;
  });
  if (rc == RTOW_OK && call.stats && k.epilogue) k.epilogue(c, call, call.stats);
  return rc;
}

// (NULL arrays and a missing scene are refused before anything is allocated; n == 0 falls through to the device form)
int query_host(rtow_ctx *c, const QueryKind &k, const QueryCall &call) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  int rc;
  if ((rc = check_counts(k, call)) || (rc = check_buffers(k, call.buf, call.n, "array", false))) return rc;
  if (k.check_sizes_staging) {
    if (!call.params) return fail(RTOW_EINVAL, "params is NULL");
    if ((rc = k.check(call))) return rc;
  }
  QueryCall dev = call;
  dev.stream = nullptr;
  if (call.n == 0) {
    std::fill(dev.buf, dev.buf + kMaxQueryBufs, nullptr);
    return query_device(c, k, dev);
  }
  if (!c->have_scene) return fail(RTOW_ENOSCENE, "no scene uploaded");
  HIPCHK(hipSetDevice(c->device));
  if ((rc = stage_in(c, k, call.buf, call.n, call.k, dev.buf)) || (rc = query_device(c, k, dev))) return rc;
  return stage_out(k, call.buf, call.n, call.k, dev.buf);
}

// ---- the camera stage (rtow_camera_rays*, rtow_guides*) ---------------------------------------------------------------------
// Kernels that generate the render's primaries themselves: the batch is not a count but what a render of `cfg` would
// trace on this rank — CameraCall: its rows and its sample set (level_plan's strict form: the reference's) — so the front
// ends are their own; the buffer checks, the staging and the launch are the rows' (kCameraRays, kGuides).
struct CameraCall {
  int rows = 0;
  long long npix = 0;         // rows * W
  uint32_t sample_first = 0;  // stream_first * (spp / nstreams)
  long long samples = 0;      // (spp / nstreams) * streams of the call
};
int camera_call(const rtow_config_t *cfg, CameraCall &k) {
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  if (cfg->precision == RTOW_F32) return fail(RTOW_EINVAL, "camera rays / guides: RTOW_F32 is not supported (binary64 builds only)");
  const long long spt = cfg->samples_per_pixel / cfg->nstreams;  // src/render.cpp:174
  const long long streams_now = cfg->stream_count > 0 ? cfg->stream_count : cfg->nstreams;
  if (spt * ((long long)cfg->stream_first + streams_now) > 0xffffffffLL) return fail(RTOW_EINVAL, "sample index beyond 32 bits");
  k.rows = rtow_local_rows(cfg);
  k.npix = (long long)k.rows * cfg->image_width;
  k.sample_first = (uint32_t)((long long)cfg->stream_first * spt);
  k.samples = spt * streams_now;
  if (k.samples > 0x7fffffffLL) return fail(RTOW_EINVAL, "%lld samples per pixel in one call", k.samples);
  return RTOW_OK;
}
// the launch of either kernel: n_items queue positions or rays; the camera's share of the launch parameters is what
// render_levels sets for the new-ray stage
int camera_launch(rtow_ctx *c, const QueryKind &kind, const QueryRun &q, const rtow_config_t *cfg, const CameraCall &k,
                  void *const *buf, long long n_items, void *hip_stream, rtow_stats_t *stats) {
  QueryArgs a = query_args(kind, buf);
  a.n = (uint32_t)n_items;
  a.sample_first = k.sample_first;
  a.samples = (int32_t)k.samples;
  return query_launch(c, kind, q, a, n_items, hip_stream, stats, [&](rtow::TraceParams &P, QueryArgs &) {
    P.cam = (const rtow::DevCamera *)c->cam_dev.p;
    P.W = cfg->image_width;
    P.H = cfg->image_height;
    P.inv_wm1 = 1.0 / (double)(cfg->image_width - 1);
    P.inv_hm1 = 1.0 / (double)(cfg->image_height - 1);
    P.rank = cfg->rank;
    P.nranks = cfg->nranks;
    P.tile_rows = cfg->tile_rows;
    P.local_rows = k.rows;
    P.seed_lo = (uint32_t)cfg->seed;
    P.seed_hi = (uint32_t)(cfg->seed >> 32);
    return (int)RTOW_OK;
  });
}
// the host forms behind their own checks: stage, run the device form, copy back
template <class Device>
int camera_host(rtow_ctx *c, const QueryKind &kind, void *const *host, long long n, Device &&device) {
  if (!c->have_scene) return fail(RTOW_ENOSCENE, "no scene uploaded");
  HIPCHK(hipSetDevice(c->device));
  void *dev[kMaxQueryBufs] = {};
  int rc;
  if ((rc = stage_in(c, kind, host, n, 1, dev)) || (rc = device(dev))) return rc;
  return stage_out(kind, host, n, 1, dev);
}

// host = false: device buffers, launched on `hip_stream`; host = true: the caller's arrays, staged around the device form
int run_camera_rays(rtow_ctx *c, const rtow_config_t *cfg, void *rays, void *ids, void *hip_stream, bool host) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  CameraCall k;
  int rc;
  if ((rc = camera_call(cfg, k))) return rc;
  const long long n = k.npix * k.samples;  // (< 2^62)
  if (n > kMaxQueryRays) return fail(RTOW_EINVAL, "rows * width * samples = %lld beyond 2^31 - 64", n);
  void *const buf[kMaxQueryBufs] = {rays, ids};
  if ((rc = check_buffers(kCameraRays, buf, n, host ? "array" : "buffer", !host))) return rc;
  if (host && n > 0)
    return camera_host(c, kCameraRays, buf, n, [&](void *const *dev) { return run_camera_rays(c, cfg, dev[0], dev[1], nullptr, false); });
  QueryRun q;
  if ((rc = query_begin(c, kCameraRays, cfg->precision, cfg->kernel, nullptr, q))) return rc;
  if (n == 0) return RTOW_OK;
  return camera_launch(c, kCameraRays, q, cfg, k, buf, n, hip_stream, nullptr);
}

int run_guides(rtow_ctx *c, const rtow_config_t *cfg, void *guides_out, void *hip_stream, rtow_stats_t *stats, bool host) {
  if (!c) return fail(RTOW_EINVAL, "ctx is NULL");
  CameraCall k;
  int rc;
  if ((rc = camera_call(cfg, k))) return rc;
  void *const buf[kMaxQueryBufs] = {guides_out};
  if (host) {
    if ((rc = check_buffers(kGuides, buf, k.npix, "array", false))) return rc;
    if (k.npix > 0)
      return camera_host(c, kGuides, buf, k.npix, [&](void *const *dev) { return run_guides(c, cfg, dev[0], nullptr, stats, false); });
  }
  // queue positions: 8 x 8 tiles over the rank's rows, 64 positions each (csrc/rtow_guides.h)
  const long long tiles = (((long long)cfg->image_width + 7) / 8) * (((long long)k.rows + 7) / 8);
  if (tiles * 64 > 0xfffffff0LL) return fail(RTOW_EINVAL, "too many pixels (%lld)", k.npix);
  if (!host && (rc = check_buffers(kGuides, buf, k.npix, "buffer", true))) return rc;
  QueryRun q;
  if ((rc = query_begin(c, kGuides, cfg->precision, cfg->kernel, stats, q))) return rc;
  if (stats) stats->local_rows = k.rows;
  if (k.npix == 0) return RTOW_OK;
  if (k.samples == 0) {  // fewer samples than streams: zero effective samples (src/render.cpp:174), zero sums
    HIPCHK(hipMemsetAsync(guides_out, 0, (size_t)k.npix * sizeof(rtow_guide_t), (hipStream_t)hip_stream));
    if (stats) HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    return RTOW_OK;
  }
  rc = camera_launch(c, kGuides, q, cfg, k, buf, tiles * 64, hip_stream, stats);
  if (rc == RTOW_OK && stats) {
    stats->samples = stats->segments = (uint64_t)k.npix * (uint64_t)k.samples;
    if (q.kernel == RTOW_KERNEL_BRUTE) stats->prim_tests = stats->segments * (uint64_t)c->n_prims;  // (its walk tests all, uncounted)
  }
  return rc;
}

}  // namespace

// ---- the guarded entry points (guarded(), rtow_ctx.h) ---------------------------------------------------------------------
extern "C" {

int64_t rtow_camera_ray_count(const rtow_config_t *cfg) {
  CameraCall k;
  if (int rc = camera_call(cfg, k)) return rc;
  return (int64_t)(k.npix * k.samples);
}

int rtow_intersect_device(rtow_ctx *c, int32_t precision, int32_t kernel, const void *d_rays, int64_t n_rays, void *d_hits,
                          void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_intersect_device", [&] {
    return query_device(c, kIntersect, {precision, kernel, n_rays, 0, nullptr, {(void *)d_rays, d_hits}, hip_stream, stats});
  });
}
int rtow_intersect(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_ray_t *rays, int64_t n_rays, rtow_hit_t *hits,
                   rtow_stats_t *stats) {
  return guarded("rtow_intersect", [&] {
    return query_host(c, kIntersect, {precision, kernel, n_rays, 0, nullptr, {(void *)rays, hits}, nullptr, stats});
  });
}
int rtow_occluded_device(rtow_ctx *c, int32_t precision, int32_t kernel, const void *d_rays, int64_t n_rays,
                         void *d_occluded, void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_occluded_device", [&] {
    return query_device(c, kOccluded, {precision, kernel, n_rays, 0, nullptr, {(void *)d_rays, d_occluded}, hip_stream, stats});
  });
}
int rtow_occluded(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_ray_t *rays, int64_t n_rays, uint8_t *occluded,
                  rtow_stats_t *stats) {
  return guarded("rtow_occluded", [&] {
    return query_host(c, kOccluded, {precision, kernel, n_rays, 0, nullptr, {(void *)rays, occluded}, nullptr, stats});
  });
}
int rtow_closest_point_device(rtow_ctx *c, int32_t precision, int32_t kernel, const void *d_queries, int64_t n,
                              void *d_hits, void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_closest_point_device", [&] {
    return query_device(c, kClosestPoint, {precision, kernel, n, 0, nullptr, {(void *)d_queries, d_hits}, hip_stream, stats});
  });
}
int rtow_closest_point(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_point_query_t *queries, int64_t n,
                       rtow_point_hit_t *hits, rtow_stats_t *stats) {
  return guarded("rtow_closest_point", [&] {
    return query_host(c, kClosestPoint, {precision, kernel, n, 0, nullptr, {(void *)queries, hits}, nullptr, stats});
  });
}
int rtow_nearest_device(rtow_ctx *c, int32_t precision, int32_t kernel, const void *d_queries, int64_t n, int32_t k,
                        void *d_hits, void *d_counts, void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_nearest_device", [&] {
    return query_device(c, kNearest, {precision, kernel, n, k, nullptr, {(void *)d_queries, d_hits, d_counts}, hip_stream, stats});
  });
}
int rtow_nearest(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_point_query_t *queries, int64_t n, int32_t k,
                 rtow_point_hit_t *hits, int32_t *counts, rtow_stats_t *stats) {
  return guarded("rtow_nearest", [&] {
    return query_host(c, kNearest, {precision, kernel, n, k, nullptr, {(void *)queries, hits, counts}, nullptr, stats});
  });
}
int rtow_first_hits_device(rtow_ctx *c, int32_t precision, int32_t kernel, const void *d_rays, int64_t n_rays,
                           int32_t max_hits, void *d_hits, void *d_counts, void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_first_hits_device", [&] {
    return query_device(c, kFirstHits,
                        {precision, kernel, n_rays, max_hits, nullptr, {(void *)d_rays, d_hits, d_counts}, hip_stream, stats});
  });
}
int rtow_first_hits(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_ray_t *rays, int64_t n_rays, int32_t max_hits,
                    rtow_hit_t *hits, int32_t *counts, rtow_stats_t *stats) {
  return guarded("rtow_first_hits", [&] {
    return query_host(c, kFirstHits, {precision, kernel, n_rays, max_hits, nullptr, {(void *)rays, hits, counts}, nullptr, stats});
  });
}
int rtow_radiance_device(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_radiance_params_t *params,
                         const void *d_rays, int64_t n_rays, const void *d_ids, void *d_rgb_sums, void *hip_stream,
                         rtow_stats_t *stats) {
  return guarded("rtow_radiance_device", [&] {
    return query_device(c, kRadiance,
                        {precision, kernel, n_rays, 0, params, {(void *)d_rays, (void *)d_ids, d_rgb_sums}, hip_stream, stats});
  });
}
int rtow_radiance(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_radiance_params_t *params, const rtow_ray_t *rays,
                  int64_t n_rays, const uint32_t *ids, double *rgb_sums, rtow_stats_t *stats) {
  return guarded("rtow_radiance", [&] {
    return query_host(c, kRadiance, {precision, kernel, n_rays, 0, params, {(void *)rays, (void *)ids, rgb_sums}, nullptr, stats});
  });
}
int rtow_path_step_device(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_step_params_t *params, const void *d_rays,
                          int64_t n_rays, const void *d_ids, void *d_next, void *d_atten, void *d_status, void *d_hits,
                          void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_path_step_device", [&] {
    return query_device(c, kStep, {precision, kernel, n_rays, 0, params,
                                   {(void *)d_rays, (void *)d_ids, d_next, d_atten, d_status, d_hits}, hip_stream, stats});
  });
}
int rtow_path_step(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_step_params_t *params, const rtow_ray_t *rays,
                   int64_t n_rays, const uint32_t *ids, rtow_ray_t *next, double *atten, int32_t *status, rtow_hit_t *hits,
                   rtow_stats_t *stats) {
  return guarded("rtow_path_step", [&] {
    return query_host(c, kStep, {precision, kernel, n_rays, 0, params,
                                 {(void *)rays, (void *)ids, next, atten, status, hits}, nullptr, stats});
  });
}
int rtow_ambient_device(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_ambient_params_t *params,
                        const void *d_points, int64_t n, const void *d_ids, void *d_out, void *d_rays_out, void *hip_stream,
                        rtow_stats_t *stats) {
  return guarded("rtow_ambient_device", [&] {
    return query_device(c, kAmbient, {precision, kernel, n, params ? params->samples : 0, params,
                                      {(void *)d_points, (void *)d_ids, d_out, d_rays_out}, hip_stream, stats});
  });
}
int rtow_ambient(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_ambient_params_t *params,
                 const rtow_surface_point_t *points, int64_t n, const uint32_t *ids, rtow_ambient_t *out, rtow_ray_t *rays_out,
                 rtow_stats_t *stats) {
  return guarded("rtow_ambient", [&] {
    return query_host(c, kAmbient, {precision, kernel, n, params ? params->samples : 0, params,
                                    {(void *)points, (void *)ids, out, rays_out}, nullptr, stats});
  });
}
int rtow_sweep_device(rtow_ctx *c, int32_t precision, int32_t kernel, const void *d_queries, int64_t n, void *d_hits,
                      void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_sweep_device", [&] {
    return query_device(c, kSweep, {precision, kernel, n, 0, nullptr, {(void *)d_queries, d_hits}, hip_stream, stats});
  });
}
int rtow_sweep(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_sweep_t *queries, int64_t n, rtow_sweep_hit_t *hits,
               rtow_stats_t *stats) {
  return guarded("rtow_sweep", [&] {
    return query_host(c, kSweep, {precision, kernel, n, 0, nullptr, {(void *)queries, hits}, nullptr, stats});
  });
}
int rtow_overlap_device(rtow_ctx *c, int32_t precision, int32_t kernel, const void *d_queries, int64_t n, int32_t max_ids,
                        void *d_counts, void *d_ids, void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_overlap_device", [&] {
    return query_device(c, kOverlap, {precision, kernel, n, max_ids, nullptr, {(void *)d_queries, d_counts, d_ids}, hip_stream, stats});
  });
}
int rtow_overlap(rtow_ctx *c, int32_t precision, int32_t kernel, const rtow_box_query_t *queries, int64_t n, int32_t max_ids,
                 int32_t *counts, int32_t *ids, rtow_stats_t *stats) {
  return guarded("rtow_overlap", [&] {
    return query_host(c, kOverlap, {precision, kernel, n, max_ids, nullptr, {(void *)queries, counts, ids}, nullptr, stats});
  });
}
int rtow_camera_rays_device(rtow_ctx *c, const rtow_config_t *cfg, void *d_rays, void *d_ids, void *hip_stream) {
  return guarded("rtow_camera_rays_device", [&] { return run_camera_rays(c, cfg, d_rays, d_ids, hip_stream, false); });
}
int rtow_camera_rays(rtow_ctx *c, const rtow_config_t *cfg, rtow_ray_t *rays, uint32_t *ids) {
  return guarded("rtow_camera_rays", [&] { return run_camera_rays(c, cfg, rays, ids, nullptr, true); });
}
int rtow_guides_device(rtow_ctx *c, const rtow_config_t *cfg, void *d_guides, void *hip_stream, rtow_stats_t *stats) {
  return guarded("rtow_guides_device", [&] { return run_guides(c, cfg, d_guides, hip_stream, stats, false); });
}
int rtow_guides(rtow_ctx *c, const rtow_config_t *cfg, rtow_guide_t *guides, rtow_stats_t *stats) {
  return guarded("rtow_guides", [&] { return run_guides(c, cfg, guides, nullptr, stats, true); });
}

}  // extern "C"
