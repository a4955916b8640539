// rtow_step.h — the path-step query kernel (rtow_path_step / rtow_path_step_device, include/rtow.h), included by
// rtow_step_strict.hip and rtow_step_fast.hip, which differ only in -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller ray ONE segment of the reference's ray_color (src/render.cpp:112-129) — the closest
// hit over [0.001, tmax], then Material::scatter (src/common-model.cpp:13-62) drawn from request 1 + bounce of the ray's
// Philox identity: the next ray, the attenuation, a status and (optionally) the hit record.  A caller who repeats it
// depth + 1 times and folds the attenuations computes what rtow_radiance computes, bit for bit in the strict build.
// The walks are the trace kernels', included read-only below exactly as rtow_query.h includes them; the hit record is
// rtow_hit_record.h's (the closest-hit query's); the shading surface, the scatter and the sky are rtow_scatter.h's (the
// radiance query's).
//
// Execution model (gfx950, wave64): rtow_query.h's — persistent waves, every wave takes 64 consecutive rays per step and
// strides over the batch; one ray is one work item and there is no queue.  Lanes past n_rays, and lanes whose ray is
// dead (tmax NaN or below 0.001), enter the walks with active = false (the walks vote across the wave).  A lane reads
// its 64-byte ray with four 16-byte loads before anything of index i is written, and touches no other index: `next` may
// be the ray array itself.  The next ray leaves with four 16-byte stores, the attenuation with three 8-byte stores (a
// 24-byte stride), the status with one 4-byte store.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtow_device.h"

#ifndef RTOW_SUFFIX
#error "define RTOW_SUFFIX"
#endif

namespace rtow {
namespace {
#include "rtow_trace_math.h"
#include "rtow_trace_rng.h"
#include "rtow_trace_hit.h"
#include "rtow_trace_stamps.h"
#include "rtow_trace_bvh.h"
#include "rtow_trace_grid.h"
#include "rtow_trace_bvh4.h"
#ifndef RTOW_FAST_MATH
#include "rtow_trace_reftree.h"
#endif
#include "rtow_kernel_frame.h"
#include "rtow_hit_record.h"
#include "rtow_scatter.h"

struct StepParams {
  TraceParams P;               // the scene (P.sc), seed_lo / seed_hi, and the walks' launch fields
  const unsigned char *rays;   // [n][64 B], 16-byte aligned
  const uint32_t *ids;         // [n][2] (pixel, sample), 8-byte aligned, or NULL: (i, 0)
  unsigned char *next;         // [n][64 B], 16-byte aligned; may be `rays`
  double *atten;               // [n][3]
  int32_t *status;             // [n] RTOW_STEP_*
  unsigned char *hits;         // [n][72 B], 8-byte aligned, or NULL
  uint32_t n;
  uint32_t request;            // 1 + bounce: the Philox request the scatter draws
  uint32_t sample_first;
  const int32_t *map;          // walk's primitive id -> insertion index
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

// RTOW_STEP_* of include/rtow.h
constexpr int32_t kStepMiss = 0, kStepScattered = 1, kStepAbsorbed = 2, kStepSkipped = 3;

// KERNEL: 1 = STREAM, 2 = BVH, 3 = GRID, 4 = BVH4, 5 = REFTREE (strict build only); LDS: the scene image is staged in
// LDS (2 and 3; for 4: the whole image, else the top of its tree — the traversal stack is in LDS either way)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 && KERNEL <= 4 ? 1024 : 256)
    RTOW_CAT(rtow_step_, RTOW_SUFFIX)(const StepParams Q) {
  const TraceParams &P = Q.P;
  const DevScene &sc = P.sc;
  const unsigned lane = lane_id();
  [[maybe_unused]] const uint32_t lane_g = blockIdx.x * blockDim.x + threadIdx.x;

  Image<LDS> im;
  [[maybe_unused]] Bvh4Reader<LDS> im4;
  stage_scene<KERNEL, LDS>(sc, im, im4);

  uint32_t nnode = 0u, nprim = 0u;
  Stamps<false> stamps;
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  // wave-uniform loop: every lane of the wave runs every step (the walks vote across the wave)
  for (uint32_t base = wave * 64u; base < Q.n; base += n_waves * 64u) {
    const uint32_t i = base + lane;
    const bool active = i < Q.n;
    V3 ro = {0, 0, 0}, rd = {0, 0, 1};
    real rtime = 0;
    double tmax = -1.0;
    Rng g = {i, Q.sample_first, Q.request};
    if (active) {
      load_ray(Q.rays, i, ro, rd, rtime, tmax);
      if (Q.ids != nullptr) {
        const uint2 id = reinterpret_cast<const uint2 *>(Q.ids)[i];
        g.pixel = id.x;
        g.sample = id.y + Q.sample_first;
      }
    }
    const bool live = active && tmax >= 0.001;  // (NaN compares false: a dead ray does no walk)

    // ---- closest hit over [0.001, inf): the render's walks, run to completion (cap = 0xffffffff) ----
    Closest best;
    best.t = (real)__builtin_huge_val();
    best.prim = -1;
    if constexpr (KERNEL == 4) {
      uint32_t w_cur = kRefNone, w_sa = 0u;
      best = closest_hit_bvh4<LDS, false>(im4, sc, P, ro, rd, rtime, live, lane_g, nnode, nprim, stamps, best, w_cur,
                                          w_sa, 0xffffffffu, P.walk_max_open);
    } else if constexpr (KERNEL == 3) {
      float t_resume = 0.0f;
      const V3 rd_walk = {plus_zero(rd.x), plus_zero(rd.y), plus_zero(rd.z)};
      best = closest_hit_grid<LDS, false>(im, sc, ro, rd_walk, rtime, live, nnode, nprim, stamps, best, t_resume,
                                          0xffffffffu, P.walk_max_open, P.leaf_votes);
    } else if constexpr (KERNEL == 2) {
      best = closest_hit_bvh<LDS, false>(im, sc, ro, rd, rtime, live, nnode, nprim, stamps);
    } else if constexpr (KERNEL == 5) {
#ifndef RTOW_FAST_MATH
      if (live) best = closest_hit_reftree(sc, to_f64(ro), to_f64(rd), (double)rtime, nnode, nprim);
#endif
    } else {
      best = closest_hit_stream(sc, to_f64(ro), to_f64(rd), (double)rtime, live);
    }

    // ---- the segment's end: the hit record, then scatter or the sky (tmax is a post-filter, as in rtow_query.h) ----
    const bool hit = live && best.prim >= 0 && best.t <= tmax;
    if (active && Q.hits != nullptr)
      write_hit_record<KERNEL, LDS>(im, im4, sc, Q.map, ro, rd, rtime, hit, best.prim, best.t,
                                    Q.hits + (size_t)i * kHitBytes);
    if (active) {
      // the dead ray: all fields 0, tmax = -1
      V3 no = {0, 0, 0}, nd = {0, 0, 0}, att = {0, 0, 0};
      real ntime = 0;
      double ntmax = -1.0;
      int32_t status = kStepSkipped;
      if (hit) {
        const V3 p = ro + rd * best.t;  // Ray::at: the origin of the scattered ray
        const Surface sf = surface_at<KERNEL, LDS>(im, im4, sc, p, rd, rtime, best.prim);
        V3 dir;
        status = kStepAbsorbed;
        if (scatter_dir(g, P.seed_lo, P.seed_hi, sf.kind, sf.fuzz, sf.ir, rd, sf.normal, sf.front, dir)) {
          status = kStepScattered;
          att = material_att<KERNEL, LDS>(im, im4, sc, (uint32_t)sf.mi);
          no = p;
          nd = dir;
          ntime = rtime;
          ntmax = __builtin_huge_val();
        }
      } else if (live) {
        status = kStepMiss;
        att = sky_color(rd);
      }
      vd2 *nx = reinterpret_cast<vd2 *>(Q.next + (size_t)i * kRayBytes);
      nx[0] = vd2{(double)no.x, (double)no.y};
      nx[1] = vd2{(double)no.z, (double)ntime};
      nx[2] = vd2{(double)nd.x, (double)nd.y};
      nx[3] = vd2{(double)nd.z, ntmax};
      double *a = Q.atten + (size_t)i * 3;
      a[0] = (double)att.x;
      a[1] = (double)att.y;
      a[2] = (double)att.z;
      Q.status[i] = status;
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

// kernel: 1 STREAM, 2 BVH, 3 GRID, 4 BVH4, 5 REFTREE (strict build): the instantiations of rtow_query.h
template <int K, bool L>
static KernelVariant<StepParams> step_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_step_, RTOW_SUFFIX)<K, L>, StepParams>(lds_bytes);
}

static KernelVariant<StepParams> step_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return step_kernel<1, false>(lds_bytes);  // (LDS: the tiled triangle loop's per-wave tiles)
    case 2: return lds_bytes > 0 ? step_kernel<2, true>(lds_bytes) : step_kernel<2, false>(0);
    case 3: return lds_bytes > 0 ? step_kernel<3, true>(lds_bytes) : step_kernel<3, false>(0);
    case 4: return b4_full ? step_kernel<4, true>(lds_bytes) : step_kernel<4, false>(lds_bytes);
#ifndef RTOW_FAST_MATH
    case 5: return step_kernel<5, false>(0);
#endif
    default: return {};
  }
}

// p: the scene, seed_lo / seed_hi, n_lanes, spill and the walk fields
int RTOW_CAT(launch_step_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                        unsigned lds_bytes, void *stream) {
  StepParams q;
  q.P = p;
  q.rays = (const unsigned char *)a.in;
  q.ids = (const uint32_t *)a.ids;
  q.next = (unsigned char *)a.next;
  q.atten = (double *)a.atten;
  q.status = (int32_t *)a.status;
  q.hits = (unsigned char *)a.hits;
  q.n = a.n;
  q.request = a.request;
  q.sample_first = a.sample_first;
  q.map = a.map;
  q.counters = a.counters;
  return launch_variant(step_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h), as query_occupancy_*.
int RTOW_CAT(step_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<StepParams> v = step_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
