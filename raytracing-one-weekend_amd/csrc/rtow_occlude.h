// rtow_occlude.h — the any-hit (occlusion) ray query kernel (rtow_occluded / rtow_occluded_device, include/rtow.h),
// included by rtow_occlude_strict.hip and rtow_occlude_fast.hip, which differ only in -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller ray, 1 if some primitive's hit test accepts a t in [0.001, tmax], else 0 — the
// shadow / visibility question.  The BVH, GRID and BVH4 walks are the tmax-bounded walks of rtow_bounded_walks.h with
// the any-hit sink of rtow_any_hit.h: one closest-so-far value seeded with tmax, and a lane that stops at the end of the
// first leaf phase in which it accepts a hit.  By the argument in rtow_bounded_walks.h the answer equals `closest hit over
// [0.001, inf) <= tmax`: bit-determined in the strict build, the same under every strategy.
//
// Execution model: that of the closest-hit query (rtow_query.h): persistent waves of 64 consecutive rays, the scene
// image staged in LDS per workgroup exactly as the render stages it, lanes past n_rays (and rays whose tmax is below
// 0.001 or NaN) entering the walks with active = false.  One byte per ray: a wave writes 64 contiguous bytes.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtow_device.h"

#ifndef RTOW_SUFFIX
#error "define RTOW_SUFFIX"
#endif

namespace rtow {
namespace {
#include "rtow_trace_math.h"
#include "rtow_trace_hit.h"
#include "rtow_trace_stamps.h"
#include "rtow_trace_bvh.h"
#include "rtow_trace_grid.h"
#include "rtow_trace_bvh4.h"
#ifndef RTOW_FAST_MATH
#include "rtow_trace_reftree.h"
#endif
#include "rtow_kernel_frame.h"
#include "rtow_bounded_walks.h"

struct OccludeParams {
  TraceParams P;               // the scene (P.sc) and the walks' launch fields: spill, n_lanes, leaf_votes
  const unsigned char *rays;   // [n][64 B], 16-byte aligned
  unsigned char *occluded;     // [n] bytes, 0 or 1
  uint32_t n;
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

#include "rtow_any_hit.h"

// KERNEL: 1 = STREAM, 2 = BVH, 3 = GRID, 4 = BVH4, 5 = REFTREE (strict build only); LDS: the scene image is staged in
// LDS (stage_scene, rtow_kernel_frame.h)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 && KERNEL <= 4 ? 1024 : 256)
    RTOW_CAT(rtow_occlude_, RTOW_SUFFIX)(const OccludeParams Q) {
  const TraceParams &P = Q.P;
  const DevScene &sc = P.sc;
  const unsigned lane = lane_id();
  [[maybe_unused]] const uint32_t lane_g = blockIdx.x * blockDim.x + threadIdx.x;

  Image<LDS> im;
  [[maybe_unused]] Bvh4Reader<LDS> im4;
  stage_scene<KERNEL, LDS>(sc, im, im4);

  uint32_t nnode = 0u, nprim = 0u;
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  // wave-uniform loop: every lane of the wave runs every step (the walks vote across the wave)
  for (uint32_t base = wave * 64u; base < Q.n; base += n_waves * 64u) {
    const uint32_t i = base + lane;
    const bool in = i < Q.n;
    V3 ro = {0, 0, 0}, rd = {0, 0, 1};
    real rtime = 0;
    double tmax = 0.0;
    if (in) load_ray(Q.rays, i, ro, rd, rtime, tmax);
    // a ray whose interval [0.001, tmax] is empty (tmax NaN included) hits nothing: it skips the walk
    const bool active = in && tmax >= RTOW_TMIN;

    bool hit = false;
    if constexpr (KERNEL == 4) {
      hit = any_hit_bvh4<LDS>(im4, sc, P, ro, rd, tmax, active, lane_g, nnode, nprim);
    } else if constexpr (KERNEL == 3) {
      hit = any_hit_grid<LDS>(im, sc, ro, rd, rtime, tmax, active, nnode, nprim, P.leaf_votes);
    } else if constexpr (KERNEL == 2) {
      hit = any_hit_bvh<LDS>(im, sc, ro, rd, rtime, tmax, active, nnode, nprim);
    } else if constexpr (KERNEL == 5) {
#ifndef RTOW_FAST_MATH
      // the reference's tree is an exactness mode: its closest hit, compared with tmax
      if (active) {
        const Closest best = closest_hit_reftree(sc, to_f64(ro), to_f64(rd), (double)rtime, nnode, nprim);
        hit = best.prim >= 0 && best.t <= tmax;
      }
#endif
    } else {
      hit = any_hit_stream(sc, to_f64(ro), to_f64(rd), (double)rtime, tmax, active, nprim);
    }
    if (in) Q.occluded[i] = hit ? 1u : 0u;
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<OccludeParams> occlude_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_occlude_, RTOW_SUFFIX)<K, L>, OccludeParams>(lds_bytes);
}

// kernel: 1 STREAM, 2 BVH, 3 GRID, 4 BVH4, 5 REFTREE (strict build).  `lds_bytes` > 0 selects the variant that stages
// the image in LDS (2, 3); for 4 the image staged whole (b4_half == 0) selects the full-LDS variant, as in the render.
static KernelVariant<OccludeParams> occlude_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return occlude_kernel<1, false>(lds_bytes);  // (LDS: the tiled triangle loop's per-wave tiles)
    case 2: return lds_bytes > 0 ? occlude_kernel<2, true>(lds_bytes) : occlude_kernel<2, false>(0);
    case 3: return lds_bytes > 0 ? occlude_kernel<3, true>(lds_bytes) : occlude_kernel<3, false>(0);
    case 4: return b4_full ? occlude_kernel<4, true>(lds_bytes) : occlude_kernel<4, false>(lds_bytes);
#ifndef RTOW_FAST_MATH
    case 5: return occlude_kernel<5, false>(0);
#endif
    default: return {};
  }
}

int RTOW_CAT(launch_occlude_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                           unsigned lds_bytes, void *stream) {
  OccludeParams q;
  q.P = p;
  q.rays = (const unsigned char *)a.in;
  q.occluded = (unsigned char *)a.result;
  q.n = a.n;
  q.counters = a.counters;
  return launch_variant(occlude_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_CAT(occlude_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<OccludeParams> v = occlude_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
