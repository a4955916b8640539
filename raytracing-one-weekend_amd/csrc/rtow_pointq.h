// rtow_pointq.h — the closest-point (distance) query kernel (rtow_closest_point / rtow_closest_point_device,
// include/rtow.h), included by rtow_pointq_strict.hip and rtow_pointq_fast.hip, which differ only in -ffp-contract and in
// RTOW_SUFFIX.
//
// What it computes: for every caller point p (and shutter time), the primitive of the resident scene nearest to p —
// its distance, the nearest point on it, its insertion index, kind and material — if that distance is <= max_dist.
// The geometry is the device's records: sphere c and copysign(r^2, r), moving sphere c0 and c1 - c0 (centre
// c0 + time * (c1 - c0), as the hit tests form it), triangle a, e1, e2 and n = e1 x e2.  The radius is sqrt(|r^2|) of the
// record (every image carries r^2; a hollow sphere is the same surface as a solid one).
//
// The per-primitive formulas and the three walks (BRUTE, BVH, BVH4) are those of rtow_point_walks.h, shared with the
// k-nearest query, with the one-entry sink PBest below: the search radius starts at max_dist (inclusive), and a
// primitive is accepted when its distance <= best so far.
//
// Execution model: that of the ray queries (rtow_query.h): persistent waves of 64 consecutive queries, the scene image
// staged in LDS per workgroup as the render stages it, lanes past n (and queries whose max_dist is NaN or negative)
// entering the walks inactive while the wave keeps voting.  Three 16-byte loads per query, three 16-byte stores per
// 48-byte result; nothing is written past n.

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
#include "rtow_trace_bvh4.h"
#include "rtow_kernel_frame.h"
#include "rtow_point_walks.h"

struct PointParams {
  TraceParams P;                 // the scene (P.sc) and the walks' launch fields: spill, n_lanes, leaf_votes
  const unsigned char *queries;  // [n][48 B], 16-byte aligned
  unsigned char *hits;           // [n][48 B], 16-byte aligned
  uint32_t n;
  const int32_t *map;            // walk's primitive id -> insertion index
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

// The one-entry sink of the point walks: the best so far is the bound.
struct PBest {
  static constexpr bool kSerial = false;
  double d;  // distance of the best primitive so far (max_dist before any)
  int prim;  // walk-order id, -1 = none
  __device__ __forceinline__ void take(double dist, int id) {
    if (dist <= d) {
      d = dist;
      prim = id;
    }
  }
  __device__ __forceinline__ double bound() const { return d; }
};

// KERNEL: 1 = BRUTE, 2 = BVH, 4 = BVH4; LDS: the scene image is staged in LDS (stage_scene, rtow_kernel_frame.h)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 ? 1024 : 256) RTOW_CAT(rtow_pointq_, RTOW_SUFFIX)(const PointParams Q) {
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
    V3d p = {0, 0, 0};
    double time = 0.0, max_dist = -1.0;
    if (in) load_point_query(Q.queries, i, p, time, max_dist);
    // a radius that is NaN or negative finds nothing: the query skips the walk
    const bool active = in && max_dist >= 0.0;
    PBest best;
    best.d = max_dist;
    best.prim = -1;
    if constexpr (KERNEL == 4) {
      closest_bvh4<LDS>(im4, sc, P, p, active, lane_g, best, nnode, nprim);
    } else if constexpr (KERNEL == 2) {
      closest_bvh<LDS>(im, sc, p, time, active, best, nnode, nprim);
    } else {
      closest_brute(sc, p, time, active, best, nprim);
    }

    // ---- the result record: the winner's point recomputed by the same formulas, its material, insertion index ----
    if (in) {
      const bool hit = active && best.prim >= 0;
      double dist = __builtin_huge_val();
      V3d q = {0, 0, 0};
      int32_t prim = -1, kind = -1, mi = -1;
      if (hit) {
        dist = point_record<KERNEL, LDS>(im, im4, sc, best.prim, p, time, q, kind, mi);
        prim = Q.map[best.prim];
      }
      store_point_hit(Q.hits + (size_t)i * kPHitBytes, dist, q, prim, kind, mi);
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<PointParams> pointq_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_pointq_, RTOW_SUFFIX)<K, L>, PointParams>(lds_bytes);
}

// kernel: 1 BRUTE, 2 BVH, 4 BVH4.  `lds_bytes` > 0 selects the BVH variant that stages the image in LDS; for 4 the image
// staged whole (b4_half == 0) selects the full-LDS variant, as in the render.  BRUTE uses no LDS.
static KernelVariant<PointParams> pointq_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return pointq_kernel<1, false>(0);
    case 2: return lds_bytes > 0 ? pointq_kernel<2, true>(lds_bytes) : pointq_kernel<2, false>(0);
    case 4: return b4_full ? pointq_kernel<4, true>(lds_bytes) : pointq_kernel<4, false>(lds_bytes);
    default: return {};
  }
}

int RTOW_CAT(launch_pointq_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                          unsigned lds_bytes, void *stream) {
  const PointParams q = {p, (const unsigned char *)a.in, (unsigned char *)a.hits, a.n, a.map, a.counters};
  return launch_variant(pointq_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_CAT(pointq_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<PointParams> v = pointq_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
