// rtow_sweep.h — the swept-sphere (sphere cast) query kernel (rtow_sweep / rtow_sweep_device, include/rtow.h), included
// by rtow_sweep_strict.hip and rtow_sweep_fast.hip, which differ only in -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller sweep — a sphere of radius rho whose centre travels o + d t, t in [0, tmax], at
// shutter time `time` — the first primitive of the resident scene the sphere touches: the t of the contact, the
// centre there, the primitive's closest point to that centre and its distance (the contact point; ~rho), insertion
// index, kind and material, and whether the sphere already touched at t = 0.  The geometry is that of the
// closest-point query (rtow_pointq.h): the device's records, the sphere SURFACE | |p - c| - R |.
//
// The per-primitive formulas and the three walks (BRUTE, BVH, BVH4) are those of rtow_sweep_walks.h; the answer is the
// minimum by (t, insertion index).  The record's dist and point are point_record (rtow_point_walks.h) at the centre.
//
// Execution model: that of the point queries (rtow_pointq.h): persistent waves of 64 consecutive queries, the scene
// image staged in LDS per workgroup, lanes past n and skipped queries entering the walks inactive while the wave keeps
// voting.  Five 16-byte loads per query, five 16-byte stores per 80-byte result; nothing is written past n.

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
#include "rtow_sweep_walks.h"

struct SweepParams {
  TraceParams P;                 // the scene (P.sc) and the walks' launch fields: spill, n_lanes, leaf_votes
  const unsigned char *queries;  // [n][80 B], 16-byte aligned
  unsigned char *hits;           // [n][80 B], 16-byte aligned
  uint32_t n;
  const int32_t *map;            // walk's primitive id -> insertion index
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

__device__ __forceinline__ bool sweep_finite(double x) { return fabs(x) < __builtin_huge_val(); }  // (NaN: false)

// KERNEL: 1 = BRUTE, 2 = BVH, 4 = BVH4; LDS: the scene image is staged in LDS (stage_scene, rtow_kernel_frame.h)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 ? 1024 : 256) RTOW_CAT(rtow_sweep_, RTOW_SUFFIX)(const SweepParams Q) {
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
    SweepRay ray = {{0, 0, 0}, {0, 0, 1}, 0.0, 0.0, 1.0};
    double tmax = -1.0;
    if (in) load_sweep(Q.queries, i, ray, tmax);
    // skipped (the miss record, no walk): a NaN word; rho negative or infinite; tmax negative; d.d zero or infinite;
    // o or time infinite
    const double a = dot(ray.d, ray.d);
    const bool active = in && sweep_finite(ray.o.x) && sweep_finite(ray.o.y) && sweep_finite(ray.o.z) &&
                        sweep_finite(ray.time) && ray.rho >= 0.0 && sweep_finite(ray.rho) && tmax >= 0.0 && a > 0.0 &&
                        sweep_finite(a);
    ray.inv_a = active ? pq_div(1.0, a) : 1.0;
    SweepBest best;
    best.t = tmax;
    best.prim = -1;
    best.ov = false;
    if constexpr (KERNEL == 4) {
      sweep_bvh4<LDS>(im4, sc, P, ray, active, lane_g, Q.map, best, nnode, nprim);
    } else if constexpr (KERNEL == 2) {
      sweep_bvh<LDS>(im, sc, ray, active, Q.map, best, nnode, nprim);
    } else {
      sweep_brute(sc, ray, active, Q.map, best, nprim);
    }

    // ---- the result record: the centre at the contact, the winner's closest point to it by point_record ----
    if (in) {
      const bool hit = active && best.prim >= 0;
      double t = __builtin_huge_val(), dist = __builtin_huge_val();
      V3d c = {0, 0, 0}, q = {0, 0, 0};
      int32_t prim = -1, kind = -1, mi = -1, ov = 0;
      if (hit) {
        t = best.t;
        c = ray.o + ray.d * t;
        dist = point_record<KERNEL, LDS, true>(im, im4, sc, best.prim, c, ray.time, q, kind, mi);
        prim = Q.map[best.prim];
        ov = best.ov ? 1 : 0;
      }
      store_sweep_hit(Q.hits + (size_t)i * kSweepHitBytes, t, dist, c, q, prim, kind, mi, ov);
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<SweepParams> sweep_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_sweep_, RTOW_SUFFIX)<K, L>, SweepParams>(lds_bytes);
}

// kernel: 1 BRUTE, 2 BVH, 4 BVH4: the instantiation set of the point queries (pointq_variant, rtow_pointq.h)
static KernelVariant<SweepParams> sweep_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return sweep_kernel<1, false>(0);
    case 2: return lds_bytes > 0 ? sweep_kernel<2, true>(lds_bytes) : sweep_kernel<2, false>(0);
    case 4: return b4_full ? sweep_kernel<4, true>(lds_bytes) : sweep_kernel<4, false>(lds_bytes);
    default: return {};
  }
}

int RTOW_CAT(launch_sweep_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                         unsigned lds_bytes, void *stream) {
  const SweepParams q = {p, (const unsigned char *)a.in, (unsigned char *)a.hits, a.n, a.map, a.counters};
  return launch_variant(sweep_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_CAT(sweep_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<SweepParams> v = sweep_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
