// rtow_overlap.h — the box-overlap query kernel (rtow_overlap / rtow_overlap_device, include/rtow.h), included by
// rtow_overlap_strict.hip and rtow_overlap_fast.hip, which differ only in -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller box [lo, hi] (with a shutter time and a first insertion index min_prim), the set O
// of primitives with insertion index >= min_prim whose geometry — closed triangles, sphere SURFACES — overlaps the closed
// box, by the predicates of rtow_overlap_walks.h: the count |O|, uncapped, and on request the max_ids (1 .. 8) lowest
// insertion indices of O, ascending, the unused slots -1.  A caller pages through all of O by asking again with
// min_prim = last id + 1.
//
// The predicate of a pair depends on nothing but the pair, and the walks prune conservatively with respect to it
// (that header), so count and ids are the same under every walk, builder and schedule: in the strict build bit-determined.
//
// Execution model: that of the k-nearest query (rtow_nearest.h): persistent waves of 64 consecutive queries, the scene
// image staged in LDS per workgroup, lanes past n and skipped queries (a NaN or an infinity among lo, hi, time; lo > hi
// in a component) entering the walks inactive while the wave keeps voting.  A lane reads its query with four 16-byte
// loads and writes its count and its max_ids ids with vector stores; the list is not kept when no ids are asked for.

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
#include "rtow_overlap_walks.h"

struct OverlapParams {
  TraceParams P;                 // the scene (P.sc) and the walks' launch fields: spill, n_lanes, leaf_votes
  const unsigned char *queries;  // [n][64 B], 16-byte aligned
  int32_t *counts;               // [n]
  int32_t *ids;                  // [n][max_ids], or nullptr
  uint32_t n;
  int32_t max_ids;               // 1 .. 8 (RTOW_MAX_OVERLAP_IDS, include/rtow.h: the list has eight slots)
  const int32_t *map;            // walk's primitive id -> insertion index
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

__device__ __forceinline__ bool overlap_finite(double x) { return fabs(x) < __builtin_huge_val(); }  // (NaN: false)

// KERNEL: 1 = BRUTE, 2 = BVH, 4 = BVH4; LDS: the scene image is staged in LDS (stage_scene, rtow_kernel_frame.h)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 ? 1024 : 256) RTOW_CAT(rtow_overlap_, RTOW_SUFFIX)(const OverlapParams Q) {
  const TraceParams &P = Q.P;
  const DevScene &sc = P.sc;
  const unsigned lane = lane_id();
  [[maybe_unused]] const uint32_t lane_g = blockIdx.x * blockDim.x + threadIdx.x;
  const int max_ids = Q.max_ids;

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
    V3d lo = {0, 0, 0}, hi = {0, 0, 0};
    double time = 0.0;
    int32_t min_prim = 0;
    if (in) load_box_query(Q.queries, i, lo, hi, time, min_prim);
    // skipped (count 0, ids -1, no walk): a NaN or an infinity among lo, hi and time; lo > hi in a component
    const bool active = in && overlap_finite(lo.x) && overlap_finite(lo.y) && overlap_finite(lo.z) &&
                        overlap_finite(hi.x) && overlap_finite(hi.y) && overlap_finite(hi.z) && overlap_finite(time) &&
                        lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
    OvBox b;
    b.lo = lo;
    b.hi = hi;
    b.time = time;
    OverlapSink out;
    out.clear();
    out.min_prim = min_prim > 0 ? min_prim : 0;
    out.keep = Q.ids != nullptr;
    out.map = Q.map;
    if constexpr (KERNEL == 4) {
      overlap_bvh4<LDS>(im4, sc, P, b, active, lane_g, out, nnode, nprim);
    } else if constexpr (KERNEL == 2) {
      overlap_bvh<LDS>(im, sc, b, active, out, nnode, nprim);
    } else {
      overlap_brute(sc, b, active, out, nprim);
    }

    if (in) {
      Q.counts[i] = out.count;
      if (Q.ids != nullptr) {
        int32_t *dst = Q.ids + (size_t)i * (size_t)max_ids;
        for (int j = 0; j < max_ids; ++j) dst[j] = out.entry(j);
      }
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<OverlapParams> overlap_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_overlap_, RTOW_SUFFIX)<K, L>, OverlapParams>(lds_bytes);
}

// kernel: 1 BRUTE, 2 BVH, 4 BVH4: the instantiation set of the point queries (pointq_variant, rtow_pointq.h)
static KernelVariant<OverlapParams> overlap_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return overlap_kernel<1, false>(0);
    case 2: return lds_bytes > 0 ? overlap_kernel<2, true>(lds_bytes) : overlap_kernel<2, false>(0);
    case 4: return b4_full ? overlap_kernel<4, true>(lds_bytes) : overlap_kernel<4, false>(lds_bytes);
    default: return {};
  }
}

int RTOW_CAT(launch_overlap_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                           unsigned lds_bytes, void *stream) {
  OverlapParams q;
  q.P = p;
  q.queries = (const unsigned char *)a.in;
  q.counts = (int32_t *)a.counts;
  q.ids = (int32_t *)a.hits;
  q.n = a.n;
  q.max_ids = a.k;
  q.map = a.map;
  q.counters = a.counters;
  return launch_variant(overlap_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_CAT(overlap_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<OverlapParams> v = overlap_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
