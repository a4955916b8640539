// rtow_nearest.h — the k-nearest-primitive (ordered distance) query kernel (rtow_nearest / rtow_nearest_device,
// include/rtow.h), included by rtow_nearest_strict.hip and rtow_nearest_fast.hip, which differ only in -ffp-contract and
// in RTOW_SUFFIX.
//
// What it computes: for every caller point p (and shutter time), the set N of primitives whose distance — the formulas
// of the closest-point query (rtow_point_walks.h), one entry per primitive — is <= max_dist, ordered ascending by
// (dist, insertion index) and cut at k (1 .. 8): k full rtow_point_hit_t records per query (the unused ones the miss
// record) and the count.
//
// The walks are the three point walks of rtow_point_walks.h with the list sink below: the bound is max_dist while the
// lane's list holds fewer than k entries and the distance of entry k - 1 after that.  Once k entries are kept, a
// primitive farther than the last of them cannot enter; one at the same distance still can (lower insertion index), and
// the walks visit every member of a tie at the bound (that header: inclusive comparisons, the slack sigma, a bound that
// only shrinks).  Hence the kept list equals "all of N, sorted, cut at k", whatever order the walk met the primitives
// in: bit-determined in the strict build, the same under every walk, builder and schedule.
//
// The list: 8 (dist, walk id) pairs per lane in registers (rtow_sorted_list.h), sorted by (dist, insertion index).  A
// candidate beyond the bound is dropped before the list is touched (so is a NaN: it compares false), and one whose
// primitive is already kept is dropped by the list (the trees hold every primitive once; the check costs eight
// compares on the few candidates that reach the list and makes "one entry per primitive" hold by construction).
//
// Execution model: that of the closest-point query (rtow_pointq.h): persistent waves of 64 consecutive queries, the scene
// image staged in LDS per workgroup, lanes past n (and queries whose max_dist is NaN or negative) entering the walks
// inactive while the wave keeps voting.  A lane writes its k records (48 B each, three 16-byte stores) and its count.

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
#include "rtow_sorted_list.h"

struct NearestParams {
  TraceParams P;                 // the scene (P.sc) and the walks' launch fields: spill, n_lanes, leaf_votes
  const unsigned char *queries;  // [n][48 B], 16-byte aligned
  unsigned char *hits;           // [n][k][48 B], 16-byte aligned
  int32_t *counts;               // [n], or nullptr
  uint32_t n;
  int32_t k;                     // 1 .. 8 (RTOW_MAX_NEAREST, include/rtow.h: the list has eight slots)
  const int32_t *map;            // walk's primitive id -> insertion index
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

// ---- the list sink of the point walks (rtow_point_walks.h) ----
// An empty slot holds max_dist, so the bound — the key of slot k - 1 — is max_dist until k entries are kept.
struct NearestSink {
  static constexpr bool kSerial = true;  // the list takes the registers an interleaved triangle test would
  SortedList8 L;
  int k;
  const int32_t *map;
  double b;  // the key of slot k - 1 (it only shrinks: an insertion only lowers the key of a slot)
  __device__ __forceinline__ void seed(double max_dist) {
    list_clear(L, max_dist);
    b = max_dist;
  }
  __device__ __forceinline__ double bound() const { return b; }
  __device__ __forceinline__ void take(double dist, int id) {
    if (dist <= b) {
      list_insert<true>(L, dist, id, map);
      b = list_bound(L, k);
    }
  }
};

// KERNEL: 1 = BRUTE, 2 = BVH, 4 = BVH4; LDS: the scene image is staged in LDS (stage_scene, rtow_kernel_frame.h)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 ? 1024 : 256) RTOW_CAT(rtow_nearest_, RTOW_SUFFIX)(const NearestParams Q) {
  const TraceParams &P = Q.P;
  const DevScene &sc = P.sc;
  const unsigned lane = lane_id();
  [[maybe_unused]] const uint32_t lane_g = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = Q.k;

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
    NearestSink sink;
    sink.k = k;
    sink.map = Q.map;
    sink.seed(max_dist);
    if constexpr (KERNEL == 4) {
      closest_bvh4<LDS>(im4, sc, P, p, active, lane_g, sink, nnode, nprim);
    } else if constexpr (KERNEL == 2) {
      closest_bvh<LDS>(im, sc, p, time, active, sink, nnode, nprim);
    } else {
      closest_brute(sc, p, time, active, sink, nprim);
    }

    // ---- the records, in list order: each entry's point recomputed by the same formulas ----
    if (in) {
      int32_t count = 0;
      unsigned char *dst = Q.hits + (size_t)i * (size_t)k * kPHitBytes;
      for (int j = 0; j < k; ++j) {
        double dj;
        int idj;
        list_entry(sink.L, j, dj, idj);
        const bool hit = active && idj >= 0;
        double dist = __builtin_huge_val();
        V3d q = {0, 0, 0};
        int32_t prim = -1, kind = -1, mi = -1;
        if (hit) {
          dist = point_record<KERNEL, LDS, NearestSink::kSerial>(im, im4, sc, idj, p, time, q, kind, mi);
          prim = Q.map[idj];
          ++count;
        }
        store_point_hit(dst + (size_t)j * kPHitBytes, dist, q, prim, kind, mi);
      }
      if (Q.counts != nullptr) Q.counts[i] = count;
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<NearestParams> nearest_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_nearest_, RTOW_SUFFIX)<K, L>, NearestParams>(lds_bytes);
}

// kernel: 1 BRUTE, 2 BVH, 4 BVH4.  `lds_bytes` > 0 selects the BVH variant that stages the image in LDS; for 4 the image
// staged whole (b4_half == 0) selects the full-LDS variant, as in the render.  BRUTE uses no LDS.
static KernelVariant<NearestParams> nearest_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return nearest_kernel<1, false>(0);
    case 2: return lds_bytes > 0 ? nearest_kernel<2, true>(lds_bytes) : nearest_kernel<2, false>(0);
    case 4: return b4_full ? nearest_kernel<4, true>(lds_bytes) : nearest_kernel<4, false>(lds_bytes);
    default: return {};
  }
}

int RTOW_CAT(launch_nearest_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                           unsigned lds_bytes, void *stream) {
  NearestParams q;
  q.P = p;
  q.queries = (const unsigned char *)a.in;
  q.hits = (unsigned char *)a.hits;
  q.counts = (int32_t *)a.counts;
  q.n = a.n;
  q.k = a.k;
  q.map = a.map;
  q.counters = a.counters;
  return launch_variant(nearest_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_CAT(nearest_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<NearestParams> v = nearest_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
