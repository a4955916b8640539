// rtow_first_hits.h — the first-k-hits (ordered multi-hit) ray query kernel (rtow_first_hits / rtow_first_hits_device,
// include/rtow.h), included by rtow_first_hits_strict.hip and rtow_first_hits_fast.hip, which differ only in
// -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller ray, the set H of primitives whose hit test accepts a t in [0.001, tmax] — one
// entry per primitive, with the root that test picks — ordered ascending by (t, insertion index) and cut at max_hits
// (1 .. 8): max_hits full rtow_hit_t records per ray (the unused ones the miss record) and the count.
//
// The BVH, GRID and BVH4 walks are the tmax-bounded walks of rtow_bounded_walks.h with the list sink below: a hit does
// not end a lane's walk, and the bound is tmax while the lane's list holds fewer than max_hits entries and the t of
// entry max_hits - 1 after that.  Once max_hits entries are kept, a primitive with t above the last of them cannot
// enter; one with t equal to it still can (lower insertion index), and the walks visit every member of a tie at the
// bound (that header: inclusive comparisons, a bound that only shrinks).  Hence the kept list equals "all of H, sorted,
// cut at max_hits", whatever order the walk met the primitives in: bit-determined in the strict build, the same under
// every strategy, builder and schedule.
//
// The list: 8 (t, walk id) pairs per lane in registers, sorted by (t, insertion index); insertion is a fully unrolled
// compare-and-shift over eight named slots (no scratch: see rtow_sorted_list.h).  The insertion index (`map[id]`) is
// read only to break an exact tie in t and at output.  A candidate whose primitive is already in the list is dropped: the grid lists a
// primitive in every cell it overlaps (the one-entry mailbox of leaf_test catches only consecutive repeats).  A primitive
// tested again after it was evicted is rejected by the ordering itself.  Slots at and beyond max_hits may hold entries
// past the cut (the list always sorts 8); they are not reported.
//
// Execution model: that of the other ray queries (rtow_query.h, rtow_occlude.h): persistent waves of 64 consecutive
// rays, the scene image staged in LDS per workgroup as the render stages it, lanes past n_rays (and rays whose tmax is
// below 0.001 or NaN) entering the walks with active = false.  A lane writes its max_hits records (72 B each, 8-byte
// stores) and its count.

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
#include "rtow_kernel_frame.h"
#include "rtow_bounded_walks.h"
#include "rtow_hit_record.h"
#include "rtow_sorted_list.h"

struct FirstHitsParams {
  TraceParams P;               // the scene (P.sc) and the walks' launch fields: spill, n_lanes, leaf_votes
  const unsigned char *rays;   // [n][64 B], 16-byte aligned
  unsigned char *hits;         // [n][max_hits][72 B], 8-byte aligned
  int32_t *counts;             // [n], or nullptr
  uint32_t n;
  int32_t max_hits;            // 1 .. 8 (RTOW_MAX_HITS, include/rtow.h: the list below has eight slots)
  const int32_t *map;          // walk's primitive id -> insertion index
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

// ---- the per-lane list (rtow_sorted_list.h, keyed by t) ----
// An empty slot holds the ray's tmax in the walk's ray parameter; a candidate whose primitive is already kept is dropped
// in a grid cell (DEDUP: the grid lists a primitive in every cell it overlaps; a tree holds every primitive once).
using HitList = SortedList8;
// What a walk does with the outcome of one primitive's test against Closest{bound, -1}.
template <bool DEDUP>
__device__ __forceinline__ void list_take(HitList &L, const Closest &c, const int32_t *map, int max_hits, double &bound) {
  if (c.prim >= 0) {
    list_insert<DEDUP>(L, (double)c.t, c.prim, map);
    bound = list_bound(L, max_hits);
  }
}
__device__ __forceinline__ Closest candidate(double bound) {
  Closest c;
  c.t = (real)bound;
  c.prim = -1;
  return c;
}

// ---- the list sink of the bounded walks (rtow_bounded_walks.h) ----
// One primitive per test: the hit tests overwrite one Closest, and every accepted primitive is a candidate.  The lane is
// never done.  In the fast build's grid walk the list holds distances, and so does the bound (the kernel converts at
// output, as closest_hit_grid does when its walk is complete).
struct FirstHitsSink {
  static constexpr bool kFold = false;  // the slack is multiplied per node, as in the state machine — six registers the list needs
  HitList &L;
  int max_hits;
  const int32_t *map;
  double bound;
  int last_id;  // leaf_test's one-entry mailbox, kept across the grid's cells: a repeat was tested against a bound no smaller
  __device__ __forceinline__ void seed(double tmax) {
    list_clear(L, tmax);
    bound = tmax;
    last_id = -1;
  }
  __device__ __forceinline__ float bound32() const { return round_up_f32(bound); }
  __device__ __forceinline__ bool done() const { return false; }
  // CELL: a grid cell (a primitive is listed in every cell it overlaps: mailbox and DEDUP); else a BVH leaf
  template <bool LDS, bool CELL>
  __device__ __forceinline__ void list(const Image<LDS> &im, const DevScene &sc, const ImgOffsets &off, uint32_t first,
                                       uint32_t count, const RayForms &ray, uint32_t &nprim) {
    for (uint32_t k = 0; k < count; ++k) {
      Closest c = candidate(bound);
      int none = -1;
      leaf_test<LDS, CELL>(im, sc, off, first + k, 1u, ray, c, nprim, CELL ? last_id : none);
      list_take<CELL>(L, c, map, max_hits, bound);
    }
  }
  template <bool LDS>
  __device__ __forceinline__ void large(const Image<LDS> &im, const DevScene &sc, const ImgOffsets &off, uint32_t lf,
                                        uint32_t n_large, const RayForms &ray, uint32_t &nprim) {
    for (uint32_t k = 0; k < n_large; ++k) {
      Closest c = candidate(bound);
      int none = -1;
      leaf_test<LDS, false, 0, true>(im, sc, off, lf + k, 1u, ray, c, nprim, none);
      list_take<true>(L, c, map, max_hits, bound);
    }
  }
  // the leaf's triangles as one-triangle leaves (leaf word: rtow_bvh4.h, [first : 18][count - 1 : 2])
  template <bool FULL>
  __device__ __forceinline__ void leaf4(const Bvh4Reader<FULL> &im, const DevScene &sc, uint32_t leaf, V3d o64, V3d d64,
                                        uint32_t &nprim) {
    const uint32_t first = (leaf & (kRefLeaf - 1u)) >> 2, count = (leaf & 3u) + 1u;
    for (uint32_t k = 0; k < count; ++k) {
      Closest c = candidate(bound);
      bvh4_leaf<FULL>(im, sc, kRefLeaf | ((first + k) << 2), o64, d64, c, nprim);
      list_take<false>(L, c, map, max_hits, bound);
    }
  }
};

template <bool LDS>
__device__ __forceinline__ void first_hits_bvh(const Image<LDS> &im, const DevScene &sc, V3 o, V3 d, real time, double tmax,
                                               bool active, int max_hits, const int32_t *map, HitList &L,
                                               uint32_t &nnode, uint32_t &nprim) {
  FirstHitsSink sink{L, max_hits, map};
  bounded_walk_bvh<LDS>(im, sc, o, d, time, tmax, active, sink, nnode, nprim);
}
template <bool LDS>
__device__ __forceinline__ void first_hits_grid(const Image<LDS> &im, const DevScene &sc, V3 o, V3 d, real time,
                                                double tmax, bool active, int max_hits, const int32_t *map, HitList &L,
                                                uint32_t &nnode, uint32_t &nprim, uint32_t leaf_votes) {
  FirstHitsSink sink{L, max_hits, map};
  bounded_walk_grid<LDS>(im, sc, o, d, time, tmax, active, sink, nnode, nprim, leaf_votes);
}
template <bool FULL>
__device__ __forceinline__ void first_hits_bvh4(const Bvh4Reader<FULL> &im, const DevScene &sc, const TraceParams &P, V3 o,
                                                V3 d, double tmax, bool active, uint32_t lane_g, int max_hits,
                                                const int32_t *map, HitList &L, uint32_t &nnode, uint32_t &nprim) {
  FirstHitsSink sink{L, max_hits, map};
  bounded_walk_bvh4<FULL>(im, sc, P, o, d, tmax, active, lane_g, sink, nnode, nprim);
}

// ---- STREAM: every primitive, in class order, from the class-major arrays (scalar loads: the index is wave-uniform) ----
__device__ __forceinline__ void first_hits_stream(const DevScene &sc, V3d o, V3d d, double time, double tmax, bool active,
                                                  int max_hits, const int32_t *map, HitList &L, uint32_t &nprim) {
  list_clear(L, tmax);
  if (!active) return;
  double bound = tmax;
  const double tmin = RTOW_TMIN;
  const double a = dot(d, d);
  const double inv_a = fast_rcp(a);  // used by the fast build only
  {
    cdptr g = (cdptr)sc.sph;
    for (int k = 0; k < sc.n_sph; ++k) {
      Closest c = candidate(bound);
      sphere_test<double>(o, d, a, inv_a, g[4 * k + 0], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3], k, tmin, c);
      list_take<false>(L, c, map, max_hits, bound);
    }
  }
  {
    cdptr g = (cdptr)sc.mov;
    const int base = sc.n_sph;
    for (int k = 0; k < sc.n_mov; ++k) {
      const double cx = g[8 * k + 0] + time * g[8 * k + 3];
      const double cy = g[8 * k + 1] + time * g[8 * k + 4];
      const double cz = g[8 * k + 2] + time * g[8 * k + 5];
      Closest c = candidate(bound);
      sphere_test<double>(o, d, a, inv_a, cx, cy, cz, g[8 * k + 6], base + k, tmin, c);
      list_take<false>(L, c, map, max_hits, bound);
    }
  }
  {
    cdptr g = (cdptr)sc.tri;  // 12 doubles per record: A, e1, e2, n
    const int base = sc.n_sph + sc.n_mov;
    for (int k = 0; k < sc.n_tri; ++k) {
      Closest c = candidate(bound);
      triangle_test<double>(o, d, V3d{g[12 * k + 0], g[12 * k + 1], g[12 * k + 2]},
                            V3d{g[12 * k + 3], g[12 * k + 4], g[12 * k + 5]},
                            V3d{g[12 * k + 6], g[12 * k + 7], g[12 * k + 8]},
                            V3d{g[12 * k + 9], g[12 * k + 10], g[12 * k + 11]}, base + k, tmin, c);
      list_take<false>(L, c, map, max_hits, bound);
    }
  }
  nprim += (uint32_t)(sc.n_sph + sc.n_mov + sc.n_tri);
}

// KERNEL: 1 = STREAM, 2 = BVH, 3 = GRID, 4 = BVH4; LDS: the scene image is staged in LDS (stage_scene)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 && KERNEL <= 4 ? 1024 : 256)
    RTOW_CAT(rtow_first_hits_, RTOW_SUFFIX)(const FirstHitsParams Q) {
  const TraceParams &P = Q.P;
  const DevScene &sc = P.sc;
  const unsigned lane = lane_id();
  [[maybe_unused]] const uint32_t lane_g = blockIdx.x * blockDim.x + threadIdx.x;
  const int max_hits = Q.max_hits;

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
    V3 wo = {0, 0, 0}, wd = {0, 0, 1};
    real wtime = 0;
    double tmax = 0.0;
    if (in) load_ray(Q.rays, i, wo, wd, wtime, tmax);
    // a ray whose interval [0.001, tmax] is empty (tmax NaN included) hits nothing: it skips the walk
    const bool active = in && tmax >= RTOW_TMIN;

    HitList L;
    if constexpr (KERNEL == 4) {
      first_hits_bvh4<LDS>(im4, sc, P, wo, wd, tmax, active, lane_g, max_hits, Q.map, L, nnode, nprim);
    } else if constexpr (KERNEL == 3) {
      first_hits_grid<LDS>(im, sc, wo, wd, wtime, tmax, active, max_hits, Q.map, L, nnode, nprim, P.leaf_votes);
    } else if constexpr (KERNEL == 2) {
      first_hits_bvh<LDS>(im, sc, wo, wd, wtime, tmax, active, max_hits, Q.map, L, nnode, nprim);
    } else {
      first_hits_stream(sc, to_f64(wo), to_f64(wd), (double)wtime, tmax, active, max_hits, Q.map, L, nprim);
    }

    // ---- the records, in list order ----
    if (in) {
      // (the ray is read again rather than kept across the walk: the walk's registers go to the list)
      V3 ro, rd;
      real rtime;
      [[maybe_unused]] double tmax_again;  // (not read: the walk is over)
      load_ray(Q.rays, i, ro, rd, rtime, tmax_again);
      int32_t count = 0;
      unsigned char *dst = Q.hits + (size_t)i * (size_t)max_hits * kHitBytes;
      for (int j = 0; j < max_hits; ++j) {
        double tj;
        int idj;
        list_entry(L, j, tj, idj);
#ifdef RTOW_UNIT_RAYS
        // distance -> the caller's parameter, as closest_hit_grid returns it (the walk's own 1 / |d|, computed again)
        if constexpr (KERNEL == 3) tj = tj * fast_rsqrt(dot(rd, rd));
#endif
        const bool hit = idj >= 0;
        count += hit ? 1 : 0;
        write_hit_record<KERNEL, LDS>(im, im4, sc, Q.map, ro, rd, rtime, hit, idj, (real)tj, dst + (size_t)j * kHitBytes);
      }
      if (Q.counts != nullptr) Q.counts[i] = count;
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<FirstHitsParams> first_hits_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_first_hits_, RTOW_SUFFIX)<K, L>, FirstHitsParams>(lds_bytes);
}

// kernel: 1 STREAM, 2 BVH, 3 GRID, 4 BVH4.  `lds_bytes` > 0 selects the variant that stages the image in LDS (2, 3); for
// 4 the image staged whole (b4_half == 0) selects the full-LDS variant, as in the render.  STREAM uses no LDS.
static KernelVariant<FirstHitsParams> first_hits_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return first_hits_kernel<1, false>(0);
    case 2: return lds_bytes > 0 ? first_hits_kernel<2, true>(lds_bytes) : first_hits_kernel<2, false>(0);
    case 3: return lds_bytes > 0 ? first_hits_kernel<3, true>(lds_bytes) : first_hits_kernel<3, false>(0);
    case 4: return b4_full ? first_hits_kernel<4, true>(lds_bytes) : first_hits_kernel<4, false>(lds_bytes);
    default: return {};
  }
}

int RTOW_CAT(launch_first_hits_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                              unsigned lds_bytes, void *stream) {
  FirstHitsParams q;
  q.P = p;
  q.rays = (const unsigned char *)a.in;
  q.hits = (unsigned char *)a.hits;
  q.counts = (int32_t *)a.counts;
  q.n = a.n;
  q.max_hits = a.k;
  q.map = a.map;
  q.counters = a.counters;
  return launch_variant(first_hits_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_CAT(first_hits_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<FirstHitsParams> v = first_hits_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
