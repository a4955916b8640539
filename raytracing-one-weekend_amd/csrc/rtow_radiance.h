// rtow_radiance.h — the radiance query kernel (rtow_radiance / rtow_radiance_device, include/rtow.h), included by
// rtow_radiance_strict.hip and rtow_radiance_fast.hip, which differ only in -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller ray, the sum over its samples of the reference's ray_color (src/render.cpp:112-129)
// — the render's per-sample work without its camera.  The walks are the trace kernels', included read-only below exactly
// as rtow_query.h includes them; the shading surface and the material fetch (rtow_trace_body.h, the `do_scat` block),
// the scatter (scatter_dir) and the sky are restated expression for expression in rtow_scatter.h, which the path-step
// query shares; the unwind of the recursion is here.  The strict build's comparison with the oracle
// (tests/test_gpu_radiance.py) is what proves the copy.
//
// Philox identity: sample j of ray i is (pixel, sample) = (ids[i][0], ids[i][1] + sample_first + j), or (i, sample_first
// + j) without ids; bounce b draws request 1 + b.  Request 0 is the render's camera block and is never drawn here.
//
// Execution model (gfx950, wave64): persistent lanes with refill.  A work item is one ray with all its samples: one
// lane adds them in sample order, so the result cannot depend on the schedule.  One trip of the wave-uniform main loop:
//   1. lanes without an item take one — from the wave's pool, which one atomic on the queue head refills (take_rays:
//      what take_items established in rtow_trace_body.h, without its empty-tile segment);
//   2. lanes starting a sample reload their ray (four 16-byte loads: the ray is not held in registers across a path),
//      lanes whose last segment hit build the hit record and scatter;
//   3. every lane enters the walk, with active = false if it has no ray (the walks vote across the wave), and the walk
//      runs to completion (cap 0xffffffff, as in the queries); then the sky or the end of the path.
// The wave leaves when the queue is empty and none of its lanes holds a path.
//
// Radiance: the strict build records the material index of every bounce in [bounce][lane] words of HBM (a buffer of the
// query's own, max_child_rays x n_lanes) and folds the attenuations from the end of the path when it reaches the sky,
// a1*(a2*(...*sky)), as the strict render does; the fast build multiplies forward in registers.  A path that ends black
// adds nothing.  The add into the running sum is never fused with the multiply that produced the colour (the render's
// rule): a ray with k samples then equals the in-order sum of k one-sample queries bit for bit in both builds.

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
#include "rtow_scatter.h"

struct RadianceParams {
  TraceParams P;               // the scene (P.sc), seed_lo / seed_hi, max_child_rays, stack, n_lanes, spill, the walk fields
  const unsigned char *rays;   // [n][64 B], 16-byte aligned
  const uint32_t *ids;         // [n][2] (pixel, first sample), 8-byte aligned, or NULL: (i, 0)
  double *out;                 // [n][3] sums
  uint32_t n;
  int32_t samples_per_ray;     // >= 1
  uint32_t sample_first;
  unsigned long long *counters;  // [0] primitive tests, [1] node tests, [2] segments, [3] queue head
};

// Rays bought per atomic on the queue head while the queue is long: 64 of 16 samples or more, and as many more of
// shorter ones as keeps a batch near 1024 samples (up to 1024 rays).  The one counter word serves about 90 requests per
// microsecond: 15.36 M one-sample rays took 3.34 ms at 64 per request (240,000 requests) and 1.87 ms at 1024.
constexpr uint32_t kRayBatch = 64, kBatchSamples = 1024;
__device__ __forceinline__ uint32_t ray_batch_max(int32_t samples_per_ray) {
  const uint32_t b = kBatchSamples / (uint32_t)(samples_per_ray < 1 ? 1 : samples_per_ray);
  return b < kRayBatch ? kRayBatch : b;
}

// A wave's share of the ray queue: [next, end) of the queue positions it has bought.  All fields are wave-uniform.
struct RayPool {
  uint32_t next = 0, end = 0;
  unsigned long long seen = 0ull;  // queue head as of this wave's last fetch
};

// Hands one queue position to every lane of `need_mask` (all lanes of the wave call this together); >= n: the queue is
// exhausted.  One atomic buys a batch — batch_max rays while the queue is long, shrinking with what is left to exactly
// what the wave needs now (guided self-scheduling: a wave that hoards rays at the end keeps the launch waiting) — and a
// wave that has seen the end of the queue stops polling the one counter word.
__device__ __forceinline__ unsigned long long take_rays(RayPool &pool, unsigned long long need_mask, unsigned lane,
                                                        uint32_t n_waves, uint32_t n, uint32_t batch_max,
                                                        unsigned long long *head) {
  const uint32_t want = (uint32_t)__popcll(need_mask);
  const uint32_t avail = pool.end - pool.next;
  const uint32_t rank = lanes_below(need_mask);
  unsigned long long mine = (unsigned long long)pool.next + rank;
  if (want > avail) {
    const unsigned long long left = (unsigned long long)n > pool.seen ? (unsigned long long)n - pool.seen : 0ull;
    uint32_t batch = (uint32_t)(left / ((unsigned long long)n_waves * 4ull));
    batch = batch > batch_max ? batch_max : batch;
    batch = batch < want - avail ? want - avail : batch;
    const int leader = __ffsll((long long)need_mask) - 1;
    unsigned long long base = pool.seen;
    if (pool.seen < (unsigned long long)n) {
      if ((int)lane == leader) base = atomicAdd(head, (unsigned long long)batch);
      base = __shfl(base, leader);
    }
    pool.seen = base + batch;
    if (rank >= avail) mine = base + (rank - avail);
    const unsigned long long nn = base + (want - avail), ne = base + batch;
    pool.next = (uint32_t)(nn < (unsigned long long)n ? nn : (unsigned long long)n);
    pool.end = (uint32_t)(ne < (unsigned long long)n ? ne : (unsigned long long)n);
  } else {
    pool.next += want;
  }
  return mine;
}

// KERNEL: 1 = STREAM, 2 = BVH, 3 = GRID, 4 = BVH4, 5 = REFTREE (strict build only); LDS: the scene image is staged in
// LDS (2 and 3; for 4: the whole image, else the top of its tree — the traversal stack is in LDS either way)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 && KERNEL <= 4 ? 1024 : 256)
    RTOW_CAT(rtow_radiance_, RTOW_SUFFIX)(const RadianceParams Q) {
  const TraceParams &P = Q.P;
  const DevScene &sc = P.sc;
  const uint32_t k0 = P.seed_lo, k1 = P.seed_hi;
  const unsigned lane = lane_id();
  [[maybe_unused]] const uint32_t lane_g = blockIdx.x * blockDim.x + threadIdx.x;

  Image<LDS> im;
  [[maybe_unused]] Bvh4Reader<LDS> im4;
  stage_scene<KERNEL, LDS>(sc, im, im4);

  // per-lane state
  bool done = false;          // the queue had nothing left for this lane
  bool need_sample = true;    // no path in flight: the next trip starts a sample (or takes an item)
  bool pending_hit = false;   // the last segment ended in a hit that is scattered at the top of the next trip
  int s_left = 0;             // samples left in the current item
  uint32_t item = 0xffffffffu;  // the ray this lane holds
  V3d acc = {0.0, 0.0, 0.0};  // sum of the item's samples so far
  V3 ro = {0, 0, 0}, rd = {0, 0, 1};
  real rtime = 0;
  int depth = 0;              // remaining child rays
  [[maybe_unused]] int nb = 0;  // bounces recorded on the path stack
#ifdef RTOW_FAST_MATH
  V3 throughput = {1, 1, 1};  // the product of the attenuations so far, multiplied forward
#endif
  Rng g = {0, 0, 0};
  uint32_t nseg = 0, nnode = 0, nprim = 0;
  Closest best;
  best.t = 0;
  best.prim = -1;
  Stamps<false> stamps;
  RayPool pool;
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;

  for (;;) {
    // ---- 1. items: a finished one goes to its result, lanes without one take the next ray of the queue ----
    const bool need_item = !done && need_sample && s_left <= 0;
    const unsigned long long need_mask = __ballot(need_item);
    if (need_mask != 0ull) {
      if (need_item && item != 0xffffffffu) {
        double *dst = Q.out + (size_t)item * 3;
        dst[0] = acc.x;
        dst[1] = acc.y;
        dst[2] = acc.z;
        item = 0xffffffffu;
      }
      const unsigned long long mine =
          take_rays(pool, need_mask, lane, n_waves, Q.n, ray_batch_max(Q.samples_per_ray), &Q.counters[3]);
      if (need_item) {
        if (mine >= (unsigned long long)Q.n) {
          done = true;
        } else {
          item = (uint32_t)mine;
          g.pixel = item;
          g.sample = Q.sample_first;
          if (Q.ids != nullptr) {
            const uint2 id = reinterpret_cast<const uint2 *>(Q.ids)[item];
            g.pixel = id.x;
            g.sample = id.y + Q.sample_first;
          }
          s_left = Q.samples_per_ray;
          acc = {0.0, 0.0, 0.0};
        }
      }
    }
    if (__ballot(!done) == 0ull) break;

    // ---- 2. new rays: the caller's ray for a new sample, the scattered ray of last trip's hit ----
    const bool do_regen = !done && need_sample;
    const bool do_scat = !done && pending_hit;
    if (do_regen) {
      [[maybe_unused]] double tmax;  // (not read: a radiance ray is unbounded)
      load_ray(Q.rays, item, ro, rd, rtime, tmax);
      depth = P.max_child_rays;
      nb = 0;
#ifdef RTOW_FAST_MATH
      throughput = {1, 1, 1};
#endif
      g.r = 1u;  // request 1 + bounce; request 0 is the render's camera block
      need_sample = false;
    }
    if (do_scat) {
      ro = ro + rd * best.t;  // Ray::at: the origin of the scattered ray
      const Surface sf = surface_at<KERNEL, LDS>(im, im4, sc, ro, rd, rtime, best.prim);
      pending_hit = false;
      // (the new direction is written over the old one; an absorbed path — black, src/render.cpp:120 — starts its next
      // sample in the next trip and never reads it)
      V3 dir;
      const bool scattered = scatter_dir(g, k0, k1, sf.kind, sf.fuzz, sf.ir, rd, sf.normal, sf.front, dir);
      rd = dir;
      if (!scattered) {
        need_sample = true;
        --s_left;
        ++g.sample;
      } else {
#ifdef RTOW_FAST_MATH
        throughput = throughput * material_att<KERNEL, LDS>(im, im4, sc, (uint32_t)sf.mi);
#else
        P.stack[(size_t)nb * P.n_lanes + lane_g] = (uint32_t)sf.mi;
#endif
        ++nb;
        --depth;
      }
    }
    const bool tracing = !done && !need_sample;  // has a ray to advance in this trip

    // ---- 3. one ray segment: the render's walks, run to completion (cap = 0xffffffff) ----
    best.t = (real)__builtin_huge_val();
    best.prim = -1;
    if constexpr (KERNEL == 4) {
      uint32_t w_cur = kRefNone, w_sa = 0u;
      best = closest_hit_bvh4<LDS, false>(im4, sc, P, ro, rd, rtime, tracing, lane_g, nnode, nprim, stamps, best, w_cur,
                                          w_sa, 0xffffffffu, P.walk_max_open);
    } else if constexpr (KERNEL == 3) {
      float t_resume = 0.0f;
      // (a caller's axis-parallel ray often carries a -0.0; a scattered ray practically never does, and the select
      // costs less than telling the two apart)
      const V3 rd_walk = {plus_zero(rd.x), plus_zero(rd.y), plus_zero(rd.z)};
      best = closest_hit_grid<LDS, false>(im, sc, ro, rd_walk, rtime, tracing, nnode, nprim, stamps, best, t_resume,
                                          0xffffffffu, P.walk_max_open, P.leaf_votes);
    } else if constexpr (KERNEL == 2) {
      best = closest_hit_bvh<LDS, false>(im, sc, ro, rd, rtime, tracing, nnode, nprim, stamps);
    } else if constexpr (KERNEL == 5) {
#ifndef RTOW_FAST_MATH
      if (tracing) best = closest_hit_reftree(sc, to_f64(ro), to_f64(rd), (double)rtime, nnode, nprim);
#endif
    } else {
      best = closest_hit_stream(sc, to_f64(ro), to_f64(rd), (double)rtime, tracing);
    }

    if (tracing) {
      ++nseg;
      if (best.prim >= 0) {
        if (depth <= 0)
          need_sample = true;  // src/render.cpp:115: black
        else
          pending_hit = true;  // scattered at the top of the next trip
      } else {
        // ---- background + unwind of the recursion (src/render.cpp:119,122-128) ----
        V3 c = sky_color(rd);
#ifdef RTOW_FAST_MATH
        c = throughput * c;
#else
        for (int q = nb - 1; q >= 0; --q)
          c = material_att<KERNEL, LDS>(im, im4, sc, P.stack[(size_t)q * P.n_lanes + lane_g]) * c;
#endif
        {
          // never fused with the multiply that produced `c` (the empty asm hides it from the contraction pass): the
          // colour of a sample is a rounded value whichever call traced it
          V3d cd = to_f64(c);
          asm volatile("" : "+v"(cd.x), "+v"(cd.y), "+v"(cd.z));
          acc = acc + cd;  // += ray_color(...)
        }
        need_sample = true;
      }
      if (need_sample) {
        --s_left;
        ++g.sample;
      }
    }
  }

  flush_counters(Q.counters, nprim, nnode);
  const unsigned long long c2 = wave_sum(nseg);  // the path segments: this kernel's own third counter
  if (lane == 0) atomicAdd(&Q.counters[2], c2);
}

}  // namespace

#include "rtow_kernel_launch.h"

// kernel: 1 STREAM, 2 BVH, 3 GRID, 4 BVH4, 5 REFTREE (strict build): the instantiations of rtow_query.h
template <int K, bool L>
static KernelVariant<RadianceParams> radiance_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_radiance_, RTOW_SUFFIX)<K, L>, RadianceParams>(lds_bytes);
}

static KernelVariant<RadianceParams> radiance_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return radiance_kernel<1, false>(lds_bytes);  // (LDS: the tiled triangle loop's per-wave tiles)
    case 2: return lds_bytes > 0 ? radiance_kernel<2, true>(lds_bytes) : radiance_kernel<2, false>(0);
    case 3: return lds_bytes > 0 ? radiance_kernel<3, true>(lds_bytes) : radiance_kernel<3, false>(0);
    case 4: return b4_full ? radiance_kernel<4, true>(lds_bytes) : radiance_kernel<4, false>(lds_bytes);
#ifndef RTOW_FAST_MATH
    case 5: return radiance_kernel<5, false>(0);
#endif
    default: return {};
  }
}

// p: the scene, seed_lo / seed_hi, max_child_rays, stack (strict), n_lanes, spill and the walk fields
int RTOW_CAT(launch_radiance_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                            unsigned lds_bytes, void *stream) {
  RadianceParams q;
  q.P = p;
  q.rays = (const unsigned char *)a.in;
  q.ids = (const uint32_t *)a.ids;
  q.out = (double *)a.result;
  q.n = a.n;
  q.samples_per_ray = a.samples;
  q.sample_first = a.sample_first;
  q.counters = a.counters;
  return launch_variant(radiance_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h), as query_occupancy_*.
int RTOW_CAT(radiance_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<RadianceParams> v = radiance_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
