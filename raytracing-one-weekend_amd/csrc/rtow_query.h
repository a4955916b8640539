// rtow_query.h — the closest-hit ray query kernel (rtow_intersect / rtow_intersect_device, include/rtow.h), included
// by rtow_query_strict.hip and rtow_query_fast.hip, which differ only in -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller ray, the reference's world hit over [0.001, +inf) (src/render.cpp:33-34,
// BVHNode::hit) with the same walks the trace kernels run — closest_hit_stream / _bvh / _grid / _bvh4 / _reftree,
// included read-only below exactly as rtow_trace_body.h includes them — then the winner's hit record (rtow_hit_record.h,
// shared with the first-k-hits query) rebuilt with the trace kernel's shading expressions: Ray::at, the sphere normal faced
// against the ray, the triangle's un-normalised e1 x e2, the material index from the scene image.  A hit beyond the
// ray's tmax is then reported as a miss (post-filter: the closest hit in [0.001, inf) lies within tmax exactly when
// any hit does; the walks are not seeded with tmax, so nothing is pruned by it).
//
// Execution model (gfx950, wave64): persistent waves.  The grid is what stays resident (occupancy query below, like
// trace_occupancy_*), capped by the number of rays; every wave takes 64 consecutive rays per step and strides over the
// batch.  Lanes past n_rays enter the walks with active = false (the walks vote across the wave: __any / __ballot).
// A lane reads its 64-byte ray with four 16-byte loads (the wave's loads cover one contiguous 4 KiB run) and writes
// its 72-byte hit record with 8-byte stores (the 72-byte stride leaves only every other record 16-byte aligned).
// The scene image is staged in LDS per workgroup once, exactly as the trace kernel stages it for the same strategy.
//
// Walk-order primitive ids -> the caller's insertion order: `map` (built by the host on first use after an upload,
// rtow_queries.cpp).  The STREAM, GRID and REFTREE walks and a device-built BVH return class-major ids; the 4-wide image and
// a host-built mesh BVH hold their triangle records in leaf order and return record slots.  The kind follows from the
// class-major ranges either way (a leaf-ordered image is a triangle mesh).

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
#include "rtow_hit_record.h"

struct QueryParams {
  TraceParams P;               // the scene (P.sc) and the walks' launch fields: spill, n_lanes, leaf_votes, walk_max_open
  const unsigned char *rays;   // [n][64 B], 16-byte aligned
  unsigned char *hits;         // [n][72 B], 8-byte aligned
  uint32_t n;
  const int32_t *map;          // walk's primitive id -> insertion index
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

// -0.0 -> +0.0, every other value unchanged (on the bits: the fast build's -fno-signed-zeros would fold `x + 0.0`).
// The grid walk's DDA takes its step direction from `d >= 0` and its increments from rcp(d) (rtow_trace_grid.h), which
// disagree for a component of -0.0 (rcp(-0) = -inf): such a ray steps the wrong way and misses.  The render's rays
// practically never carry an exact -0.0; a caller's axis-parallel ray (-e_z) often does.  The walk itself is the
// benchmarked kernel's and stays as it is; the query hands it the direction with +0.0 instead.  The hit tests give the
// same t and primitive for either sign of a zero component (it changes only the sign of products that are exactly
// zero), and the hit record is built from the caller's direction.
__device__ __forceinline__ double plus_zero(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return __longlong_as_double((long long)(b == 0x8000000000000000ull ? 0ull : b));
}

// KERNEL: 1 = STREAM, 2 = BVH, 3 = GRID, 4 = BVH4, 5 = REFTREE (strict build only); LDS: the scene image is staged in
// LDS (2 and 3; for 4: the whole image, else the top of its tree — the traversal stack is in LDS either way)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 && KERNEL <= 4 ? 1024 : 256)
    RTOW_CAT(rtow_query_, RTOW_SUFFIX)(const QueryParams Q) {
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
    real rtime = 0, tmax = 0;
    if (active) {
      const vd2 *r = reinterpret_cast<const vd2 *>(Q.rays + (size_t)i * kRayBytes);
      const vd2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];  // {ox, oy} {oz, time} {dx, dy} {dz, tmax}
      ro = {r0.x, r0.y, r1.x};
      rtime = r1.y;
      rd = {r2.x, r2.y, r3.x};
      tmax = r3.y;
    }

    // ---- closest hit over [0.001, inf): the render's walks, run to completion (cap = 0xffffffff) ----
    Closest best;
    best.t = (real)__builtin_huge_val();
    best.prim = -1;
    if constexpr (KERNEL == 4) {
      uint32_t w_cur = kRefNone, w_sa = 0u;
      best = closest_hit_bvh4<LDS, false>(im4, sc, P, ro, rd, rtime, active, lane_g, nnode, nprim, stamps, best, w_cur,
                                          w_sa, 0xffffffffu, P.walk_max_open);
    } else if constexpr (KERNEL == 3) {
      float t_resume = 0.0f;
      // (the fast build's walk returns t in the caller's parameter already: rtow_trace_grid.h, RTOW_UNIT_RAYS)
      const V3 rd_walk = {plus_zero(rd.x), plus_zero(rd.y), plus_zero(rd.z)};
      best = closest_hit_grid<LDS, false>(im, sc, ro, rd_walk, rtime, active, nnode, nprim, stamps, best, t_resume,
                                          0xffffffffu, P.walk_max_open, P.leaf_votes);
    } else if constexpr (KERNEL == 2) {
      best = closest_hit_bvh<LDS, false>(im, sc, ro, rd, rtime, active, nnode, nprim, stamps);
    } else if constexpr (KERNEL == 5) {
#ifndef RTOW_FAST_MATH
      if (active) best = closest_hit_reftree(sc, to_f64(ro), to_f64(rd), (double)rtime, nnode, nprim);
#endif
    } else {
      best = closest_hit_stream(sc, to_f64(ro), to_f64(rd), (double)rtime, active);
    }

    // ---- the hit record of the winner (rtow_hit_record.h) ----
    const bool hit = active && best.prim >= 0 && best.t <= tmax;
    if (active)
      write_hit_record<KERNEL, LDS>(im, im4, sc, Q.map, ro, rd, rtime, hit, best.prim, best.t,
                                    Q.hits + (size_t)i * kHitBytes);
  }

  // statistics: one atomic per wave and counter
  const unsigned long long c0 = wave_sum(nprim), c1 = wave_sum(nnode);
  if (lane == 0) {
    atomicAdd(&Q.counters[0], c0);
    atomicAdd(&Q.counters[1], c1);
  }
}

}  // namespace

#include "rtow_kernel_launch.h"

// kernel: 1 STREAM, 2 BVH, 3 GRID, 4 BVH4, 5 REFTREE (strict build).  `lds_bytes` > 0 selects the variant that stages
// the image in LDS (2, 3); for 4 the image staged whole (b4_half == 0) selects the full-LDS variant, as in the render.
template <int K, bool L>
static KernelVariant<QueryParams> query_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_query_, RTOW_SUFFIX)<K, L>, QueryParams>(lds_bytes);
}

static KernelVariant<QueryParams> query_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return query_kernel<1, false>(lds_bytes);  // (LDS: the tiled triangle loop's per-wave tiles)
    case 2: return lds_bytes > 0 ? query_kernel<2, true>(lds_bytes) : query_kernel<2, false>(0);
    case 3: return lds_bytes > 0 ? query_kernel<3, true>(lds_bytes) : query_kernel<3, false>(0);
    case 4: return b4_full ? query_kernel<4, true>(lds_bytes) : query_kernel<4, false>(lds_bytes);
#ifndef RTOW_FAST_MATH
    case 5: return query_kernel<5, false>(0);
#endif
    default: return {};
  }
}

int RTOW_CAT(launch_query_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                         unsigned lds_bytes, void *stream) {
  const QueryParams q = {p, (const unsigned char *)a.in, (unsigned char *)a.hits, a.n, a.map, a.counters};
  return launch_variant(query_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_CAT(query_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<QueryParams> v = query_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
