// rtow_ambient.h — the ambient (hemisphere visibility) query kernel (rtow_ambient / rtow_ambient_device, include/rtow.h),
// included by rtow_ambient_strict.hip and rtow_ambient_fast.hip, which differ only in -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller surface point, `samples` cosine-weighted directions over the hemisphere of its
// normal, drawn in registers from the point's Philox identity, each asked the occlusion query's question (rtow_any_hit.h:
// is there a hit within [0.001, max_dist]?), and over the samples that are NOT occluded the count, the sum of the
// directions (the bent normal) and the sum of the reference's sky colour.  What a caller of rtow_occluded would do with
// n x samples rays of 64 bytes each, without the rays ever reaching memory (unless the caller asks for them: rays_out).
//
// The arithmetic, in the order it is evaluated (the strict build evaluates it without contraction: tests/ambient_ref.py
// is the same order in numpy).  Point i, sample j:
//   block   philox4x32(counter = (0, sample, pixel, 0), key = seed): REQUEST 0 of (pixel, sample) = (ids[i][0],
//           ids[i][1] + sample_first + j), or (i, sample_first + j) without ids — sums mod 2^32
//   disk    (px, py) = lens_from_block(block)                                      rtow_trace_rng.h: uniform on the disk
//   height  pz = sqrt(max(1 - (px * px + py * py), 0))                             (the clamp: px^2 + py^2 reaches 1 + 1.3e-8)
//   normal  nn = (N.x * N.x + N.y * N.y) + N.z * N.z  (dot);  len = sqrt(nn);  n = (N.x / len, N.y / len, N.z / len)
//           (nn is a normal binary64, 2^-1022 <= nn < inf, or the point is skipped: a subnormal nn has too few bits)
//   frame   s = copysign(1, n.z);  a = -1 / (s + n.z);  c = (n.x * n.y) * a        (Duff et al., "Building an orthonormal
//           t = (1 + ((s * n.x) * n.x) * a,  s * c,  -(s * n.x))                    basis, revisited", JCGT 6(1), 2017)
//           b = (c,  s + ((n.y * n.y) * a),  -n.y)
//   dir     d.k = (t.k * px + b.k * py) + n.k * pz  for k = x, y, z — not renormalised
//   sky     sky_color(d) of rtow_scatter.h
// and, for a sample that is not occluded, in sample order, by the lane that owns the point, from +0.0:
//   open += 1;  bent.k += d.k;  sky.k += sky_color(d).k
// The unit normal and the frame are made again for every sample from the point's record, which is read again for every
// sample (see the sample loop): nothing of the point is carried through a walk.
//
// Execution model (gfx950, wave64): rtow_occlude.h's — persistent waves, every wave takes 64 consecutive points per
// step and strides over the batch; the scene image staged in LDS as the render stages it.  Inside a step the sample
// loop is wave-uniform (`samples` is one number per call): every lane draws its direction, the wave runs ONE any-hit
// walk for its 64 rays (the walks vote across the wave), every lane accumulates.  Lanes past n and skipped points (a
// normal without a direction, an empty interval) enter the walks with active = false and add nothing.  The record leaves
// with four 16-byte stores; with rays_out, every sample's ray leaves with four 16-byte stores (a skipped point's: the
// dead ray of rtow_path_step, all fields 0 and tmax = -1).
// The parallelism of a launch is its POINTS (a lane per point, the samples in sequence: that is what makes the in-order
// sums free): a batch of fewer points than the machine has lanes (262,144 at four waves per SIMD) leaves lanes idle
// whatever its sample count — DESIGN.md §4.18 has the measurement.

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
#include "rtow_bounded_walks.h"
#include "rtow_any_hit.h"
#include "rtow_scatter.h"

struct AmbientParams {
  TraceParams P;                // the scene (P.sc), seed_lo / seed_hi, and the walks' launch fields
  const unsigned char *points;  // [n][64 B] rtow_surface_point_t, 16-byte aligned
  const uint32_t *ids;          // [n][2] (pixel, sample), 8-byte aligned, or NULL: (i, 0)
  unsigned char *out;           // [n][64 B] rtow_ambient_t, 16-byte aligned
  unsigned char *rays_out;      // [n][samples][64 B] rtow_ray_t, 16-byte aligned, or NULL
  uint32_t n;
  uint32_t samples;             // 1 .. 65536
  uint32_t sample_first;
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

// The pointer as a value the compiler cannot trace to its last use: a load through it is made where it is written, in
// every round of the sample loop, and not hoisted out of the loop into registers.  No instruction.
__device__ __forceinline__ const unsigned char *reloaded(const unsigned char *p) {
  asm volatile("" : "+s"(p));
  return p;
}

// Sample direction of the hemisphere of the unit normal `n` for the disk point (px, py): the header's `height`, `frame`
// and `dir` lines, operand for operand.
__device__ __forceinline__ V3 hemisphere_dir(V3 n, real px, real py) {
  const real pz = fast_sqrt(fmax(real(1.0) - (px * px + py * py), real(0.0)));
  const real s = copysign(real(1.0), n.z);
  const real a = fast_div(real(-1.0), s + n.z);
  const real c = (n.x * n.y) * a;
  const real sx = s * n.x;
  const V3 t = {real(1.0) + (sx * n.x) * a, s * c, -sx};
  const V3 b = {c, s + ((n.y * n.y) * a), -n.y};
  return V3{(t.x * px + b.x * py) + n.x * pz, (t.y * px + b.y * py) + n.y * pz, (t.z * px + b.z * py) + n.z * pz};
}

// KERNEL: 1 = STREAM, 2 = BVH, 3 = GRID, 4 = BVH4, 5 = REFTREE (strict build only); LDS: the scene image is staged in
// LDS (stage_scene, rtow_kernel_frame.h) — the instantiations of rtow_occlude.h
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 && KERNEL <= 4 ? 1024 : 256)
    RTOW_CAT(rtow_ambient_, RTOW_SUFFIX)(const AmbientParams Q) {
  const TraceParams &P = Q.P;
  const DevScene &sc = P.sc;
  const unsigned lane = lane_id();
  [[maybe_unused]] const uint32_t lane_g = blockIdx.x * blockDim.x + threadIdx.x;

  Image<LDS> im;
  [[maybe_unused]] Bvh4Reader<LDS> im4;
  stage_scene<KERNEL, LDS>(sc, im, im4);

  uint32_t nnode = 0u, nprim = 0u;
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
  // A wave's step is 64 x samples walks, so a batch is short in steps: the waves are numbered across the workgroups
  // (workgroup-minor), and a batch of fewer steps than waves still spreads over every workgroup of the launch.
  const uint32_t wave = (threadIdx.x >> 6) * gridDim.x + blockIdx.x;
  // wave-uniform loops: every lane of the wave runs every step and every sample (the walks vote across the wave)
  for (uint32_t base = wave * 64u; base < Q.n; base += n_waves * 64u) {
    const uint32_t i = base + lane;
    const bool in = i < Q.n;
    uint32_t pixel = i, sample = Q.sample_first;
    bool active = false;
    if (in) {
      if (Q.ids != nullptr) {
        const uint2 id = reinterpret_cast<const uint2 *>(Q.ids)[i];
        pixel = id.x;
        sample = id.y + Q.sample_first;
      }
      // a skipped point: normal . normal is 0, subnormal, NaN or infinite, or the interval [0.001, max_dist] is empty
      // (NaN included).  A subnormal nn has lost bits to underflow and n = N / sqrt(nn) is no unit vector (a length of
      // 1e-160 gives |d| - 1 = 5e-4); from 2^-1022 on, products that underflow cost nn at most 3 * 2^-1075 / 2^-1022 = 3 u.
      V3 po, nrm;
      real ptime;
      double tmax;
      load_ray(Q.points, i, po, nrm, ptime, tmax);  // (rtow_surface_point_t has the layout of rtow_ray_t)
      const real nn = dot(nrm, nrm);
      active = nn >= real(0x1p-1022) && nn < (real)__builtin_huge_val() && tmax >= RTOW_TMIN;
    }

    // Across a walk the lane keeps its seven sums and the sample's direction, nothing else of the point: the record (64
    // bytes the wave's previous sample left in the cache) is read again for every sample and the unit normal made again
    // from it.  Carried instead, the point, the normal and the frame cost the walks 30 registers and the GRID and BVH4
    // variants, at 1024 lanes per workgroup, their freedom from scratch.
    uint32_t open = 0u;
    V3 bent = {0, 0, 0}, sky = {0, 0, 0};
    for (uint32_t j = 0u; j < Q.samples; ++j) {
      V3 po = {0, 0, 0}, nrm = {0, 0, 1};
      real ptime = 0;
      double tmax = 0.0;
      if (active) load_ray(reloaded(Q.points), i, po, nrm, ptime, tmax);
      const real len = fast_sqrt_pos(dot(nrm, nrm));
      const V3 nh = {fast_div(nrm.x, len), fast_div(nrm.y, len), fast_div(nrm.z, len)};
      uint32_t o0, o1, o2, o3;
      philox4x32(0u, sample + j, pixel, 0u, P.seed_lo, P.seed_hi, o0, o1, o2, o3);
      real px, py;
      lens_from_block(o0, o1, o2, o3, px, py);
      const V3 d = hemisphere_dir(nh, px, py);

      if (in && Q.rays_out != nullptr) {
        vd2 *r = reinterpret_cast<vd2 *>(Q.rays_out + ((size_t)i * Q.samples + j) * kRayBytes);
        const vd2 zero = {0.0, 0.0};
        r[0] = active ? vd2{(double)po.x, (double)po.y} : zero;
        r[1] = active ? vd2{(double)po.z, (double)ptime} : zero;
        r[2] = active ? vd2{(double)d.x, (double)d.y} : zero;
        r[3] = active ? vd2{(double)d.z, tmax} : vd2{0.0, -1.0};
      }

      bool hit = false;
      if constexpr (KERNEL == 4) {
        hit = any_hit_bvh4<LDS>(im4, sc, P, po, d, tmax, active, lane_g, nnode, nprim);
      } else if constexpr (KERNEL == 3) {
        hit = any_hit_grid<LDS>(im, sc, po, d, ptime, tmax, active, nnode, nprim, P.leaf_votes);
      } else if constexpr (KERNEL == 2) {
        hit = any_hit_bvh<LDS>(im, sc, po, d, ptime, tmax, active, nnode, nprim);
      } else if constexpr (KERNEL == 5) {
#ifndef RTOW_FAST_MATH
        // the reference's tree is an exactness mode: its closest hit, compared with max_dist
        if (active) {
          const Closest best = closest_hit_reftree(sc, to_f64(po), to_f64(d), (double)ptime, nnode, nprim);
          hit = best.prim >= 0 && best.t <= tmax;
        }
#endif
      } else {
        hit = any_hit_stream(sc, to_f64(po), to_f64(d), (double)ptime, tmax, active, nprim);
      }

      if (active && !hit) {
        open += 1u;
        bent = bent + d;
        sky = sky + sky_color(d);
      }
    }

    if (in) {
      vd2 *o = reinterpret_cast<vd2 *>(Q.out + (size_t)i * 64u);
      o[0] = vd2{(double)open, (double)bent.x};
      o[1] = vd2{(double)bent.y, (double)bent.z};
      o[2] = vd2{(double)sky.x, (double)sky.y};
      o[3] = vd2{(double)sky.z, active ? (double)Q.samples : 0.0};
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<AmbientParams> ambient_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_ambient_, RTOW_SUFFIX)<K, L>, AmbientParams>(lds_bytes);
}

// kernel: 1 STREAM, 2 BVH, 3 GRID, 4 BVH4, 5 REFTREE (strict build): the instantiations of rtow_occlude.h
static KernelVariant<AmbientParams> ambient_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return ambient_kernel<1, false>(lds_bytes);  // (LDS: the tiled triangle loop's per-wave tiles)
    case 2: return lds_bytes > 0 ? ambient_kernel<2, true>(lds_bytes) : ambient_kernel<2, false>(0);
    case 3: return lds_bytes > 0 ? ambient_kernel<3, true>(lds_bytes) : ambient_kernel<3, false>(0);
    case 4: return b4_full ? ambient_kernel<4, true>(lds_bytes) : ambient_kernel<4, false>(lds_bytes);
#ifndef RTOW_FAST_MATH
    case 5: return ambient_kernel<5, false>(0);
#endif
    default: return {};
  }
}

// p: the scene, seed_lo / seed_hi, n_lanes, spill and the walk fields
int RTOW_CAT(launch_ambient_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                           unsigned lds_bytes, void *stream) {
  AmbientParams q;
  q.P = p;
  q.points = (const unsigned char *)a.in;
  q.ids = (const uint32_t *)a.ids;
  q.out = (unsigned char *)a.result;
  q.rays_out = (unsigned char *)a.rays_out;
  q.n = a.n;
  q.samples = (uint32_t)a.samples;
  q.sample_first = a.sample_first;
  q.counters = a.counters;
  return launch_variant(ambient_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h), as occlude_occupancy_*.
int RTOW_CAT(ambient_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<AmbientParams> v = ambient_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
