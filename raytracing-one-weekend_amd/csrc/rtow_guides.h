// rtow_guides.h — the camera stage as a product of its own: the primaries of the resident camera (rtow_camera_rays /
// rtow_camera_rays_device) and the first-hit guide buffers a denoiser takes beside the beauty image (rtow_guides /
// rtow_guides_device, include/rtow.h).  Included by rtow_guides_strict.hip and rtow_guides_fast.hip, which differ only in
// -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: Camera::get_ray (src/render.cpp:158-159, src/common-model.cpp:156-167) fed from request 0 of
// (pixel, sample) — rtow_trace_body.h's camera_ray restated expression for expression (the fast build multiplies by the
// host's 1 / (W - 1) and 1 / (H - 1) where the strict build divides, as the fast render does) — and, for the guides,
// the closest hit of that primary over [0.001, inf) with the trace kernels' walks, included read-only below exactly as
// rtow_query.h includes them, then the hit record and the material fetch of rtow_trace_body.h's `do_scat` block and the
// sky of ray_color's miss branch (src/render.cpp:122-128), restated as rtow_radiance.h restates them.  The strict build's
// comparison with the oracle's ray log (tests/test_gpu_guides.py) is what proves the copy.
//
// Guide values of ONE sample with primary (o, d, time), closest hit (t, primitive) — the operand order is the written one:
//   hit   albedo  a                         the material's attenuation: albedo (Lambertian, Metal), (1, 1, 1) (Dielectric)
//         normal  sphere    N               Hit::normal: normalize(p - c) with p = o + d * t, negated when it does not face
//                                           the ray (normalize(v) = v * (1 / sqrt(v.x*v.x + v.y*v.y + v.z*v.z)))
//                 triangle  (n.x / s, n.y / s, n.z / s),  s = sqrt(n.x*n.x + n.y*n.y + n.z*n.z),  n = e1 x e2 of the record
//                                           (the det >= 1e-6 cut of the hit test guarantees n != 0)
//         depth   t * sqrt(d.x*d.x + d.y*d.y + d.z*d.z)
//         hits    1.0
//   miss  albedo  (1 - w) * (1, 1, 1) + w * (0.5, 0.7, 1.0),  w = 0.5 * (u.y + 1.0),  u = normalize(d)
//         normal, depth, hits: nothing is added
// and a pixel's value is the sum of its samples' values in sample order from +0.0, each add on rounded operands (never
// fused with the multiply that produced the operand: the empty asm statements below).  The strict build evaluates every
// expression without contraction; the fast build contracted, with the fast build's sqrt, rcp and div (rtow_trace_math.h).
// dot(d, d) > 0 for a ray that hit something and s > 0, so no quotient is 0 / 0: no result is NaN for a finite scene.
//
// Execution model of the guides kernel (gfx950, wave64): persistent lanes with refill, as rtow_radiance.h.  A work item
// is one pixel with all its samples: one lane owns the eight sums, so the result cannot depend on the schedule.  Items
// are bought from a queue word with take_rays' scheme.  Queue position -> pixel: 8 x 8 tiles of the rank's rows, tiles
// row-major, 64 consecutive positions per tile (a wave's batch is then a compact bundle of primaries that walk nearly
// the same nodes); positions of a border tile that fall outside the rows are taken and dropped.  One trip of the
// wave-uniform loop: lanes without an item take one (a finished item is written first: four 16-byte stores), every lane
// with an item generates its next primary, every lane enters the walk (active = false without a primary: the walks vote
// across the wave) and the walk runs to completion; then the fold.  No per-bounce buffer and no scratch outside REFTREE's stack.
//
// The camera-ray kernel: one lane per (pixel, sample), a stride loop; one Philox block, the camera block through
// wave-uniform loads, four 16-byte stores and one 8-byte id store (skipped for a NULL ids).  It reads nothing of the
// scene but the camera, so it runs after a lean upload too.

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

constexpr uint32_t kGuideBytes = 64u;  // rtow_guide_t, include/rtow.h

struct GuideParams {
  TraceParams P;      // the scene (P.sc), cam, W, H, inv_wm1 / inv_hm1, rank / nranks / tile_rows, local_rows, seed_lo /
                      // seed_hi, n_lanes, spill and the walk fields
  unsigned char *out; // guides: [local_rows * W][64 B]; camera rays: [n][64 B]; 16-byte aligned
  uint32_t *ids;      // camera rays: [n][2] (pixel, sample), 8-byte aligned, or NULL
  uint32_t n;         // guides: queue positions (tiles * 64); camera rays: local_rows * W * samples
  uint32_t sample_first;
  int32_t samples;    // samples per pixel of this call, >= 1
  uint32_t tiles_x;   // guides: 8 x 8 tiles per tile row = ceil(W / 8)
  unsigned long long *counters;  // [0] primitive tests, [1] node tests, [3] queue head
};

// -0.0 -> +0.0, every other value unchanged (rtow_query.h: the grid walk's DDA takes its step direction from `d >= 0`
// and its increments from rcp(d), which disagree for -0.0; the hit tests give the same t and primitive either way).
__device__ __forceinline__ double plus_zero(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return __longlong_as_double((long long)(b == 0x8000000000000000ull ? 0ull : b));
}

// local row of this rank -> global row: the rank's q-th strip is global strip q * nranks + rank (decode_item, rtow_trace_body.h)
__device__ __forceinline__ uint32_t global_row(const TraceParams &P, uint32_t lr) {
  const uint32_t q = lr / (uint32_t)P.tile_rows;
  return (q * (uint32_t)P.nranks + (uint32_t)P.rank) * (uint32_t)P.tile_rows + (lr - q * (uint32_t)P.tile_rows);
}

// Camera::get_ray for sample (g.pixel, g.sample) of pixel (column j, global row gi): rtow_trace_body.h's camera_ray (the
// strict build) and its new-ray stage's reciprocals (the fast build), restated.  All from the sample's request 0.
__device__ __forceinline__ void camera_ray(const TraceParams &P, const Rng &g, uint32_t k0, uint32_t k1, uint32_t j,
                                           uint32_t gi, V3 &ro, V3 &rd, real &rtime) {
  const int from_top_i = P.H - (int)gi - 1;
  uint32_t o0, o1, o2, o3;
  philox4x32(0u, g.sample, g.pixel, 0u, k0, k1, o0, o1, o2, o3);
  real ju, jv, jt, px, py;
  jitter_from_block(o0, o1, o2, ju, jv, jt);
  lens_from_block(o0, o1, o2, o3, px, py);
#ifdef RTOW_FAST_MATH
  const real u = ((real)(int)j + ju) * (real)P.inv_wm1;
  const real v = ((real)from_top_i + jv) * (real)P.inv_hm1;
#else
  const real u = fast_div((real)(int)j + ju, (real)(P.W - 1));
  const real v = fast_div((real)from_top_i + jv, (real)(P.H - 1));
#endif
  // camera block: wave-uniform scalar loads (origin u v horizontal vertical llc | lens t0 t1)
  cdptr cm = (cdptr)(const double *)P.cam;
  const real lens = cm[18], ct0 = cm[19], ct1 = cm[20];
  const real rdx = lens * px, rdy = lens * py;
  const V3 offset = V3{cm[3], cm[4], cm[5]} * rdx + V3{cm[6], cm[7], cm[8]} * rdy;
  const V3 from = V3{cm[0], cm[1], cm[2]} + offset;
  rd = V3{cm[15], cm[16], cm[17]} + u * V3{cm[9], cm[10], cm[11]} + v * V3{cm[12], cm[13], cm[14]} - from;
  ro = from;
  rtime = jt * (ct1 - ct0) + ct0;
}

// ---- the primaries ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) RTOW_CAT(rtow_camera_rays_, RTOW_SUFFIX)(const GuideParams Q) {
  const TraceParams &P = Q.P;
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t S = (uint32_t)Q.samples, W = (uint32_t)P.W;
  // (64-bit loop index: n <= 2^31 - 64 and the stride may carry it past 2^32)
  for (unsigned long long i64 = blockIdx.x * blockDim.x + threadIdx.x; i64 < (unsigned long long)Q.n; i64 += stride) {
    const uint32_t i = (uint32_t)i64;
    const uint32_t lp = i / S, s = i - lp * S;  // local pixel (row-major over the rank's rows), sample of the call
    const uint32_t lr = lp / W, j = lp - lr * W;
    const uint32_t gi = global_row(P, lr);
    Rng g = {gi * W + j, Q.sample_first + s, 0u};
    V3 ro, rd;
    real rtime;
    camera_ray(P, g, P.seed_lo, P.seed_hi, j, gi, ro, rd, rtime);
    vd2 *r = reinterpret_cast<vd2 *>(Q.out + (size_t)i * kRayBytes);
    r[0] = vd2{ro.x, ro.y};
    r[1] = vd2{ro.z, rtime};
    r[2] = vd2{rd.x, rd.y};
    r[3] = vd2{rd.z, __builtin_huge_val()};
    if (Q.ids != nullptr) reinterpret_cast<uint2 *>(Q.ids)[i] = make_uint2(g.pixel, g.sample);
  }
}

// ---- the guides ---------------------------------------------------------------------------------------------------------
// Queue positions bought per atomic while the queue is long: whole tiles, and as many as keeps a batch near 1024 samples
constexpr uint32_t kPosBatch = 64u, kBatchSamples = 1024u;
__device__ __forceinline__ uint32_t pos_batch_max(int32_t samples) {
  const uint32_t b = (kBatchSamples / (uint32_t)(samples < 1 ? 1 : samples)) & ~63u;
  return b < kPosBatch ? kPosBatch : b;
}

// A wave's share of the queue and how it is refilled: rtow_radiance.h's RayPool / take_rays, restated.
struct PosPool {
  uint32_t next = 0, end = 0;
  unsigned long long seen = 0ull;  // queue head as of this wave's last fetch
};
__device__ __forceinline__ unsigned long long take_positions(PosPool &pool, unsigned long long need_mask, unsigned lane,
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

// the add of one guide value: on a rounded operand (the empty asm hides the producing multiply from the contraction pass)
__device__ __forceinline__ void add_rounded(double &acc, double v) {
  asm volatile("" : "+v"(v));
  acc = acc + v;
}

// KERNEL: 1 = STREAM, 2 = BVH, 3 = GRID, 4 = BVH4, 5 = REFTREE (strict build only); LDS: the scene image is staged in
// LDS (2 and 3; for 4: the whole image, else the top of its tree — the traversal stack is in LDS either way)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 && KERNEL <= 4 ? 1024 : 256)
    RTOW_CAT(rtow_guides_, RTOW_SUFFIX)(const GuideParams Q) {
  const TraceParams &P = Q.P;
  const DevScene &sc = P.sc;
  const uint32_t k0 = P.seed_lo, k1 = P.seed_hi;
  const unsigned lane = lane_id();
  [[maybe_unused]] const uint32_t lane_g = blockIdx.x * blockDim.x + threadIdx.x;

  Image<LDS> im;
  [[maybe_unused]] Bvh4Reader<LDS> im4;
  stage_scene<KERNEL, LDS>(sc, im, im4);

  // per-lane state
  bool done = false;            // the queue had nothing left for this lane
  int s_left = 0;               // samples left in the current item
  uint32_t item = 0xffffffffu;  // the local pixel (row-major over the rank's rows) this lane holds
  uint32_t pj = 0u, pgi = 0u;   // its column and global row
  V3d a_alb = {0.0, 0.0, 0.0}, a_nrm = {0.0, 0.0, 0.0};
  double a_depth = 0.0, a_hits = 0.0;
  Rng g = {0, 0, 0};
  uint32_t nnode = 0, nprim = 0;
  Stamps<false> stamps;
  PosPool pool;
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;

  for (;;) {
    // ---- 1. items: a finished one goes to its result, lanes without one take the next position of the queue ----
    const bool need_item = !done && s_left <= 0;
    const unsigned long long need_mask = __ballot(need_item);
    if (need_mask != 0ull) {
      if (need_item && item != 0xffffffffu) {
        vd2 *dst = reinterpret_cast<vd2 *>(Q.out + (size_t)item * kGuideBytes);
        dst[0] = vd2{a_alb.x, a_alb.y};
        dst[1] = vd2{a_alb.z, a_nrm.x};
        dst[2] = vd2{a_nrm.y, a_nrm.z};
        dst[3] = vd2{a_depth, a_hits};
        item = 0xffffffffu;
      }
      const unsigned long long mine =
          take_positions(pool, need_mask, lane, n_waves, Q.n, pos_batch_max(Q.samples), &Q.counters[3]);
      if (need_item) {
        if (mine >= (unsigned long long)Q.n) {
          done = true;
        } else {
          // position -> tile (row-major) and pixel inside it; a border tile's positions outside the rows are dropped
          const uint32_t pos = (uint32_t)mine, tile = pos >> 6, w = pos & 63u;
          const uint32_t ty = tile / Q.tiles_x, tx = tile - ty * Q.tiles_x;
          const uint32_t lr = ty * 8u + (w >> 3), j = tx * 8u + (w & 7u);
          if (lr < (uint32_t)P.local_rows && j < (uint32_t)P.W) {
            item = lr * (uint32_t)P.W + j;
            pj = j;
            pgi = global_row(P, lr);
            g.pixel = pgi * (uint32_t)P.W + j;
            g.sample = Q.sample_first;
            s_left = Q.samples;
            a_alb = {0.0, 0.0, 0.0};
            a_nrm = {0.0, 0.0, 0.0};
            a_depth = 0.0;
            a_hits = 0.0;
          }
        }
      }
    }
    if (__ballot(!done) == 0ull) break;

    // ---- 2. the next primary of every lane that holds a pixel ----
    const bool tracing = !done && s_left > 0;
    V3 ro = {0, 0, 0}, rd = {0, 0, 1};
    real rtime = 0;
    if (tracing) camera_ray(P, g, k0, k1, pj, pgi, ro, rd, rtime);

    // ---- 3. closest hit over [0.001, inf): the render's walks, run to completion (cap = 0xffffffff) ----
    Closest best;
    best.t = (real)__builtin_huge_val();
    best.prim = -1;
    if constexpr (KERNEL == 4) {
      uint32_t w_cur = kRefNone, w_sa = 0u;
      best = closest_hit_bvh4<LDS, false>(im4, sc, P, ro, rd, rtime, tracing, lane_g, nnode, nprim, stamps, best, w_cur,
                                          w_sa, 0xffffffffu, P.walk_max_open);
    } else if constexpr (KERNEL == 3) {
      float t_resume = 0.0f;
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

    // ---- 4. the fold ----
    if (tracing) {
      if (best.prim >= 0) {
        // the Hit of the winner (src/common-model.cpp:83-90, :121) and its material: rtow_trace_body.h, `do_scat`
        V3 normal, att;
        const V3 p = ro + rd * best.t;  // Ray::at
        const int pid = best.prim;
        bool tri = false;
        if constexpr (KERNEL == 4) {
          const uint32_t r = sc.b4_off_tri + 96u * (uint32_t)pid;
          const vd2 q4 = im4.t2(r + 64u), q5 = im4.t2(r + 80u);
          normal = {(real)q4.y, (real)q5.x, (real)q5.y};
          tri = true;
          const int mi = (int)im4.u32(sc.b4_off_pmat + 4u * (uint32_t)pid);
          const uint32_t mr = sc.b4_off_mats + 48u * (uint32_t)mi;
          const vd2 m0 = im4.d2(mr), m1 = im4.d2(mr + 16u);  // {att.x, att.y}, {att.z, fuzz}
          att = V3{(real)m0.x, (real)m0.y, (real)m1.x};
        } else if constexpr (KERNEL == 2 || KERNEL == 3) {
          const uint32_t o_sph = KERNEL == 3 ? sc.g_off_sph : sc.off_sph;
          const uint32_t o_mov = KERNEL == 3 ? sc.g_off_mov : sc.off_mov;
          const uint32_t o_tri = KERNEL == 3 ? sc.g_off_tri : sc.off_tri;
          const uint32_t o_pmat = KERNEL == 3 ? sc.g_off_pmat : sc.off_pmat;
          const uint32_t o_mats = KERNEL == 3 ? sc.g_off_mats : sc.off_mats;
          if (pid < sc.n_sph + sc.n_mov) {
            V3 center;
            bool inward;  // negative radius: only the sign of the signed r*r is used here
            if (pid < sc.n_sph) {
              const double2 p0 = im.d2(o_sph + 32u * (uint32_t)pid), p1 = im.d2(o_sph + 32u * (uint32_t)pid + 16u);
              center = {(real)p0.x, (real)p0.y, (real)p1.x};
              inward = p1.y < 0.0;
            } else {
              const uint32_t r = o_mov + 64u * (uint32_t)(pid - sc.n_sph);
              const double2 p0 = im.d2(r), p1 = im.d2(r + 16u), p2 = im.d2(r + 32u), p3 = im.d2(r + 48u);
              center = {p0.x + rtime * p1.y, p0.y + rtime * p2.x, p1.x + rtime * p2.y};
              inward = p3.x < 0.0;
            }
            normal = normalize(p - center);
            const bool front = (dot(rd, normal) < real(0.0)) ^ inward;
            normal = front ? normal : -normal;
          } else {
            const uint32_t r = o_tri + 96u * (uint32_t)(pid - sc.n_sph - sc.n_mov);
            const double2 q4 = im.d2(r + 64u), q5 = im.d2(r + 80u);
            normal = {q4.y, q5.x, q5.y};
            tri = true;
          }
          const int mi = (int)im.u32(o_pmat + 4u * (uint32_t)pid);
          const uint32_t mr = o_mats + 48u * (uint32_t)mi;
          const double2 m0 = im.d2(mr), m1 = im.d2(mr + 16u);  // {att.x, att.y}, {att.z, fuzz}
          att = V3{(real)m0.x, (real)m0.y, (real)m1.x};
        } else {
          if (pid < sc.n_sph + sc.n_mov) {
            V3 center;
            bool inward;
            if (pid < sc.n_sph) {
              const double *q = sc.sph + 4 * (size_t)pid;
              center = {(real)q[0], (real)q[1], (real)q[2]};
              inward = sc.sph_r[pid] < 0.0;
            } else {
              const double *q = sc.mov + 8 * (size_t)(pid - sc.n_sph);
              center = {q[0] + rtime * q[3], q[1] + rtime * q[4], q[2] + rtime * q[5]};
              inward = q[7] < 0.0;
            }
            normal = normalize(p - center);
            const bool front = (dot(rd, normal) < real(0.0)) ^ inward;
            normal = front ? normal : -normal;
          } else {
            const double *q = sc.tri + 12 * (size_t)(pid - sc.n_sph - sc.n_mov);
            normal = {(real)q[9], (real)q[10], (real)q[11]};
            tri = true;
          }
          const DevMaterial *m = sc.mats + sc.prim_mat[pid];
          att = V3{(real)m->att[0], (real)m->att[1], (real)m->att[2]};
        }
        if (tri) {  // n / sqrt(n . n): one square root, three divisions
          const real s = fast_sqrt_pos(dot(normal, normal));
          normal = {fast_div(normal.x, s), fast_div(normal.y, s), fast_div(normal.z, s)};
        }
        const real dist = best.t * fast_sqrt(dot(rd, rd));
        add_rounded(a_alb.x, (double)att.x);
        add_rounded(a_alb.y, (double)att.y);
        add_rounded(a_alb.z, (double)att.z);
        add_rounded(a_nrm.x, (double)normal.x);
        add_rounded(a_nrm.y, (double)normal.y);
        add_rounded(a_nrm.z, (double)normal.z);
        add_rounded(a_depth, (double)dist);
        a_hits = a_hits + 1.0;
      } else {
        // background (src/render.cpp:122-128): rtow_radiance.h's sky
        const V3 unit = normalize(rd);
        const real t = real(0.5) * (unit.y + real(+1.0));
        const V3 c = (real(1.0) - t) * V3{1, 1, 1} + t * V3{real(0.5), real(0.7), real(1.0)};
        add_rounded(a_alb.x, (double)c.x);
        add_rounded(a_alb.y, (double)c.y);
        add_rounded(a_alb.z, (double)c.z);
      }
      --s_left;
      ++g.sample;
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

// kernel: 1 STREAM, 2 BVH, 3 GRID, 4 BVH4, 5 REFTREE (strict build): the instantiations of rtow_query.h
template <int K, bool L>
static KernelVariant<GuideParams> guides_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_CAT(rtow_guides_, RTOW_SUFFIX)<K, L>, GuideParams>(lds_bytes);
}

static KernelVariant<GuideParams> guides_variant(int kernel, unsigned lds_bytes, bool b4_full) {
  switch (kernel) {
    case 1: return guides_kernel<1, false>(lds_bytes);  // (LDS: the tiled triangle loop's per-wave tiles)
    case 2: return lds_bytes > 0 ? guides_kernel<2, true>(lds_bytes) : guides_kernel<2, false>(0);
    case 3: return lds_bytes > 0 ? guides_kernel<3, true>(lds_bytes) : guides_kernel<3, false>(0);
    case 4: return b4_full ? guides_kernel<4, true>(lds_bytes) : guides_kernel<4, false>(lds_bytes);
#ifndef RTOW_FAST_MATH
    case 5: return guides_kernel<5, false>(0);
#endif
    default: return {};
  }
}

// a.result: the guide records or the rays; a.ids: the camera rays' optional sample ids
static GuideParams guide_params(const TraceParams &p, const QueryArgs &a, void *ids, unsigned long long *counters) {
  GuideParams q;
  q.P = p;
  q.out = (unsigned char *)a.result;
  q.ids = (uint32_t *)ids;
  q.n = a.n;
  q.sample_first = a.sample_first;
  q.samples = a.samples;
  q.tiles_x = ((uint32_t)p.W + 7u) / 8u;
  q.counters = counters;
  return q;
}

// p: the scene, the camera, W / H and their reciprocals, the rank's rows, seed_lo / seed_hi and the walk fields;
// n: queue positions = tiles of the rank's rows * 64
int RTOW_CAT(launch_guides_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                          unsigned lds_bytes, void *stream) {
  const GuideParams q = guide_params(p, a, nullptr, a.counters);
  return launch_variant(guides_variant(kernel, lds_bytes, p.sc.b4_half == 0u), q, grid, block, stream);
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h), as query_occupancy_*.
int RTOW_CAT(guides_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<GuideParams> v = guides_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

// p: the camera, W / H and their reciprocals, the rank's rows, seed_lo / seed_hi; n = local_rows * W * samples rays
// (one kernel that walks nothing: `kernel`, `lds_bytes` and the counters of the common signature are not used)
int RTOW_CAT(launch_camera_rays_, RTOW_SUFFIX)(const TraceParams &p, const QueryArgs &a, int kernel, int grid, int block,
                                               unsigned lds_bytes, void *stream) {
  const GuideParams q = guide_params(p, a, a.ids, nullptr);
  return launch_kernel<RTOW_CAT(rtow_camera_rays_, RTOW_SUFFIX), GuideParams>(q, grid, block, 0u, (hipStream_t)stream);
}

}  // namespace rtow
