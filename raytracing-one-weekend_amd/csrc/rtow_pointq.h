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
// Per-primitive formulas (point_sphere / point_triangle below; written once, in a fixed operation order: the strict build
// compiles them with -ffp-contract=off and tests/point_ref.py mirrors them bit for bit):
//   * sphere: d = p - c, len = sqrt(d.d), dist = |len - R|; the point c + (d * (1 / len)) * R, or c + (R, 0, 0) for
//     len = 0 (p at the centre: no NaN);
//   * triangle: the best of four FEASIBLE candidates, by squared length of the residual p - q: the clamped projections
//     onto the three edges (a + s e1, a + t e2, (a + e1) + u (e2 - e1); a zero-length edge gives its first vertex) and,
//     when n.n > 0 and the Gram-form barycentrics (e2.e2 w.e1 - e1.e2 w.e2, e1.e1 w.e2 - e1.e2 w.e1) lie in [0, n.n],
//     the projection onto the plane.  Every division is guarded (no NaN, no blow-up on a sliver: a degenerate triangle
//     answers as its edges do), and since every candidate lies on the triangle the computed distance is never below the
//     exact one by more than its rounding.
//
// Walks (the trees are the render's images, read with the pieces the ray queries use: Image, Bvh4Reader, bvh4_stack):
//   * BRUTE (1): every primitive, from the class record arrays of DevScene (scalar loads: the loop is wave-uniform);
//   * BVH (2): the threaded binary walk; a box whose lower bound cannot beat the best so far takes `skip`;
//   * BVH4 (4): nearest child first by box distance with the per-lane LDS stack (and spill) of the 4-wide ray walk; an
//     entry carries 11 bits of its box's squared distance, rounded down, and a popped entry beyond the best is dropped.
// Pruning is conservative with respect to the per-primitive distance computed here: the box bound is
// evaluated in binary64 from the binary32 / binary16 planes (decoded c + h * is), compared against
// (best + sigma)^2 with sigma = 2^-40 (|p|_1 + M), M the root box's magnitude — above every rounding of a primitive's
// computed distance for any finite p.  The search radius starts at max_dist (inclusive): a primitive is accepted when its
// distance <= best so far.
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
#define RTOW_PCAT2(a, b) a##b
#define RTOW_PCAT(a, b) RTOW_PCAT2(a, b)

namespace rtow {
namespace {
#include "rtow_trace_math.h"
#include "rtow_trace_hit.h"
#include "rtow_trace_stamps.h"
#include "rtow_trace_bvh.h"
#include "rtow_trace_bvh4.h"
#include "rtow_kernel_frame.h"

constexpr uint32_t kPQueryBytes = 48u, kPHitBytes = 48u;  // rtow_point_query_t, rtow_point_hit_t (include/rtow.h)

struct PointParams {
  TraceParams P;                 // the scene (P.sc) and the walks' launch fields: spill, n_lanes, leaf_votes
  const unsigned char *queries;  // [n][48 B], 16-byte aligned
  unsigned char *hits;           // [n][48 B], 16-byte aligned
  uint32_t n;
  const int32_t *map;            // walk's primitive id -> insertion index
  unsigned long long *counters;  // [0] primitive tests, [1] node tests
};

struct PBest {
  double d;  // distance of the best primitive so far (max_dist before any)
  int prim;  // walk-order id, -1 = none
};

// ---- arithmetic: IEEE in the strict build, the fast build's refined hardware seeds (rtow_trace_math.h) ----
__device__ __forceinline__ double pq_sqrt(double x) {
#ifdef RTOW_FAST_MATH
  return (x > 0.0 && x < __builtin_huge_val()) ? fast_sqrt_pos(x) : x;  // (0 -> 0, +inf -> +inf)
#else
  return sqrt(x);
#endif
}
__device__ __forceinline__ double pq_div(double n, double d) {  // d > 0
#ifdef RTOW_FAST_MATH
  return d < __builtin_huge_val() ? n * fast_rcp(d) : 0.0;
#else
  return n / d;
#endif
}
__device__ __forceinline__ double clamp01(double x) { return fmin(fmax(x, 0.0), 1.0); }

// ---- per-primitive distance and nearest point (Q: also the point) ----
template <bool Q>
__device__ __forceinline__ double point_sphere(V3d p, double cx, double cy, double cz, double r2, V3d &q) {
  const double dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
  const double len = pq_sqrt(dx * dx + dy * dy + dz * dz);
  const double R = pq_sqrt(fabs(r2));
  if constexpr (Q) {
    if (len > 0.0) {
      const double inv = pq_div(1.0, len);
      q = V3d{cx + (dx * inv) * R, cy + (dy * inv) * R, cz + (dz * inv) * R};
    } else {
      q = V3d{cx + R, cy, cz};
    }
  }
  return fabs(len - R);
}

template <bool Q>
__device__ __forceinline__ double point_triangle(V3d p, V3d a, V3d e1, V3d e2, V3d n, V3d &q) {
  const V3d w = p - a;
  const double d1 = dot(w, e1), d2 = dot(w, e2);
  const double ee1 = dot(e1, e1), ee2 = dot(e2, e2), e12 = dot(e1, e2);
  const V3d f = e2 - e1, g = w - e1;
  const double ff = dot(f, f), dg = dot(g, f);
  const double s1 = ee1 > 0.0 ? clamp01(pq_div(d1, ee1)) : 0.0;
  const double t2 = ee2 > 0.0 ? clamp01(pq_div(d2, ee2)) : 0.0;
  const double u3 = ff > 0.0 ? clamp01(pq_div(dg, ff)) : 0.0;
  const V3d r1 = w - e1 * s1, r2 = w - e2 * t2, r3 = g - f * u3;
  double best = dot(r1, r1);
  int which = 0;
  const double b2 = dot(r2, r2), b3 = dot(r3, r3);
  if (b2 < best) best = b2, which = 1;
  if (b3 < best) best = b3, which = 2;
  const double nn = dot(n, n);
  const double sn = ee2 * d1 - e12 * d2, tn = ee1 * d2 - e12 * d1;
  double s = 0.0, t = 0.0;
  if (nn > 0.0 && sn >= 0.0 && tn >= 0.0 && sn + tn <= nn) {
    s = pq_div(sn, nn);
    t = pq_div(tn, nn);
    const V3d r0 = (w - e1 * s) - e2 * t;
    const double b0 = dot(r0, r0);
    if (b0 < best) best = b0, which = 3;
  }
  if constexpr (Q) {
    q = which == 0   ? a + e1 * s1
        : which == 1 ? a + e2 * t2
        : which == 2 ? (a + e1) + f * u3
                     : (a + e1 * s) + e2 * t;
  }
  return pq_sqrt(best);
}

__device__ __forceinline__ void accept(double d, int id, PBest &best) {
  if (d <= best.d) {
    best.d = d;
    best.prim = id;
  }
}

// The squared search radius a box must exceed to be pruned: (best + sigma)^2.
__device__ __forceinline__ double prune_sq(double best, double sigma) {
  const double r = best + sigma;
  return r * r;
}
// Squared distance from p to the box [lo, hi] (binary64; +inf for an empty slot's inverted box).
__device__ __forceinline__ double box_sq(V3d p, double lx, double ly, double lz, double hx, double hy, double hz) {
  const double dx = fmax(fmax(lx - p.x, p.x - hx), 0.0);
  const double dy = fmax(fmax(ly - p.y, p.y - hy), 0.0);
  const double dz = fmax(fmax(lz - p.z, p.z - hz), 0.0);
  return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ double box_mag(double lx, double ly, double lz, double hx, double hy, double hz) {
  return fmax(fabs(lx), fabs(hx)) + fmax(fabs(ly), fabs(hy)) + fmax(fabs(lz), fabs(hz));
}
__device__ __forceinline__ double pq_sigma(V3d p, double mag) {
  return 0x1p-40 * ((fabs(p.x) + fabs(p.y) + fabs(p.z)) + mag);
}

// ---- the primitives of a BVH image (rtow_trace_bvh.h leaf_test: ids or leaf order, class by id range) ----
template <bool LDS, bool Q>
__device__ __forceinline__ double point_image_prim(const Image<LDS> &im, const DevScene &sc, int id, V3d p, double time,
                                                   V3d &q) {
  if (id < sc.n_sph) {
    const uint32_t r = sc.off_sph + 32u * (uint32_t)id;
    const double2 p0 = im.d2(r), p1 = im.d2(r + 16u);
    return point_sphere<Q>(p, p0.x, p0.y, p1.x, p1.y, q);
  } else if (id < sc.n_sph + sc.n_mov) {
    const uint32_t r = sc.off_mov + 64u * (uint32_t)(id - sc.n_sph);
    const double2 p0 = im.d2(r), p1 = im.d2(r + 16u), p2 = im.d2(r + 32u), p3 = im.d2(r + 48u);
    return point_sphere<Q>(p, p0.x + time * p1.y, p0.y + time * p2.x, p1.x + time * p2.y, p3.x, q);
  }
  const uint32_t r = sc.off_tri + 96u * (uint32_t)(id - sc.n_sph - sc.n_mov);
  const double2 q0 = im.d2(r), q1 = im.d2(r + 16u), q2 = im.d2(r + 32u), q3 = im.d2(r + 48u), q4 = im.d2(r + 64u),
                q5 = im.d2(r + 80u);
  return point_triangle<Q>(p, V3d{q0.x, q0.y, q1.x}, V3d{q1.y, q2.x, q2.y}, V3d{q3.x, q3.y, q4.x}, V3d{q4.y, q5.x, q5.y},
                           q);
}

// ---- BRUTE: every primitive from the class record arrays (wave-uniform loop: scalar loads) ----
template <bool Q>
__device__ __forceinline__ double point_class_prim(const DevScene &sc, int id, V3d p, double time, V3d &q) {
  if (id < sc.n_sph) {
    const double *g = sc.sph + 4 * (size_t)id;
    return point_sphere<Q>(p, g[0], g[1], g[2], g[3], q);
  } else if (id < sc.n_sph + sc.n_mov) {
    const double *g = sc.mov + 8 * (size_t)(id - sc.n_sph);
    return point_sphere<Q>(p, g[0] + time * g[3], g[1] + time * g[4], g[2] + time * g[5], g[6], q);
  }
  const double *g = sc.tri + 12 * (size_t)(id - sc.n_sph - sc.n_mov);
  return point_triangle<Q>(p, V3d{g[0], g[1], g[2]}, V3d{g[3], g[4], g[5]}, V3d{g[6], g[7], g[8]},
                           V3d{g[9], g[10], g[11]}, q);
}

__device__ __forceinline__ void closest_brute(const DevScene &sc, V3d p, double time, bool active, PBest &best,
                                              uint32_t &nprim) {
  V3d q;
  {
    cdptr g = (cdptr)sc.sph;
    for (int k = 0; k < sc.n_sph; ++k)
      if (active) accept(point_sphere<false>(p, g[4 * k + 0], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3], q), k, best);
  }
  {
    cdptr g = (cdptr)sc.mov;
    for (int k = 0; k < sc.n_mov; ++k)
      if (active)
        accept(point_sphere<false>(p, g[8 * k + 0] + time * g[8 * k + 3], g[8 * k + 1] + time * g[8 * k + 4],
                                   g[8 * k + 2] + time * g[8 * k + 5], g[8 * k + 6], q),
               sc.n_sph + k, best);
  }
  {
    cdptr g = (cdptr)sc.tri;
    const int base = sc.n_sph + sc.n_mov;
    for (int k = 0; k < sc.n_tri; ++k)
      if (active)
        accept(point_triangle<false>(p, V3d{g[12 * k + 0], g[12 * k + 1], g[12 * k + 2]},
                                     V3d{g[12 * k + 3], g[12 * k + 4], g[12 * k + 5]},
                                     V3d{g[12 * k + 6], g[12 * k + 7], g[12 * k + 8]},
                                     V3d{g[12 * k + 9], g[12 * k + 10], g[12 * k + 11]}, q),
               base + k, best);
  }
  if (active) nprim += (uint32_t)(sc.n_sph + sc.n_mov + sc.n_tri);
}

// ---- BVH: the threaded walk of closest_hit_bvh (rtow_trace_bvh.h) with box distances instead of slabs ----
template <bool LDS>
__device__ __forceinline__ void closest_bvh(const Image<LDS> &im, const DevScene &sc, V3d p, double time, bool active,
                                            PBest &best, uint32_t &nnode, uint32_t &nprim) {
  const uint32_t END = (uint32_t)sc.n_nodes;
  double sigma = 0.0;
  if (active) {  // the root box bounds every primitive: its magnitude scales the slack
    const float4 r0 = im.f4(0u), r1 = im.f4(16u);
    sigma = pq_sigma(p, box_mag(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y));
  }
  double lim = prune_sq(best.d, sigma);
  int last_id = -1;
  uint32_t node = active ? 0u : END;
  uint32_t q0 = 0u, q1 = 0u, q2 = 0u, q3 = 0u;  // queued leaves (0 = empty), oldest first
  V3d q;
  for (;;) {
    if (node < END) {
      const float4 r0 = im.f4(node * 32u), r1 = im.f4(node * 32u + 16u);
      ++nnode;
      const bool near = !(box_sq(p, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y) > lim);
      const uint32_t skip = __float_as_uint(r1.z), leaf = __float_as_uint(r1.w);
      if (near && leaf != 0u) {
        if (q0 == 0u)
          q0 = leaf;
        else if (q1 == 0u)
          q1 = leaf;
        else if (q2 == 0u)
          q2 = leaf;
        else
          q3 = leaf;
      }
      node = (near && leaf == 0u) ? node + 1u : skip;
    }
    const bool any_walking = __any(node < END);
    if (__any(q3 != 0u) || !any_walking) {
      if (q0 != 0u) {
        const uint32_t first = q0 >> 3, count = q0 & 7u;
        for (uint32_t k = 0; k < count; ++k) {
          const int id = sc.leaf_direct ? (int)(first + k) : (int)im.u32(sc.off_ids + 4u * (first + k));
          if (id == last_id) continue;
          last_id = id;
          ++nprim;
          accept(point_image_prim<LDS, false>(im, sc, id, p, time, q), id, best);
        }
      }
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = 0u;
      lim = prune_sq(best.d, sigma);
      if (!any_walking && !__any(q0 != 0u)) break;
    }
  }
}

// ---- BVH4: nearest child first, the per-lane stack of the 4-wide ray walk (rtow_trace_bvh4.h) ----
// The six plane vectors of a node (lo.x hi.x lo.y hi.y lo.z hi.z, four children each) decoded to binary64 world
// coordinates, and its child words.
template <bool FULL>
__device__ __forceinline__ void bvh4_node(const Bvh4Reader<FULL> &im, const DevScene &sc, uint32_t node, double (&pl)[6][4],
                                          vu4 &cw) {
  if constexpr (FULL) {
    const uint32_t nb = node * 128u;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const vf4 v = lds_read<vf4>(nb + 16u * (uint32_t)k);
      pl[k][0] = v.x, pl[k][1] = v.y, pl[k][2] = v.z, pl[k][3] = v.w;
    }
    cw = lds_read<vu4>(nb + 96u);
  } else {
    const uint32_t nb = node * 64u;
    vu4 ax[3];
    if (nb < im.lds_limit) {
#pragma unroll
      for (int k = 0; k < 3; ++k) ax[k] = lds_read<vu4>(nb + 16u * (uint32_t)k);
      cw = lds_read<vu4>(nb + 48u);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) ax[k] = glb_read<vu4>(im.g, nb + 16u * (uint32_t)k);
      cw = glb_read<vu4>(im.g, nb + 48u);
    }
    typedef uint32_t vu2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const vu2 lo = {ax[k].x, ax[k].y}, hi = {ax[k].z, ax[k].w};
      const vh4 hl = __builtin_bit_cast(vh4, lo), hh = __builtin_bit_cast(vh4, hi);
      const double c = sc.b4_c[k], is = (double)sc.b4_is[k];
      pl[2 * k][0] = c + (double)(float)hl.x * is, pl[2 * k][1] = c + (double)(float)hl.y * is;
      pl[2 * k][2] = c + (double)(float)hl.z * is, pl[2 * k][3] = c + (double)(float)hl.w * is;
      pl[2 * k + 1][0] = c + (double)(float)hh.x * is, pl[2 * k + 1][1] = c + (double)(float)hh.y * is;
      pl[2 * k + 1][2] = c + (double)(float)hh.z * is, pl[2 * k + 1][3] = c + (double)(float)hh.w * is;
    }
  }
}

// a stack key: the top 11 bits of a binary32 LOWER bound of a squared distance (or the f32 upper bound of the radius)
__device__ __forceinline__ uint32_t sq_key_down(double b2) { return __float_as_uint((float)b2 * 0.99999988f) >> 20; }
__device__ __forceinline__ uint32_t sq_key_up(double lim) { return __float_as_uint(round_up_f32(lim)) >> 20; }

template <bool FULL>
__device__ __forceinline__ void closest_bvh4(const Bvh4Reader<FULL> &im, const DevScene &sc, const TraceParams &P, V3d p,
                                             bool active, uint32_t lane_g, PBest &best, uint32_t &nnode,
                                             uint32_t &nprim) {
  const Bvh4Stack st = bvh4_stack(sc);
  double sigma = 0.0;
  if (active) {  // the root's children bound every primitive
    double pl[6][4];
    vu4 cw;
    bvh4_node<FULL>(im, sc, 0u, pl, cw);
    const uint32_t c[4] = {cw.x, cw.y, cw.z, cw.w};
    double mag = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c[j] != kRefNone) mag = fmax(mag, box_mag(pl[0][j], pl[2][j], pl[4][j], pl[1][j], pl[3][j], pl[5][j]));
    sigma = pq_sigma(p, mag);
  }
  double lim = prune_sq(best.d, sigma);
  uint32_t klim = sq_key_up(lim);
  uint32_t sa = st.lds;
  uint32_t cur = active ? 0u : kRefNone;  // node 0 = root
  uint32_t q0 = kRefNone, q1 = kRefNone;  // queued leaves, oldest first
  V3d q;
  for (;;) {
    // (1) a leaf reached by the walk waits in the queue for the next leaf phase
    if ((cur & kRefLeaf) != 0u && cur < kRefPop && q1 == kRefNone) {
      if (q0 == kRefNone)
        q0 = cur;
      else
        q1 = cur;
      cur = kRefPop;
    }
    // (2) next entry from the stack; an entry whose box is beyond the search radius is dropped
    if (cur == kRefPop) {
      if (sa == st.lds) {
        cur = kRefNone;
      } else {
        sa -= kBvh4StackStride;
        uint32_t e;
        if (sa < st.end)
          e = lds_read<uint32_t>(sa);
        else
          e = P.spill[(size_t)((sa - st.end) >> kBvh4StackStrideLog2) * P.n_lanes + lane_g];
        cur = (e >> 21) > klim ? kRefPop : (e & 0x1fffffu);
      }
    }
    // (3) one node: four box distances, the nearest child within the radius next, the others to the stack
    if (cur < kRefLeaf) {
      double pl[6][4];
      vu4 cw;
      bvh4_node<FULL>(im, sc, cur, pl, cw);
      ++nnode;
      const uint32_t c[4] = {cw.x, cw.y, cw.z, cw.w};
      double b2[4];
      uint32_t k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        b2[j] = box_sq(p, pl[0][j], pl[2][j], pl[4][j], pl[1][j], pl[3][j], pl[5][j]);
        const bool h = c[j] != kRefNone && !(b2[j] > lim);
        k[j] = h ? ((__float_as_uint((float)b2[j] * 0.99999988f) & ~3u) | (uint32_t)j) : 0xffffffffu;
      }
      const uint32_t kmin = min(min(k[0], k[1]), min(k[2], k[3]));
      const uint32_t s = kmin & 3u;
      cur = kmin == 0xffffffffu ? kRefPop : c[s];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k[j] != 0xffffffffu && (uint32_t)j != s) {
          const uint32_t e = (sq_key_down(b2[j]) << 21) | c[j];
          if (sa < st.end)
            lds_write<uint32_t>(sa, e);
          else
            P.spill[(size_t)((sa - st.end) >> kBvh4StackStrideLog2) * P.n_lanes + lane_g] = e;
          sa += kBvh4StackStride;
        }
      }
    }
    const bool any_walking = __any(cur != kRefNone);
    const unsigned long long m_pending = __ballot(q0 != kRefNone);
    if ((m_pending != 0ull && ((uint32_t)__popcll(m_pending) >= P.leaf_votes || __ballot(bvh4_busy(cur, q1)) == 0ull)) ||
        !any_walking) {
      if (q0 != kRefNone) {
        const uint32_t first = (q0 & (kRefLeaf - 1u)) >> 2, count = (q0 & 3u) + 1u;
        for (uint32_t j = 0; j < count; ++j) {
          const uint32_t r = sc.b4_off_tri + 96u * (first + j);
          const vd2 t0 = im.t2(r), t1 = im.t2(r + 16u), t2 = im.t2(r + 32u), t3 = im.t2(r + 48u), t4 = im.t2(r + 64u),
                    t5 = im.t2(r + 80u);
          ++nprim;
          accept(point_triangle<false>(p, V3d{t0.x, t0.y, t1.x}, V3d{t1.y, t2.x, t2.y}, V3d{t3.x, t3.y, t4.x},
                                       V3d{t4.y, t5.x, t5.y}, q),
                 (int)(first + j), best);
        }
      }
      q0 = q1;
      q1 = kRefNone;
      lim = prune_sq(best.d, sigma);
      klim = sq_key_up(lim);
      if (!any_walking && !__any(q0 != kRefNone)) break;
    }
  }
}

// KERNEL: 1 = BRUTE, 2 = BVH, 4 = BVH4; LDS: the scene image is staged in LDS (stage_scene, rtow_kernel_frame.h)
template <int KERNEL, bool LDS>
__global__ void __launch_bounds__(KERNEL >= 2 ? 1024 : 256) RTOW_PCAT(rtow_pointq_, RTOW_SUFFIX)(const PointParams Q) {
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
    if (in) {
      const vd2 *r = reinterpret_cast<const vd2 *>(Q.queries + (size_t)i * kPQueryBytes);
      const vd2 r0 = r[0], r1 = r[1], r2 = r[2];  // {px, py} {pz, time} {max_dist, pad}
      p = {r0.x, r0.y, r1.x};
      time = r1.y;
      max_dist = r2.x;
    }
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
        const int pid = best.prim;
        if constexpr (KERNEL == 4) {
          const uint32_t r = sc.b4_off_tri + 96u * (uint32_t)pid;
          const vd2 t0 = im4.t2(r), t1 = im4.t2(r + 16u), t2 = im4.t2(r + 32u), t3 = im4.t2(r + 48u),
                    t4 = im4.t2(r + 64u), t5 = im4.t2(r + 80u);
          dist = point_triangle<true>(p, V3d{t0.x, t0.y, t1.x}, V3d{t1.y, t2.x, t2.y}, V3d{t3.x, t3.y, t4.x},
                                      V3d{t4.y, t5.x, t5.y}, q);
          kind = 2;  // (a 4-wide image is a triangle mesh)
          mi = (int)im4.u32(sc.b4_off_pmat + 4u * (uint32_t)pid);
        } else {
          kind = pid < sc.n_sph ? 0 : (pid < sc.n_sph + sc.n_mov ? 1 : 2);
          if constexpr (KERNEL == 2) {
            dist = point_image_prim<LDS, true>(im, sc, pid, p, time, q);
            mi = (int)im.u32(sc.off_pmat + 4u * (uint32_t)pid);
          } else {
            dist = point_class_prim<true>(sc, pid, p, time, q);
            mi = sc.prim_mat[pid];
          }
        }
        prim = Q.map[pid];
      }
      vd2 *h = reinterpret_cast<vd2 *>(Q.hits + (size_t)i * kPHitBytes);
      h[0] = vd2{dist, q.x};
      h[1] = vd2{q.y, q.z};
      reinterpret_cast<int4 *>(h + 2)[0] = make_int4(prim, kind, mi, 0);
    }
  }

  flush_counters(Q.counters, nprim, nnode);
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<PointParams> pointq_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_PCAT(rtow_pointq_, RTOW_SUFFIX)<K, L>, PointParams>(lds_bytes);
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

int RTOW_PCAT(launch_pointq_, RTOW_SUFFIX)(const TraceParams &p, const void *queries, void *hits, uint32_t n,
                                           const int32_t *map, unsigned long long *counters, int kernel, int grid,
                                           int block, unsigned lds_bytes, void *stream) {
  PointParams q;
  q.P = p;
  q.queries = (const unsigned char *)queries;
  q.hits = (unsigned char *)hits;
  q.n = n;
  q.map = map;
  q.counters = counters;
  const KernelVariant<PointParams> v = pointq_variant(kernel, lds_bytes, p.sc.b4_half == 0u);
  return v.fn ? v.launch(q, grid, block, v.lds_bytes, (hipStream_t)stream) : (int)hipErrorInvalidValue;
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_PCAT(pointq_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<PointParams> v = pointq_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
