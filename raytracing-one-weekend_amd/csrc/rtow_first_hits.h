// rtow_first_hits.h — the first-k-hits (ordered multi-hit) ray query kernel (rtow_first_hits / rtow_first_hits_device,
// include/rtow.h), included by rtow_first_hits_strict.hip and rtow_first_hits_fast.hip, which differ only in
// -ffp-contract and in RTOW_SUFFIX.
//
// What it computes: for every caller ray, the set H of primitives whose hit test accepts a t in [0.001, tmax] — one
// entry per primitive, with the root that test picks — ordered ascending by (t, insertion index) and cut at max_hits
// (1 .. 8): max_hits full rtow_hit_t records per ray (the unused ones the miss record) and the count.
//
// The walks below are the any-hit walks of rtow_occlude.h (the render's walks seeded with tmax, without suspend /
// resume) with two changes: a hit does not end a lane's walk, and the bound the boxes, cells and primitive tests cull
// against is tmax while the lane's list holds fewer than max_hits entries and the t of entry max_hits - 1 after that.
// The pieces they are built from (Image, the ray forms, leaf_test, the hit tests, the 4-wide step, leaf and stack) are
// the render's, included read-only.
//
// Why the shrinking bound is exact: a primitive's test with upper bound b accepts exactly when its unbounded test
// returns a t <= b (rtow_occlude.h: sphere_resolve picks its root by tmin alone, a triangle has one t), with the same
// bits.  Once max_hits entries are kept, a primitive with t above the last of them cannot enter; one with t equal to it
// still can (lower insertion index), and the bound is inclusive everywhere — the box and cell intervals are conservative
// f32 supersets compared with <=, the primitive tests accept t <= bound — so every member of a tie at the bound is
// visited.  The bound only shrinks, so a subtree, cell or primitive once rejected stays rejected.  Hence the kept list
// equals "all of H, sorted, cut at max_hits", whatever order the walk met the primitives in: bit-determined in the
// strict build, the same under every strategy, builder and schedule.
//
// The list: 8 (t, walk id) pairs per lane in registers, sorted by (t, insertion index); insertion is a fully unrolled
// compare-and-shift over eight named slots (no scratch: see HitList).  The insertion index (`map[id]`) is read only to break an
// exact tie in t and at output.  A candidate whose primitive is already in the list is dropped: the grid lists a
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
#define RTOW_FCAT2(a, b) a##b
#define RTOW_FCAT(a, b) RTOW_FCAT2(a, b)

namespace rtow {
namespace {
#include "rtow_trace_math.h"
#include "rtow_trace_hit.h"
#include "rtow_trace_stamps.h"
#include "rtow_trace_bvh.h"
#include "rtow_trace_grid.h"
#include "rtow_trace_bvh4.h"
#include "rtow_kernel_frame.h"
#include "rtow_hit_record.h"

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

// ---- the per-lane list ----
// Eight named slots, not arrays: the compiler folds a chain of selects over array elements into one dynamically indexed
// load, which sends the whole list to scratch; named members are registers from the first pass on.
#define RTOW_FH_SLOTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
struct HitList {
  double t0, t1, t2, t3, t4, t5, t6, t7;  // ascending by (t, map[id]); an empty slot holds the ray's tmax (no kept t is above it)
  int i0, i1, i2, i3, i4, i5, i6, i7;     // walk ids; -1 = empty slot (empty slots are a suffix)
};
// `tmax` in the walk's ray parameter
__device__ __forceinline__ void list_clear(HitList &L, double tmax) {
#define RTOW_FH_X(j) L.t##j = tmax, L.i##j = -1;
  RTOW_FH_SLOTS(RTOW_FH_X)
#undef RTOW_FH_X
}
// The culling bound: the t of slot max_hits - 1 — tmax while fewer than max_hits entries are kept (an empty slot holds
// it, so the walk keeps no copy of tmax), then the t of the last entry that will be reported.
__device__ __forceinline__ double list_bound(const HitList &L, int max_hits) {
  double b = L.t7;
#define RTOW_FH_X(j) if (max_hits == j + 1) b = L.t##j;
  RTOW_FH_SLOTS(RTOW_FH_X)
#undef RTOW_FH_X
  return b;
}
// Entry j of the list (wave-uniform j).  (The empty asm keeps the selects a chain: left alone, the compiler parks the
// eight t in scratch and loads slot j from there.)
__device__ __forceinline__ void list_entry(const HitList &L, int j, double &t, int &id) {
  t = L.t7, id = L.i7;
#define RTOW_FH_X(k)                  \
  if (j == k) t = L.t##k, id = L.i##k; \
  asm volatile("" : "+v"(t), "+v"(id));
  RTOW_FH_SLOTS(RTOW_FH_X)
#undef RTOW_FH_X
}
// Inserts (t, id) in (t, map[id]) order by compare-and-shift over the eight slots; the entry pushed out of slot 7, or
// the candidate itself, is dropped.
// DEDUP: drop a candidate whose primitive is already kept (the grid; a tree holds every primitive once).
template <bool DEDUP>
__device__ __forceinline__ void list_insert(HitList &L, double t, int id, const int32_t *map) {
  if constexpr (DEDUP) {
    bool dup = false;
#define RTOW_FH_X(j) dup = dup || L.i##j == id;
    RTOW_FH_SLOTS(RTOW_FH_X)
#undef RTOW_FH_X
    if (dup) return;
  }
  // b<j>: entry j stays in front of the candidate (a prefix of the list, which is sorted); an exact tie in t is decided
  // by the insertion index
#define RTOW_FH_X(j)                                              \
  bool b##j = L.t##j < t;                                         \
  if (L.t##j == t && L.i##j >= 0) b##j = map[L.i##j] < map[id];
  RTOW_FH_SLOTS(RTOW_FH_X)
#undef RTOW_FH_X
#define RTOW_FH_SHIFT(j, jm)            \
  if (!b##j) {                          \
    L.t##j = b##jm ? t : L.t##jm;       \
    L.i##j = b##jm ? id : L.i##jm;      \
  }
  RTOW_FH_SHIFT(7, 6)
  RTOW_FH_SHIFT(6, 5)
  RTOW_FH_SHIFT(5, 4)
  RTOW_FH_SHIFT(4, 3)
  RTOW_FH_SHIFT(3, 2)
  RTOW_FH_SHIFT(2, 1)
  RTOW_FH_SHIFT(1, 0)
#undef RTOW_FH_SHIFT
  if (!b0) {
    L.t0 = t;
    L.i0 = id;
  }
}
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

// ---- BVH: the threaded walk of any_hit_bvh (rtow_occlude.h), bound from the list, no early exit ----
template <bool LDS>
__device__ __forceinline__ void first_hits_bvh(const Image<LDS> &im, const DevScene &sc, V3 o, V3 d, real time, double tmax,
                                               bool active, int max_hits, const int32_t *map, HitList &L,
                                               uint32_t &nnode, uint32_t &nprim) {
  list_clear(L, tmax);
  double bound = tmax;
  const RayForms ray = make_ray_forms(o, d, time);
  const float ix = safe_inv((float)d.x), iy = safe_inv((float)d.y), iz = safe_inv((float)d.z);
  const float oix = (float)o.x * ix, oiy = (float)o.y * iy, oiz = (float)o.z * iz;
  const float tmin32 = 0.0009f;  // < RTOW_TMIN
  const float slack = 1.00002f;  // relative slack on the far side of the interval
  float tmax32 = round_up_f32(bound);
  const uint32_t END = (uint32_t)sc.n_nodes;
  const ImgOffsets off = {sc.off_ids, sc.off_sph, sc.off_mov, sc.off_tri, 0u, 0u, sc.off_sph32, sc.off_mov32};
  uint32_t node = active ? 0u : END;
  uint32_t q0 = 0u, q1 = 0u, q2 = 0u, q3 = 0u;  // queued leaves (0 = empty), oldest first
  for (;;) {
    if (node < END) {
      const float4 r0 = im.f4(node * 32u), r1 = im.f4(node * 32u + 16u);
      ++nnode;
      const float ax = fmaf(r0.x, ix, -oix), bx = fmaf(r0.w, ix, -oix);
      const float ay = fmaf(r0.y, iy, -oiy), by = fmaf(r1.x, iy, -oiy);
      const float az = fmaf(r0.z, iz, -oiz), bz = fmaf(r1.y, iz, -oiz);
      const float tnear = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin32));
      const float tfar = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax32));
      const bool hit = tnear <= tfar * slack;
      const uint32_t skip = __float_as_uint(r1.z), leaf = __float_as_uint(r1.w);
      if (hit && leaf != 0u) {
        if (q0 == 0u)
          q0 = leaf;
        else if (q1 == 0u)
          q1 = leaf;
        else if (q2 == 0u)
          q2 = leaf;
        else
          q3 = leaf;
      }
      node = (hit && leaf == 0u) ? node + 1u : skip;
    }
    const bool any_walking = __any(node < END);
    if (__any(q3 != 0u) || !any_walking) {
      if (q0 != 0u) {
        // one primitive per test: the hit tests overwrite one Closest, and every accepted primitive is a candidate
        const uint32_t first = q0 >> 3, count = q0 & 7u;
        for (uint32_t k = 0; k < count; ++k) {
          Closest c = candidate(bound);
          int last_id = -1;
          leaf_test<LDS, false>(im, sc, off, first + k, 1u, ray, c, nprim, last_id);
          list_take<false>(L, c, map, max_hits, bound);
        }
        tmax32 = round_up_f32(bound);
      }
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = 0u;
      if (!__any(node < END) && !__any(q0 != 0u)) break;
    }
  }
}

// ---- GRID: the 3D-DDA of any_hit_grid (rtow_occlude.h: step sign from the reciprocal), bound from the list ----
// The fast build walks the unit direction: the list holds distances, and so does the bound (the kernel converts at
// output, as closest_hit_grid does when its walk is complete).
template <bool LDS>
__device__ __forceinline__ void first_hits_grid(const Image<LDS> &im, const DevScene &sc, V3 o, V3 d, real time,
                                                  double tmax, bool active, int max_hits, const int32_t *map, HitList &L,
                                                  uint32_t &nnode, uint32_t &nprim, uint32_t leaf_votes) {
#ifdef RTOW_UNIT_RAYS
  const double a_ref = dot(d, d);
  const double inv_len = fast_rsqrt(a_ref), len = a_ref * inv_len;
  d = d * inv_len;
  const RayForms ray = make_unit_ray_forms(o, d, time, len);
  const float tmin32w = 0.0009f * (float)len;
  const double tmaxw = tmax * len;
#else
  const RayForms ray = make_ray_forms(o, d, time);
  const float tmin32w = 0.0009f;
  const double tmaxw = tmax;
#endif
  list_clear(L, tmaxw);
  double bound = tmaxw;
  ImgOffsets off = {sc.g_off_ids, sc.g_off_sph, sc.g_off_mov, sc.g_off_tri, 0u, 0u, sc.g_off_sph32, sc.g_off_mov32};
  const RTOW_CONST float *hf = (const RTOW_CONST float *)sc.gblob;
  const RTOW_CONST int32_t *hi = (const RTOW_CONST int32_t *)sc.gblob;
  const float gx = hf[0], gy = hf[1], gz = hf[2];
  const float cx = hf[3], cy = hf[4], cz = hf[5];
  const float icx = hf[6], icy = hf[7], icz = hf[8];
  const int nx = hi[9], ny = hi[10], nz = hi[11];
  const uint32_t n_large = (uint32_t)hi[12], off_large = (uint32_t)hi[13];
  off.fat = (uint32_t)hi[14];
  off.fat_stride = (uint32_t)hi[15];

  // the large primitives (the ground sphere), for every ray, one at a time
  if (active && n_large != 0u) {
    const uint32_t lf = (off_large - off.ids) >> 2;
    for (uint32_t k = 0; k < n_large; ++k) {
      Closest c = candidate(bound);
      int last_id = -1;
      leaf_test<LDS, false, 0, true>(im, sc, off, lf + k, 1u, ray, c, nprim, last_id);
      list_take<true>(L, c, map, max_hits, bound);
    }
  }
  float tmax32 = round_up_f32(bound);
  stage_prio<kPrioSetup>();  // (the issue priorities of any_hit_grid: set-up, cell walk, cell lists)

  const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
  const float ox = (float)o.x, oy = (float)o.y, oz = (float)o.z;
  const float ix = safe_inv(dx), iy = safe_inv(dy), iz = safe_inv(dz);
  const float oix = ox * ix, oiy = oy * iy, oiz = oz * iz;
  const float hx = fmaf((float)nx, cx, gx), hy = fmaf((float)ny, cy, gy), hz = fmaf((float)nz, cz, gz);
  const float ax = fmaf(gx, ix, -oix), bx = fmaf(hx, ix, -oix);
  const float ay = fmaf(gy, iy, -oiy), by = fmaf(hy, iy, -oiy);
  const float az = fmaf(gz, iz, -oiz), bz = fmaf(hz, iz, -oiz);
  const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin32w));
  const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax32));
  bool walking = active && t0 <= t1 * 1.00002f;

  const float px = fmaf(t0, dx, ox), py = fmaf(t0, dy, oy), pz = fmaf(t0, dz, oz);
  int c0 = (int)floorf((px - gx) * icx), c1 = (int)floorf((py - gy) * icy), c2 = (int)floorf((pz - gz) * icz);
  c0 = min(max(c0, 0), nx - 1);
  c1 = min(max(c1, 0), ny - 1);
  c2 = min(max(c2, 0), nz - 1);
  const bool fx = !(ix < 0.0f), fy = !(iy < 0.0f), fz = !(iz < 0.0f);  // the sign of the reciprocal: -0.0 steps down
  float tmx = fmaf(fmaf((float)(c0 + (fx ? 1 : 0)), cx, gx), ix, -oix);
  float tmy = fmaf(fmaf((float)(c1 + (fy ? 1 : 0)), cy, gy), iy, -oiy);
  float tmz = fmaf(fmaf((float)(c2 + (fz ? 1 : 0)), cz, gz), iz, -oiz);
  const float tdx = fabsf(cx * ix), tdy = fabsf(cy * iy), tdz = fabsf(cz * iz);
  int remx = fx ? nx - 1 - c0 : c0, remy = fy ? ny - 1 - c1 : c1, remz = fz ? nz - 1 - c2 : c2;
  const int incx = fx ? 1 : -1, incy = fy ? nx : -nx, incz = fz ? nx * ny : -(nx * ny);
  int idx = (c2 * ny + c1) * nx + c0;

  int last_id = -1;  // leaf_test's one-entry mailbox, kept across cells: a repeat was tested against a bound no smaller
  stage_prio<kPrioStage>();
  uint32_t q0 = 0u, q1 = 0u;
  for (;;) {
    if (walking && q1 == 0u) {  // (a lane with two cells queued waits for the next leaf phase)
      const uint32_t cw = im.u32(sc.g_off_cells + 4u * (uint32_t)idx);
      ++nnode;
      if (cw != 0u) {
        if (q0 == 0u)
          q0 = cw;
        else
          q1 = cw;
      }
      const float tnext = fminf(fminf(tmx, tmy), tmz);
      const bool sx = tmx == tnext;
      const bool sy = !sx && tmy == tnext;
      const int rem = sx ? remx : (sy ? remy : remz);
      walking = rem > 0 && !(tnext > tmax32);
      idx += sx ? incx : (sy ? incy : incz);
      tmx += sx ? tdx : 0.0f;
      tmy += sy ? tdy : 0.0f;
      tmz += (!sx && !sy) ? tdz : 0.0f;
      remx -= sx ? 1 : 0;
      remy -= sy ? 1 : 0;
      remz -= (!sx && !sy) ? 1 : 0;
    }
    const bool any_walking = __any(walking);
    const unsigned long long m_pending = __ballot(q0 != 0u);
    if ((m_pending != 0ull && ((uint32_t)__popcll(m_pending) >= leaf_votes || __ballot(walking && q1 == 0u) == 0ull)) ||
        !any_walking) {
      stage_prio<kPrioLeaf>();
      if (q0 != 0u) {
        const uint32_t first = q0 >> 8, count = q0 & 255u;
        for (uint32_t k = 0; k < count; ++k) {
          Closest c = candidate(bound);
          leaf_test<LDS, true>(im, sc, off, first + k, 1u, ray, c, nprim, last_id);
          list_take<true>(L, c, map, max_hits, bound);
        }
        tmax32 = round_up_f32(bound);
      }
      q0 = q1;
      q1 = 0u;
      stage_prio<kPrioStage>();
      if (!__any(walking) && !__any(q0 != 0u)) break;
    }
  }
}

// ---- BVH4: the trip loop of any_hit_bvh4 (rtow_occlude.h), bound from the list, no early exit ----
template <bool FULL>
__device__ __forceinline__ void first_hits_bvh4(const Bvh4Reader<FULL> &im, const DevScene &sc, const TraceParams &P, V3 o,
                                                V3 d, double tmax, bool active, uint32_t lane_g, int max_hits,
                                                const int32_t *map, HitList &L, uint32_t &nnode, uint32_t &nprim) {
  list_clear(L, tmax);
  double bound = tmax;
  const V3d o64 = to_f64(o), d64 = to_f64(d);
  const Bvh4Ray ray = bvh4_ray<FULL>(sc, o, d);
  const Bvh4Stack st = bvh4_stack(sc);
  float tmax32 = round_up_f32(bound);
  uint32_t sa = st.lds;
  uint32_t cur = active ? 0u : kRefNone;  // node 0 = root
  uint32_t q0 = kRefNone, q1 = kRefNone;  // queued leaves, oldest first
  if constexpr (FULL) stage_prio<kPrioLeaf>();
  for (;;) {
    // (FOLD = false: the slack is multiplied per node, as in the state machine — six registers the list needs)
    bvh4_step<FULL, false>(im, P, ray, tmax32, st, lane_g, cur, sa, q0, q1, nnode);
    const bool any_walking = __any(cur != kRefNone);
    const unsigned long long m_pending = __ballot(q0 != kRefNone);
    if ((m_pending != 0ull && ((uint32_t)__popcll(m_pending) >= P.leaf_votes || __ballot(bvh4_busy(cur, q1)) == 0ull)) ||
        !any_walking) {
      if (q0 != kRefNone) {
        // the leaf's triangles as one-triangle leaves (leaf word: rtow_bvh4.h, [first : 18][count - 1 : 2])
        const uint32_t first = (q0 & (kRefLeaf - 1u)) >> 2, count = (q0 & 3u) + 1u;
        for (uint32_t k = 0; k < count; ++k) {
          Closest c = candidate(bound);
          bvh4_leaf<FULL>(im, sc, kRefLeaf | ((first + k) << 2), o64, d64, c, nprim);
          list_take<false>(L, c, map, max_hits, bound);
        }
        tmax32 = round_up_f32(bound);
      }
      q0 = q1;
      q1 = kRefNone;
      if (!__any(cur != kRefNone) && !__any(q0 != kRefNone)) break;
    }
  }
  if constexpr (FULL) stage_prio<kPrioStage>();
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
    RTOW_FCAT(rtow_first_hits_, RTOW_SUFFIX)(const FirstHitsParams Q) {
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
    if (in) {
      const vd2 *r = reinterpret_cast<const vd2 *>(Q.rays + (size_t)i * kRayBytes);
      const vd2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];  // {ox, oy} {oz, time} {dx, dy} {dz, tmax}
      wo = {r0.x, r0.y, r1.x};
      wtime = r1.y;
      wd = {r2.x, r2.y, r3.x};
      tmax = r3.y;
    }
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
      const vd2 *r = reinterpret_cast<const vd2 *>(Q.rays + (size_t)i * kRayBytes);
      const vd2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
      const V3 ro = {r0.x, r0.y, r1.x}, rd = {r2.x, r2.y, r3.x};
      const real rtime = r1.y;
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

  // statistics: one atomic per wave and counter
  const unsigned long long c0 = wave_sum(nprim), c1 = wave_sum(nnode);
  if (lane == 0) {
    atomicAdd(&Q.counters[0], c0);
    atomicAdd(&Q.counters[1], c1);
  }
}

}  // namespace

#include "rtow_kernel_launch.h"

template <int K, bool L>
static KernelVariant<FirstHitsParams> first_hits_kernel(unsigned lds_bytes) {
  return kernel_variant<RTOW_FCAT(rtow_first_hits_, RTOW_SUFFIX)<K, L>, FirstHitsParams>(lds_bytes);
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

int RTOW_FCAT(launch_first_hits_, RTOW_SUFFIX)(const TraceParams &p, const void *rays, void *hits, int32_t *counts,
                                               uint32_t n, int32_t max_hits, const int32_t *map,
                                               unsigned long long *counters, int kernel, int grid, int block,
                                               unsigned lds_bytes, void *stream) {
  FirstHitsParams q;
  q.P = p;
  q.rays = (const unsigned char *)rays;
  q.hits = (unsigned char *)hits;
  q.counts = counts;
  q.n = n;
  q.max_hits = max_hits;
  q.map = map;
  q.counters = counters;
  const KernelVariant<FirstHitsParams> v = first_hits_variant(kernel, lds_bytes, p.sc.b4_half == 0u);
  return v.fn ? v.launch(q, grid, block, v.lds_bytes, (hipStream_t)stream) : (int)hipErrorInvalidValue;
}

// Workgroups per CU that stay resident (resident_blocks, rtow_kernel_launch.h).  Both 4-wide variants have the same
// launch bounds; the full-LDS one stands for both.
int RTOW_FCAT(first_hits_occupancy_, RTOW_SUFFIX)(int kernel, int block, unsigned lds_bytes, int *vgprs) {
  const KernelVariant<FirstHitsParams> v = first_hits_variant(kernel, lds_bytes, true);
  return resident_blocks(v.fn, block, v.lds_bytes, vgprs);
}

}  // namespace rtow
