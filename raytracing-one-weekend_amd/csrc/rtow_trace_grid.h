// rtow_trace_grid.h — part of the trace kernels (included by rtow_trace_body.h inside namespace rtow::{anonymous};
// see that file for the execution model).  The uniform-grid (3D-DDA) walk.
#pragma once
#include "rtow_dda_step.h"
// --------------------------------------------------------- closest hit: GRID ---
// 3D-DDA over the uniform grid of rtow_grid.h.  Primitives far larger than the rest (the
// ground sphere) are not in the grid; every ray tests that short list first.  Cells are
// visited in order along the ray; a non-empty cell is queued like a BVH leaf and tested in
// the SIMT-dense leaf phase.  The walk ends when the ray leaves the grid (integer cell
// counters, so at most nx+ny+nz steps whatever the floats do) or when the exit distance of
// the current cell is beyond the closest hit so far.
//
// Resumable walk.  A wave's walk lasts as long as its slowest lane — typically one or two rays that
// graze the ground and cross ten cells while the others need one or two.  When the walk has run
// `cap` loop trips and at most `max_open` lanes are still walking, it stops: the queued cells are
// tested, and every lane that is not finished remembers where it stands — the closest hit so far
// (`best`) and the ray parameter at which it entered its current cell (`t_resume` > 0).  The caller
// shades the finished lanes as usual and calls again in its next trip; a resumed lane skips the
// large-primitive list and re-enters the grid at t_resume (a hair earlier: the cell containing that
// point or its predecessor, so no cell is skipped; a cell tested twice changes nothing).  Because of that
// step back, `cap` must be at least 3 (the host clamps it): at most two consecutive cell crossings share one
// ray parameter, so three steps always end in a cell that starts later than the one the lane resumed in.
//
// FLAT (kSpecFlatY, rtow_device.h): the resident grid has ONE layer of cells in y.  The set-up and the step are the
// two-axis forms of rtow_dda_step.h: same cells in the same order, same t_entry; everything else is untouched.
//
// Per-scene constants.  The generic instantiation (SPEC == 0: the query, occlusion, radiance and guide kernels, and the
// trace kernels under RTOW_NO_SPEC) reads the 64-byte header of the image and derives the far planes, the clamps and the
// strides from it.  The specialised instantiations take all of that ready-made from `wk`, the block the host derived
// from the same header (rtow_walk_consts.h, TraceParams::walk): adjacent words of the kernel-argument segment in the
// order the walk consumes them, read with wide scalar loads at the walk's entry and waited for once.  Same values bit for
// bit, so same cells, same counters, same image; the arithmetic behind the constants is the same code for both.
// The block also names the first (up to four) static spheres of the large-primitive list — id and byte offset of the
// record — which are the same for every wave of every launch on a resident image.  The class-2 walk (static + moving
// spheres) tests those from wave-uniform values: no id reads, no dependent LDS round trip in front of the record reads,
// and none of the four per-lane `id < n_sph` tests that decide between the record formats there.  The class-1 walk keeps
// reading the ids: it has no such tests to lose, its ids arrive in VGPRs for nothing (one ds_read_b128), and a
// wave-uniform id costs a v_mov per accepted root (v_cndmask takes one scalar operand, and that is VCC) — measured
// slower than the id reads on the cover scene.
//
// CN: the type of the statistics counters: uint32_t, or WalkCount<> of rtow_trace_hit.h (empty in the trace kernels
// launched for a caller that takes no statistics).
template <bool LDS, bool ST, int SPEC = 0, bool FLAT = false, class CN = uint32_t>
__device__ __forceinline__ Closest closest_hit_grid(const Image<LDS> &im, const DevScene &sc, V3 o,
                                                    V3 d, real time, bool active, CN &nnode,
                                                    CN &nprim, Stamps<ST> &stamps, Closest best,
                                                    float &t_resume, uint32_t cap, uint32_t max_open,
                                                    uint32_t leaf_votes, const RTOW_CONST GridWalkConsts *wk = nullptr) {
  const bool resumed = t_resume > 0.0f;
  const float t_in = t_resume;
  if (!resumed) {
    best.t = (real)__builtin_huge_val();
    best.prim = -1;
  }
#ifdef RTOW_UNIT_RAYS
  // the walk runs on the unit direction (rtow_trace_bvh.h, RTOW_UNIT_RAYS): its ray parameter is a distance.  The
  // closest hit goes out in the caller's parameter, t = distance / |d|, ONCE: when the segment's walk is complete.  A
  // walk that stops to be resumed keeps `best.t` as the distance it is (the caller does not read it before the walk
  // is complete): converting there and back on every resume would round it differently for every schedule of the
  // wave, and the image must not depend on who traces what next to whom.
  const double a_ref = dot(d, d);
  const double inv_len = fast_rsqrt(a_ref), len = a_ref * inv_len;
  d = d * inv_len;
  const RayForms ray = make_unit_ray_forms(o, d, time, len);
  const float tmin32w = 0.0009f * (float)len;
#else
  const RayForms ray = make_ray_forms(o, d, time);
  const float tmin32w = 0.0009f;
#endif
  ImgOffsets off = {sc.g_off_ids, sc.g_off_sph, sc.g_off_mov, sc.g_off_tri, 0u, 0u, sc.g_off_sph32, sc.g_off_mov32};
  int last_id = -1;
  float gx, gy, gz, hx, hy, hz, cx, cy, cz, icx, icy, icz;
  int nx, ny, nxm1, nym1, nzm1, neg_nx, nxny, neg_nxny;
  [[maybe_unused]] int nz = 0;  // (the generic walk derives the far planes below, where it always did)
  uint32_t n_large, lf, cells;
  // the class walks: the head of the large list from the block (rtow_walk_consts.h) — ids and record offsets as
  // wave-uniform values; nf entries of the list are served from them, the rest by the generic loops below
  constexpr bool kLargeHead = SPEC == 2;
  [[maybe_unused]] uint32_t nf = 0u, lrec[4] = {0u, 0u, 0u, 0u};
  [[maybe_unused]] int lid[4] = {-1, -1, -1, -1};
  if constexpr (SPEC != 0) {
    // the host's block: wave-uniform scalar loads from the kernel-argument segment (the 3D walk's five words — cy, icy,
    // ny - 1 and the z strides — are dead in the two-axis walk and not loaded there)
    gx = wk->gx, gy = wk->gy, gz = wk->gz, hx = wk->hx, hy = wk->hy, hz = wk->hz;
    cx = wk->cx, cy = wk->cy, cz = wk->cz, icx = wk->icx, icy = wk->icy, icz = wk->icz;
    nx = wk->nx, ny = wk->ny, nxm1 = wk->nxm1, nym1 = wk->nym1, nzm1 = wk->nzm1;
    neg_nx = wk->neg_nx, nxny = wk->nxny, neg_nxny = wk->neg_nxny;
    n_large = wk->n_large, lf = wk->large_first, cells = wk->cells;
    off.fat = wk->fat;
    off.fat_stride = wk->fat_stride;
    if constexpr (kLargeHead) {
      nf = wk->n_large_fast;
#pragma unroll
      for (int j = 0; j < 4; ++j) lrec[j] = wk->large_rec[j], lid[j] = (int)wk->large_id[j];
      // (pinned here: left to itself the compiler sinks these loads into the list's branch, behind a wait of their own)
      asm volatile("" : "+s"(nf), "+s"(lrec[0]), "+s"(lrec[1]), "+s"(lrec[2]), "+s"(lrec[3]), "+s"(lid[0]), "+s"(lid[1]),
                   "+s"(lid[2]), "+s"(lid[3]));
    }
  } else {
    // header: wave-uniform scalar loads from the global copy of the image
    const RTOW_CONST float *hf = (const RTOW_CONST float *)sc.gblob;
    const RTOW_CONST int32_t *hi = (const RTOW_CONST int32_t *)sc.gblob;
    gx = hf[0], gy = hf[1], gz = hf[2];
    cx = hf[3], cy = hf[4], cz = hf[5];
    icx = hf[6], icy = hf[7], icz = hf[8];
    nx = hi[9], ny = hi[10], nz = hi[11];
    nxm1 = nx - 1, nym1 = ny - 1, nzm1 = nz - 1;
    neg_nx = -nx, nxny = nx * ny, neg_nxny = -(nx * ny);
    n_large = (uint32_t)hi[12];
    lf = ((uint32_t)hi[13] - off.ids) >> 2;  // (off_large: the list's byte offset in the image)
    cells = sc.g_off_cells;
    off.fat = (uint32_t)hi[14];
    off.fat_stride = (uint32_t)hi[15];
  }

  // the large primitives, for every ray.  Static spheres are taken four (then two) at a time:
  // all records are loaded and all discriminants computed before any hit branch, so LDS
  // latency and the f64 dependency chains of one test overlap the others.
  if (active && !resumed && n_large != 0u) {
    uint32_t k = 0;
    if constexpr (kLargeHead) {
      // Same tests, same operands and same order as the loops below run for these entries (sphere_disc of every
      // entry, then sphere_resolve in list order): the accepted (t, primitive), nprim and last_id are theirs.
      double dd[4], hh[4];
      if (nf == 4u) {  // (the cover scenes: the ground and the three big spheres)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double2 p0 = im.d2(lrec[j]), p1 = im.d2(lrec[j] + 16u);
          dd[j] = sphere_disc<double>(ray.o64, ray.d64, ray.a64, p0.x, p0.y, p1.x, p1.y, hh[j]);
        }
        nprim += 4u;
#pragma unroll
        for (int j = 0; j < 4; ++j) sphere_resolve<double>(dd[j], hh[j], ray.a64, ray.inv_a64, lid[j], ray.tmin, best);
        last_id = lid[3];
      } else if (nf != 0u) {  // one to three entries (wave-uniform branches)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if ((uint32_t)j < nf) {
            const double2 p0 = im.d2(lrec[j]), p1 = im.d2(lrec[j] + 16u);
            dd[j] = sphere_disc<double>(ray.o64, ray.d64, ray.a64, p0.x, p0.y, p1.x, p1.y, hh[j]);
          }
        nprim += nf;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if ((uint32_t)j < nf) {
            sphere_resolve<double>(dd[j], hh[j], ray.a64, ray.inv_a64, lid[j], ray.tmin, best);
            last_id = lid[j];
          }
      }
      k = nf;
    }
    for (; k + 3 < n_large; k += 4) {
      int id[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) id[j] = (int)im.u32(off.ids + 4u * (lf + k + j));
      if (SPEC == 1 || (id[0] < sc.n_sph && id[1] < sc.n_sph && id[2] < sc.n_sph && id[3] < sc.n_sph)) {
        double dd[4], hh[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t r = off.sph + 32u * (uint32_t)id[j];
          const double2 p0 = im.d2(r), p1 = im.d2(r + 16u);
          dd[j] = sphere_disc<double>(ray.o64, ray.d64, ray.a64, p0.x, p0.y, p1.x, p1.y, hh[j]);
        }
        nprim += 4u;
#pragma unroll
        for (int j = 0; j < 4; ++j) sphere_resolve<double>(dd[j], hh[j], ray.a64, ray.inv_a64, id[j], ray.tmin, best);
        last_id = id[3];
      } else {
        leaf_test<LDS, false, SPEC, true>(im, sc, off, lf + k, 4u, ray, best, nprim, last_id);
      }
    }
    for (; k + 1 < n_large; k += 2) {
      const int ia = (int)im.u32(off.ids + 4u * (lf + k)), ib = (int)im.u32(off.ids + 4u * (lf + k + 1));
      if (SPEC == 1 || (ia < sc.n_sph && ib < sc.n_sph)) {
        const uint32_t ra = off.sph + 32u * (uint32_t)ia, rb = off.sph + 32u * (uint32_t)ib;
        const double2 a0 = im.d2(ra), a1 = im.d2(ra + 16u), b0 = im.d2(rb), b1 = im.d2(rb + 16u);
        double ha, hb;
        const double da = sphere_disc<double>(ray.o64, ray.d64, ray.a64, a0.x, a0.y, a1.x, a1.y, ha);
        const double db = sphere_disc<double>(ray.o64, ray.d64, ray.a64, b0.x, b0.y, b1.x, b1.y, hb);
        nprim += 2u;
        sphere_resolve<double>(da, ha, ray.a64, ray.inv_a64, ia, ray.tmin, best);
        sphere_resolve<double>(db, hb, ray.a64, ray.inv_a64, ib, ray.tmin, best);
        last_id = ib;
      } else {
        leaf_test<LDS, false, SPEC, true>(im, sc, off, lf + k, 2u, ray, best, nprim, last_id);
      }
    }
    if (k < n_large) leaf_test<LDS, false, SPEC, true>(im, sc, off, lf + k, n_large - k, ray, best, nprim, last_id);
  }
  float tmax32 = round_up_f32(best.t);
  // the walk's set-up — clip against the grid, first cell, the DDA's increments: some eighty binary32 instructions and
  // no memory access — one step below the stage priority (round 5: +0.9 % on the cover scene once the rejection loops
  // were gone and VALU issue utilisation had fallen from 0.96 to 0.89)
  stage_prio<kPrioSetup>();

  // clip the ray to the grid bounds (f32, conservative by the padding of rtow_grid.h)
  const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
  const float ox = (float)o.x, oy = (float)o.y, oz = (float)o.z;
  const float ix = safe_inv(dx), iy = safe_inv(dy), iz = safe_inv(dz);
  const float oix = ox * ix, oiy = oy * iy, oiz = oz * iz;
  if constexpr (SPEC == 0) hx = fmaf((float)nx, cx, gx), hy = fmaf((float)ny, cy, gy), hz = fmaf((float)nz, cz, gz);
  const float ax = fmaf(gx, ix, -oix), bx = fmaf(hx, ix, -oix);
  const float ay = fmaf(gy, iy, -oiy), by = fmaf(hy, iy, -oiy);
  const float az = fmaf(gz, iz, -oiz), bz = fmaf(hz, iz, -oiz);
  const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), fmaxf(tmin32w, t_resume * 0.999999f)));
  const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax32));
  bool walking = active && t0 <= t1 * 1.00002f;

  // starting cell and DDA state (rtow_dda_step.h)
  const bool fx = dx >= 0.0f, fy = dy >= 0.0f, fz = dz >= 0.0f;
  const float tdx = fabsf(cx * ix), tdz = fabsf(cz * iz);
  const float px = fmaf(t0, dx, ox), pz = fmaf(t0, dz, oz);
  int c0 = (int)floorf((px - gx) * icx), c2 = (int)floorf((pz - gz) * icz);
  c0 = min(max(c0, 0), nxm1);
  c2 = min(max(c2, 0), nzm1);
  typename DdaWalkOf<FLAT>::type w;
  w.tmx = fmaf(fmaf((float)(c0 + (fx ? 1 : 0)), cx, gx), ix, -oix);
  w.tmz = fmaf(fmaf((float)(c2 + (fz ? 1 : 0)), cz, gz), iz, -oiz);
  w.tdx = tdx, w.tdz = tdz;
  w.remx = fx ? nxm1 - c0 : c0, w.remz = fz ? nzm1 - c2 : c2;
  w.incx = fx ? 1 : -1;
  if constexpr (FLAT) {
    // one layer in y (the host checked the header: ny == 1): the y cell is 0, its far wall is the slab's exit plane —
    // the generic tmy, fmaf(fmaf((float)(fy ? 1 : 0), cy, gy), iy, -oiy), is `by` or `ay` of the clip above
    w.ty_exit = fy ? by : ay;
    w.incz = fz ? nx : neg_nx;
    w.idx = c2 * nx + c0;
  } else {
    const float py = fmaf(t0, dy, oy);
    int c1 = (int)floorf((py - gy) * icy);
    c1 = min(max(c1, 0), nym1);
    w.tmy = fmaf(fmaf((float)(c1 + (fy ? 1 : 0)), cy, gy), iy, -oiy);
    w.tdy = fabsf(cy * iy);
    w.remy = fy ? nym1 - c1 : c1;
    w.incy = fy ? nx : neg_nx, w.incz = fz ? nxny : neg_nxny;
    w.idx = (c2 * ny + c1) * nx + c0;
  }

  stage_prio<kPrioStage>();
  uint32_t q0 = 0u, q1 = 0u;
  float t_entry = t0;  // ray parameter at which the lane entered its current cell
  uint32_t trips = 0u;  // wave-uniform
  for (;;) {
    if constexpr (ST) {
      stamps.iters += 1;
      const unsigned long long m_step = __ballot(walking && q1 == 0u);
      stamps.step_lanes += (unsigned long long)__popcll(m_step);
      if (m_step != 0ull && (m_step & ~stamps.primary) == 0ull) stamps.iters_cam += 1;
    }
    if (walking && q1 == 0u) {  // (a lane with two cells queued waits for the next leaf phase)
      const uint32_t cw = im.u32(cells + 4u * (uint32_t)w.idx);
      ++nnode;
      if (cw != 0u) {
        if (q0 == 0u)
          q0 = cw;
        else
          q1 = cw;
      }
      walking = dda_step(w, tmax32, t_entry);
    }
    const unsigned long long m_walking = __ballot(walking);
    const bool any_walking = m_walking != 0ull;
    ++trips;
    // stop here and resume in the caller's next trip?  (never on the first trips: most lanes finish there)
    // ... never before every resumed lane has got strictly beyond the point it resumed at: progress of a
    // resumed walk is then structural (t_entry takes finitely many f32 values), whatever the rounding does
    // when a ray runs through a cell corner
    const bool suspend = any_walking && trips >= cap && (uint32_t)__popcll(m_walking) <= max_open &&
                         __ballot(walking && resumed && !(t_entry > t_in)) == 0ull;
    // leaf phase: when `leaf_votes` lanes hold a queued cell, when no lane can take a step, or at the end
    const unsigned long long m_pending = __ballot(q0 != 0u);
    if ((m_pending != 0ull && ((uint32_t)__popcll(m_pending) >= leaf_votes || __ballot(walking && q1 == 0u) == 0ull)) ||
        !any_walking || suspend) {
      stamps.mark(RG_WALK, __ballot(active));
      if constexpr (ST) {
        stamps.phases += 1;
        stamps.leaf_lanes += (unsigned long long)__popcll(m_pending);
        if (m_pending != 0ull && (m_pending & ~stamps.primary) == 0ull) stamps.phases_cam += 1;
      }
      stage_prio<kPrioLeaf>();  // a chain of three dependent LDS reads per list entry: first in line for the issue slots
      if (q0 != 0u) leaf_test<LDS, true, SPEC>(im, sc, off, q0 >> 8, q0 & 255u, ray, best, nprim, last_id);
      q0 = q1;
      q1 = 0u;
      if (suspend && __any(q0 != 0u)) {  // both queued cells before stopping
        if (q0 != 0u) leaf_test<LDS, true, SPEC>(im, sc, off, q0 >> 8, q0 & 255u, ray, best, nprim, last_id);
        q0 = 0u;
      }
      tmax32 = round_up_f32(best.t);
      stamps.mark(RG_LEAF, m_pending);
      stage_prio<kPrioStage>();
      if (suspend) {
        // a lane whose next cell starts beyond the hit it has just found is finished after all
        t_resume = (walking && !(t_entry > tmax32)) ? t_entry : 0.0f;
#ifdef RTOW_UNIT_RAYS
        if (!(t_resume > 0.0f)) best.t = best.t * inv_len;  // (the lanes whose walk is complete)
#endif
        return best;
      }
      if (!any_walking && !__any(q0 != 0u)) break;
    }
  }
  t_resume = 0.0f;
#ifdef RTOW_UNIT_RAYS
  best.t = best.t * inv_len;
#endif
  return best;
}

