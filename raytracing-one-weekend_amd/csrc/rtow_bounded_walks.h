// rtow_bounded_walks.h — the walks of the queries that are bounded by the caller's tmax: any-hit (rtow_occlude.h) and
// first-k-hits (rtow_first_hits.h).  Included inside `namespace rtow { namespace {` after the trace headers, the way
// the other walk headers are.  These are the render's walks (rtow_trace_bvh.h, rtow_trace_grid.h, rtow_trace_bvh4.h)
// without suspend / resume, built from the render's pieces (Image, the ray forms, leaf_test, the hit tests, the 4-wide
// step, leaf and stack, the DDA step), which are included read-only: the benchmarked walks themselves are not touched.
// What differs from them: the bound that boxes, cells and primitive tests cull against starts at the ray's tmax instead
// of +inf, and what happens to an accepted primitive is the caller's business.
//
// The caller's business is a sink: a plain struct passed by reference, every member __forceinline__.
//   void  seed(double tmax)      the walk's start; `tmax` is in the walk's ray parameter (the fast build's grid walk
//                                runs on the unit direction: a distance, tmax * |d|)
//   float bound32() const        the current bound for box and cell culling, rounded up to f32.  It may only shrink.
//   void  list<LDS, CELL>(..)    tests one queued list of an image: a BVH leaf, or (CELL) a grid cell
//   void  large<LDS>(..)         tests the grid's large-primitive list, which every ray meets before the DDA
//   void  leaf4<FULL>(..)        tests one queued leaf of the 4-wide image
//   bool  done() const           asked after the large list and after each leaf phase: the lane wants nothing more.
//                                The walk then drops the node in hand, the queues and the stack; the wave keeps voting.
//   kFold                        bvh4_step's FOLD argument
// The sink owns leaf_test's one-entry mailbox (`last_id`), so how long an entry lives is the sink's decision too.
//
// Why a bound below +inf is exact.  A primitive's hit test with upper bound b accepts exactly when its unbounded test
// returns a t <= b, with the same bits: sphere_resolve picks its root by tmin alone (root1 <= root2, so a near root
// beyond b rules out the far one), a triangle has one t.  The f32 box and cell intervals are conservative supersets, as
// they are for the closest-hit walks, and every comparison against the bound is inclusive (boxes and cells with <=, the
// primitive tests accept t <= b), so a primitive AT the bound is visited.  A bound that only shrinks never readmits
// what it rejected.  Hence a walk meets every primitive whose t lies within the final bound, whatever the strategy,
// builder or schedule: bit-determined in the strict build.  (The fast build's grid walk compares distances and its
// triangle test compares t * det: its answer can differ from `t <= tmax` on the fast closest hit only when t is within
// rounding of tmax.)

// ---- BVH: the threaded walk of closest_hit_bvh (rtow_trace_bvh.h) ----
template <bool LDS, class Sink>
__device__ __forceinline__ void bounded_walk_bvh(const Image<LDS> &im, const DevScene &sc, V3 o, V3 d, real time,
                                                 double tmax, bool active, Sink &sink, uint32_t &nnode, uint32_t &nprim) {
  sink.seed(tmax);
  const RayForms ray = make_ray_forms(o, d, time);
  const float ix = safe_inv((float)d.x), iy = safe_inv((float)d.y), iz = safe_inv((float)d.z);
  const float oix = (float)o.x * ix, oiy = (float)o.y * iy, oiz = (float)o.z * iz;
  const float tmin32 = 0.0009f;  // < RTOW_TMIN
  const float slack = 1.00002f;  // relative slack on the far side of the interval
  float tmax32 = sink.bound32();
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
        sink.template list<LDS, false>(im, sc, off, q0 >> 3, q0 & 7u, ray, nprim);
        tmax32 = sink.bound32();
      }
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = 0u;
      if (sink.done()) {
        node = END;
        q0 = q1 = q2 = 0u;
      }
      if (!__any(node < END) && !__any(q0 != 0u)) break;
    }
  }
}

// ---- GRID: the 3D-DDA of closest_hit_grid (rtow_trace_grid.h) ----
// The DDA's step direction is taken from the sign of the reciprocal it steps with (1 / -0.0 is negative), not from
// `d >= 0` as the render's walk does: the two disagree for a -0.0 component, which made that walk step the wrong way
// (rtow_query.h hands it +0.0 instead; here the walk is consistent by construction and takes the caller's direction).
template <bool LDS, class Sink>
__device__ __forceinline__ void bounded_walk_grid(const Image<LDS> &im, const DevScene &sc, V3 o, V3 d, real time,
                                                  double tmax, bool active, Sink &sink, uint32_t &nnode, uint32_t &nprim,
                                                  uint32_t leaf_votes) {
#ifdef RTOW_UNIT_RAYS
  // the fast build walks the unit direction (rtow_trace_bvh.h, RTOW_UNIT_RAYS): its ray parameter is a distance, and so
  // is the bound it starts from and every t the sink sees
  const double a_ref = dot(d, d);
  const double inv_len = fast_rsqrt(a_ref), len = a_ref * inv_len;
  d = d * inv_len;
  const RayForms ray = make_unit_ray_forms(o, d, time, len);
  const float tmin32w = 0.0009f * (float)len;
  sink.seed(tmax * len);
#else
  const RayForms ray = make_ray_forms(o, d, time);
  const float tmin32w = 0.0009f;
  sink.seed(tmax);
#endif
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

  // the large primitives (the ground sphere), for every ray, before the DDA
  if (active && n_large != 0u) sink.template large<LDS>(im, sc, off, (off_large - off.ids) >> 2, n_large, ray, nprim);
  float tmax32 = sink.bound32();
  stage_prio<kPrioSetup>();  // (the issue priorities of closest_hit_grid: set-up, cell walk, cell lists)

  // clip the ray to the grid bounds (f32, conservative by the padding of rtow_grid.h)
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
  bool walking = active && !sink.done() && t0 <= t1 * 1.00002f;

  // starting cell and DDA state (rtow_dda_step.h)
  const float px = fmaf(t0, dx, ox), py = fmaf(t0, dy, oy), pz = fmaf(t0, dz, oz);
  int c0 = (int)floorf((px - gx) * icx), c1 = (int)floorf((py - gy) * icy), c2 = (int)floorf((pz - gz) * icz);
  c0 = min(max(c0, 0), nx - 1);
  c1 = min(max(c1, 0), ny - 1);
  c2 = min(max(c2, 0), nz - 1);
  const bool fx = !(ix < 0.0f), fy = !(iy < 0.0f), fz = !(iz < 0.0f);  // (see above: the sign of the reciprocal)
  DdaWalk3 w;
  w.tmx = fmaf(fmaf((float)(c0 + (fx ? 1 : 0)), cx, gx), ix, -oix);
  w.tmy = fmaf(fmaf((float)(c1 + (fy ? 1 : 0)), cy, gy), iy, -oiy);
  w.tmz = fmaf(fmaf((float)(c2 + (fz ? 1 : 0)), cz, gz), iz, -oiz);
  w.tdx = fabsf(cx * ix), w.tdy = fabsf(cy * iy), w.tdz = fabsf(cz * iz);
  w.remx = fx ? nx - 1 - c0 : c0, w.remy = fy ? ny - 1 - c1 : c1, w.remz = fz ? nz - 1 - c2 : c2;
  w.incx = fx ? 1 : -1, w.incy = fy ? nx : -nx, w.incz = fz ? nx * ny : -(nx * ny);
  w.idx = (c2 * ny + c1) * nx + c0;

  stage_prio<kPrioStage>();
  uint32_t q0 = 0u, q1 = 0u;
  for (;;) {
    if (walking && q1 == 0u) {  // (a lane with two cells queued waits for the next leaf phase)
      const uint32_t cw = im.u32(sc.g_off_cells + 4u * (uint32_t)w.idx);
      ++nnode;
      if (cw != 0u) {
        if (q0 == 0u)
          q0 = cw;
        else
          q1 = cw;
      }
      [[maybe_unused]] float t_entry;
      walking = dda_step(w, tmax32, t_entry);
    }
    // leaf phase: when `leaf_votes` lanes hold a queued cell, when no lane can take a step, or at the end
    const bool any_walking = __any(walking);
    const unsigned long long m_pending = __ballot(q0 != 0u);
    if ((m_pending != 0ull && ((uint32_t)__popcll(m_pending) >= leaf_votes || __ballot(walking && q1 == 0u) == 0ull)) ||
        !any_walking) {
      stage_prio<kPrioLeaf>();
      if (q0 != 0u) {
        sink.template list<LDS, true>(im, sc, off, q0 >> 8, q0 & 255u, ray, nprim);
        tmax32 = sink.bound32();
      }
      q0 = q1;
      q1 = 0u;
      if (sink.done()) {  // the lane's DDA stops here
        walking = false;
        q0 = 0u;
      }
      stage_prio<kPrioStage>();
      if (!__any(walking) && !__any(q0 != 0u)) break;
    }
  }
}

// ---- BVH4: the trip loop of closest_hit_bvh4 (rtow_trace_bvh4.h) ----
template <bool FULL, class Sink>
__device__ __forceinline__ void bounded_walk_bvh4(const Bvh4Reader<FULL> &im, const DevScene &sc, const TraceParams &P,
                                                  V3 o, V3 d, double tmax, bool active, uint32_t lane_g, Sink &sink,
                                                  uint32_t &nnode, uint32_t &nprim) {
  sink.seed(tmax);
  const V3d o64 = to_f64(o), d64 = to_f64(d);
  const Bvh4Ray ray = bvh4_ray<FULL>(sc, o, d);
  const Bvh4Stack st = bvh4_stack(sc);
  float tmax32 = sink.bound32();
  uint32_t sa = st.lds;
  uint32_t cur = active ? 0u : kRefNone;  // node 0 = root
  uint32_t q0 = kRefNone, q1 = kRefNone;  // queued leaves, oldest first
  if constexpr (FULL) stage_prio<kPrioLeaf>();
  for (;;) {
    bvh4_step<FULL, Sink::kFold>(im, P, ray, tmax32, st, lane_g, cur, sa, q0, q1, nnode);
    const bool any_walking = __any(cur != kRefNone);
    const unsigned long long m_pending = __ballot(q0 != kRefNone);
    if ((m_pending != 0ull && ((uint32_t)__popcll(m_pending) >= P.leaf_votes || __ballot(bvh4_busy(cur, q1)) == 0ull)) ||
        !any_walking) {
      if (q0 != kRefNone) {
        sink.template leaf4<FULL>(im, sc, q0, o64, d64, nprim);
        tmax32 = sink.bound32();
      }
      q0 = q1;
      q1 = kRefNone;
      if (sink.done()) {  // drop the node in hand, the queued leaf and the stack
        cur = kRefNone;
        q0 = kRefNone;
        sa = st.lds;
      }
      if (!__any(cur != kRefNone) && !__any(q0 != kRefNone)) break;
    }
  }
  if constexpr (FULL) stage_prio<kPrioStage>();
}
