// rtow_sweep_walks.h — the per-primitive sweep formulas and the three pruned sweep walks of the swept-sphere query
// (rtow_sweep.h).  Included inside namespace rtow { namespace { ... } } after rtow_point_walks.h, whose record layouts,
// distance formulas (point_sphere, point_triangle), node decoding (bvh4_node), stack keys and arithmetic (pq_sqrt,
// pq_div) it uses read-only.
//
// A sweep is a sphere of radius rho whose centre travels p(t) = o + d t; a primitive answers with the smallest t in
// [0, bound] at which its distance to p(t) is <= rho (include/rtow.h has the definition).  The formulas below are
// written once, in a fixed operation order: the strict build compiles them with -ffp-contract=off and
// tests/sweep_ref.py mirrors them in numpy bit for bit.
//
// Every root is taken through the foot of the perpendicular, not through the textbook discriminant h^2 - a c, which
// cancels for an origin far from the scene and for a sweep nearly parallel to an edge (sweep_root): with t0 = -h / a
// and q = w + d t0 the perpendicular from the centre to the line of travel, the roots of |w + d t| = r are
// t0 -+ sqrt((r^2 - q.q) / a).  q carries one rounding of |w| and one of |t0 d| per component, so the distance of the
// contact from the surface is off by a few u (|w| + |t d|) whatever the angle (DESIGN §4.19 counts them).
//
// Per primitive (sweep_sphere, sweep_triangle):
//   * start overlap: point_sphere / point_triangle at o gives a distance <= rho: t = 0 and the overlap flag;
//   * otherwise NO piece asks again whether the sweep starts outside it.  Over the reals a failed overlap test implies
//     it; in binary64 the overlap test (a rounded distance against rho) and a second test (rounded squares against
//     rho^2, (R +- rho)^2) disagree on a shell a few ulps thick, and a sweep that starts there — one that continues
//     from the centre of an earlier contact — would belong to neither branch and pass through the primitive it rests
//     on.  Instead every near root is clamped at 0 (sweep_root), so a start that a piece's own arithmetic puts inside
//     it answers t = 0 (without the overlap flag: the contact is at rho within the band);
//   * sphere, R = sqrt(|r^2|): from the outer side (w.w >= |r^2|) the near root of |p - c| = R + rho if the centre
//     approaches (h < 0) and the perpendicular is short enough (r^2 - q.q >= 0: a tangent pass touches); from the
//     inner side (w.w < |r^2|, which with no overlap means R > rho) the far root of |p - c| = R - rho, which exists
//     for every direction: a negative r^2 - q.q there is rounding and counts as 0;
//   * triangle, the minimum of: the face (n.n > 0, the centre approaching the plane: where it reaches the offset
//     plane on its side — at once when it starts within the slab — if the Gram-form barycentrics of that point lie
//     inside), the three edges (e.e > 0: the near root of the cylinder of radius rho about the edge line in the plane
//     across the edge, if the sweep approaches the axis and the axial parameter at contact lies in [0, e.e]) and the
//     three vertices (the near root of the sphere of radius rho, if the sweep approaches).  A start inside a piece
//     that the overlap test did not see lies outside the triangle's own region of that piece (beyond a cap, beside the
//     prism), where the axial or barycentric test rejects it, or in the shell.
// A candidate whose terms overflow or are NaN fails a comparison and is no candidate: no NaN leaves these functions for
// a finite query, and +inf means "none".
//
// Walks: ray walks against boxes inflated by pad = rho + sigma, with the binary64 slab test below and the near clamp
// at 0.  sigma = 2^-40 (|o|_1 + M + rho), M the root box's magnitude, is above every rounding of the slab arithmetic and
// of a candidate's contact point (DESIGN §4.19 has the argument), the cube the box is grown by contains the sphere, and
// every comparison against the bound is inclusive: a walk meets every primitive whose computed t is within the final
// bound.  The sink orders answers by (t, insertion index), so the strict answer is that of the definition under every
// walk, builder and schedule.

constexpr uint32_t kSweepBytes = 80u, kSweepHitBytes = 80u;  // rtow_sweep_t, rtow_sweep_hit_t (include/rtow.h)

struct SweepRay {
  V3d o, d;
  double time, rho;
  double inv_a;  // 1 / d.d
};

constexpr double kNoSweep = __builtin_huge_val();

// The near (FAR: far) root of |w + d t| = r given h = w.d and inv_a = 1 / d.d, clamped to t >= 0; +inf when the line
// passes farther than r.  The far root is asked for from inside the ball only, where the line cannot pass farther: a
// negative r^2 - q.q is then 0 (a NaN stays one and is no candidate).
template <bool FAR>
__device__ __forceinline__ double sweep_root(V3d w, V3d d, double h, double inv_a, double r) {
  const double t0 = -(h * inv_a);
  const V3d q = w + d * t0;
  double dd = r * r - dot(q, q);
  if (FAR && dd < 0.0) dd = 0.0;
  if (!(dd >= 0.0)) return kNoSweep;
  const double s = pq_sqrt(dd * inv_a);
  const double t = FAR ? t0 + s : t0 - s;
  return t > 0.0 ? t : (t <= 0.0 ? 0.0 : kNoSweep);
}

__device__ __forceinline__ double sweep_sphere(const SweepRay &r, double cx, double cy, double cz, double r2, bool &ov) {
  V3d q;
  ov = point_sphere<false>(r.o, cx, cy, cz, r2, q) <= r.rho;
  if (ov) return 0.0;
  const double R = pq_sqrt(fabs(r2));
  const V3d w = {r.o.x - cx, r.o.y - cy, r.o.z - cz};
  const double L2 = dot(w, w), h = dot(w, r.d);
  const double ro = R + r.rho, ri = R - r.rho;
  if (L2 < fabs(r2)) return ri > 0.0 ? sweep_root<true>(w, r.d, h, r.inv_a, ri) : kNoSweep;
  return h < 0.0 ? sweep_root<false>(w, r.d, h, r.inv_a, ro) : kNoSweep;
}

// The sphere of radius rho about a vertex, w = o - vertex.
__device__ __forceinline__ double sweep_vertex(const SweepRay &r, V3d w) {
  const double h = dot(w, r.d);
  if (!(h < 0.0)) return kNoSweep;
  return sweep_root<false>(w, r.d, h, r.inv_a, r.rho);
}

// The cylinder of radius rho about the line of edge e, w = o - (the edge's first vertex): the sweep and the origin are
// projected across the edge (wp, dp: one rounding of |w|, |d| per component, so a nearly parallel sweep keeps a
// leading coefficient dp.dp with a small RELATIVE error), the root is taken there.
__device__ __forceinline__ double sweep_edge(const SweepRay &r, V3d w, V3d e) {
  const double ee = dot(e, e);
  if (!(ee > 0.0)) return kNoSweep;
  const double ie = pq_div(1.0, ee);
  const double we = dot(w, e), de = dot(r.d, e);
  const V3d wp = w - e * (we * ie), dp = r.d - e * (de * ie);
  const double A = dot(dp, dp), h = dot(wp, dp);
  if (!(A > 0.0 && h < 0.0)) return kNoSweep;
  const double t = sweep_root<false>(wp, dp, h, pq_div(1.0, A), r.rho);
  const double ax = we + de * t;  // the axial parameter at contact, times e.e
  return (ax >= 0.0 && ax <= ee) ? t : kNoSweep;
}

template <bool SERIAL>
__device__ __forceinline__ double sweep_triangle(const SweepRay &r, V3d a, V3d e1, V3d e2, V3d n, bool &ov) {
  V3d q;
  ov = point_triangle<false, SERIAL>(r.o, a, e1, e2, n, q) <= r.rho;
  if (ov) return 0.0;
  const V3d w = r.o - a;
  double best = kNoSweep;
  candidate_fence<SERIAL>();
  const double nn = dot(n, n);
  if (nn > 0.0) {  // the face
    const double wn = dot(n, w), dn = dot(n, r.d);
    const double num = fabs(wn) - r.rho * pq_sqrt(nn);
    if (wn > 0.0 ? dn < 0.0 : dn > 0.0) {  // (a start within the slab reaches its offset plane at once)
      const double t = pq_div(num <= 0.0 ? 0.0 : num, fabs(dn));
      const V3d p = w + r.d * t;
      const double d1 = dot(p, e1), d2 = dot(p, e2);
      const double ee1 = dot(e1, e1), ee2 = dot(e2, e2), e12 = dot(e1, e2);
      const double sn = ee2 * d1 - e12 * d2, tn = ee1 * d2 - e12 * d1;
      if (sn >= 0.0 && tn >= 0.0 && sn + tn <= nn && t < kNoSweep) best = t;
    }
  }
  candidate_fence<SERIAL>();
  best = fmin(best, sweep_edge(r, w, e1));
  candidate_fence<SERIAL>();
  best = fmin(best, sweep_edge(r, w, e2));
  candidate_fence<SERIAL>();
  best = fmin(best, sweep_vertex(r, w));
  candidate_fence<SERIAL>();
  const V3d g = w - e1;
  best = fmin(best, sweep_edge(r, g, e2 - e1));
  candidate_fence<SERIAL>();
  best = fmin(best, sweep_vertex(r, g));
  candidate_fence<SERIAL>();
  best = fmin(best, sweep_vertex(r, w - e2));
  return best;
}

// ---- the sink: the best (t, insertion index) so far; its t is the walks' bound ----
struct SweepBest {
  double t;  // t of the best primitive so far (tmax before any)
  int prim;  // walk-order id, -1 = none
  bool ov;   // the best primitive's start-overlap flag
  // Accepted when t <= the bound (inclusive), a tie going to the lower insertion index (map: walk id -> insertion index).
  __device__ __forceinline__ void take(double tt, bool o, int id, const int32_t *map) {
    if (!(tt <= t && tt < kNoSweep)) return;
    if (tt == t && prim >= 0 && !(map[id] < map[prim])) return;
    t = tt;
    prim = id;
    ov = o;
  }
  __device__ __forceinline__ double bound() const { return t; }
};

// ---- the primitives of a BVH image, and of the class record arrays (point_image_prim / point_class_prim) ----
template <bool LDS, bool SERIAL>
__device__ __forceinline__ double sweep_image_prim(const Image<LDS> &im, const DevScene &sc, int id, const SweepRay &ray,
                                                   bool &ov) {
  if (id < sc.n_sph) {
    const uint32_t r = sc.off_sph + 32u * (uint32_t)id;
    const double2 p0 = im.d2(r), p1 = im.d2(r + 16u);
    return sweep_sphere(ray, p0.x, p0.y, p1.x, p1.y, ov);
  } else if (id < sc.n_sph + sc.n_mov) {
    const uint32_t r = sc.off_mov + 64u * (uint32_t)(id - sc.n_sph);
    const double2 p0 = im.d2(r), p1 = im.d2(r + 16u), p2 = im.d2(r + 32u), p3 = im.d2(r + 48u);
    return sweep_sphere(ray, p0.x + ray.time * p1.y, p0.y + ray.time * p2.x, p1.x + ray.time * p2.y, p3.x, ov);
  }
  const uint32_t r = sc.off_tri + 96u * (uint32_t)(id - sc.n_sph - sc.n_mov);
  const double2 q0 = im.d2(r), q1 = im.d2(r + 16u), q2 = im.d2(r + 32u), q3 = im.d2(r + 48u), q4 = im.d2(r + 64u),
                q5 = im.d2(r + 80u);
  return sweep_triangle<SERIAL>(ray, V3d{q0.x, q0.y, q1.x}, V3d{q1.y, q2.x, q2.y}, V3d{q3.x, q3.y, q4.x},
                                V3d{q4.y, q5.x, q5.y}, ov);
}

// ---- BRUTE: every primitive from the class record arrays (wave-uniform loop: scalar loads) ----
__device__ __forceinline__ void sweep_brute(const DevScene &sc, const SweepRay &ray, bool active, const int32_t *map,
                                            SweepBest &best, uint32_t &nprim) {
  bool ov;
  {
    cdptr g = (cdptr)sc.sph;
    for (int k = 0; k < sc.n_sph; ++k)
      if (active) {
        const double t = sweep_sphere(ray, g[4 * k + 0], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3], ov);
        best.take(t, ov, k, map);
      }
  }
  {
    cdptr g = (cdptr)sc.mov;
    for (int k = 0; k < sc.n_mov; ++k)
      if (active) {
        const double t = sweep_sphere(ray, g[8 * k + 0] + ray.time * g[8 * k + 3], g[8 * k + 1] + ray.time * g[8 * k + 4],
                                      g[8 * k + 2] + ray.time * g[8 * k + 5], g[8 * k + 6], ov);
        best.take(t, ov, sc.n_sph + k, map);
      }
  }
  {
    cdptr g = (cdptr)sc.tri;
    const int base = sc.n_sph + sc.n_mov;
    for (int k = 0; k < sc.n_tri; ++k)
      if (active) {
        const double t = sweep_triangle<true>(ray, V3d{g[12 * k + 0], g[12 * k + 1], g[12 * k + 2]},
                                              V3d{g[12 * k + 3], g[12 * k + 4], g[12 * k + 5]},
                                              V3d{g[12 * k + 6], g[12 * k + 7], g[12 * k + 8]},
                                              V3d{g[12 * k + 9], g[12 * k + 10], g[12 * k + 11]}, ov);
        best.take(t, ov, base + k, map);
      }
  }
  if (active) nprim += (uint32_t)(sc.n_sph + sc.n_mov + sc.n_tri);
}

// ---- the slab test on an inflated box (binary64) ----
// o, 1 / d per axis (+-inf for a zero component) and pad = rho + sigma.  Entry t of [lo - pad, hi + pad], clamped to
// [0, bound]; +inf on a miss.  A NaN (0 * inf: the origin exactly on an inflated plane of an axis the sweep does not
// move along) drops out of fmin / fmax on the side that may reject the box: the origin is then sigma outside the box
// grown by rho, where no primitive of the box can be touched.
struct SweepSlab {
  V3d o, inv;
  double pad;
};
__device__ __forceinline__ SweepSlab sweep_slab(const SweepRay &r, double mag) {
  const double sigma = 0x1p-40 * (((fabs(r.o.x) + fabs(r.o.y) + fabs(r.o.z)) + mag) + r.rho);
  return {r.o, V3d{1.0 / r.d.x, 1.0 / r.d.y, 1.0 / r.d.z}, r.rho + sigma};
}
__device__ __forceinline__ double slab_entry(const SweepSlab &s, double lx, double ly, double lz, double hx, double hy,
                                             double hz, double bound) {
  const double ax = ((lx - s.pad) - s.o.x) * s.inv.x, bx = ((hx + s.pad) - s.o.x) * s.inv.x;
  const double ay = ((ly - s.pad) - s.o.y) * s.inv.y, by = ((hy + s.pad) - s.o.y) * s.inv.y;
  const double az = ((lz - s.pad) - s.o.z) * s.inv.z, bz = ((hz + s.pad) - s.o.z) * s.inv.z;
  const double tn = fmax(fmax(fmin(ax, bx), fmin(ay, by)), fmax(fmin(az, bz), 0.0));
  const double tf = fmin(fmin(fmax(ax, bx), fmax(ay, by)), fmin(fmax(az, bz), bound));
  return (tn <= tf && tn < kNoSweep) ? tn : kNoSweep;
}

// ---- BVH: the threaded walk and leaf queue of bounded_walk_bvh (rtow_bounded_walks.h) on inflated boxes ----
template <bool LDS>
__device__ __forceinline__ void sweep_bvh(const Image<LDS> &im, const DevScene &sc, const SweepRay &ray, bool active,
                                          const int32_t *map, SweepBest &best, uint32_t &nnode, uint32_t &nprim) {
  const uint32_t END = (uint32_t)sc.n_nodes;
  SweepSlab slab = sweep_slab(ray, 0.0);
  if (active) {  // the root box bounds every primitive: its magnitude scales the slack
    const float4 r0 = im.f4(0u), r1 = im.f4(16u);
    slab = sweep_slab(ray, box_mag(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y));
  }
  double lim = best.bound();
  int last_id = -1;
  uint32_t node = active ? 0u : END;
  uint32_t q0 = 0u, q1 = 0u, q2 = 0u, q3 = 0u;  // queued leaves (0 = empty), oldest first
  for (;;) {
    if (node < END) {
      const float4 r0 = im.f4(node * 32u), r1 = im.f4(node * 32u + 16u);
      ++nnode;
      const bool hit = slab_entry(slab, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, lim) < kNoSweep;
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
        const uint32_t first = q0 >> 3, count = q0 & 7u;
        for (uint32_t k = 0; k < count; ++k) {
          const int id = sc.leaf_direct ? (int)(first + k) : (int)im.u32(sc.off_ids + 4u * (first + k));
          if (id == last_id) continue;
          last_id = id;
          ++nprim;
          bool ov;
          const double t = sweep_image_prim<LDS, true>(im, sc, id, ray, ov);
          best.take(t, ov, id, map);
        }
      }
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = 0u;
      lim = best.bound();
      if (!any_walking && !__any(q0 != 0u)) break;
    }
  }
}

// ---- BVH4: nearest child first by entry t, the per-lane stack and spill of the 4-wide walks (closest_bvh4) ----
// A stack entry carries 11 bits of its box's entry t, rounded down (sq_key_down on t >= 0); a popped entry beyond the
// bound (rounded up) is dropped.
__device__ __forceinline__ uint32_t sweep_key(double tn) {
  return __float_as_uint((float)tn * 0.99999988f) & 0x7fffffffu;  // (t >= 0: the mask only clears the sign of a -0)
}
template <bool FULL>
__device__ __forceinline__ void sweep_bvh4(const Bvh4Reader<FULL> &im, const DevScene &sc, const TraceParams &P,
                                           const SweepRay &ray, bool active, uint32_t lane_g, const int32_t *map,
                                           SweepBest &best, uint32_t &nnode, uint32_t &nprim) {
  const Bvh4Stack st = bvh4_stack(sc);
  SweepSlab slab = sweep_slab(ray, 0.0);
  if (active) {  // the root's children bound every primitive
    double pl[6][4];
    vu4 cw;
    bvh4_node<FULL>(im, sc, 0u, pl, cw);
    const uint32_t c[4] = {cw.x, cw.y, cw.z, cw.w};
    double mag = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c[j] != kRefNone) mag = fmax(mag, box_mag(pl[0][j], pl[2][j], pl[4][j], pl[1][j], pl[3][j], pl[5][j]));
    slab = sweep_slab(ray, mag);
  }
  double lim = best.bound();
  uint32_t klim = sq_key_up(lim);
  uint32_t sa = st.lds;
  uint32_t cur = active ? 0u : kRefNone;  // node 0 = root
  uint32_t q0 = kRefNone, q1 = kRefNone;  // queued leaves, oldest first
  for (;;) {
    // (1) a leaf reached by the walk waits in the queue for the next leaf phase
    if ((cur & kRefLeaf) != 0u && cur < kRefPop && q1 == kRefNone) {
      if (q0 == kRefNone)
        q0 = cur;
      else
        q1 = cur;
      cur = kRefPop;
    }
    // (2) next entry from the stack; an entry whose box is entered beyond the bound is dropped
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
    // (3) one node: four slab tests, the child entered first next, the others to the stack
    if (cur < kRefLeaf) {
      double pl[6][4];
      vu4 cw;
      bvh4_node<FULL>(im, sc, cur, pl, cw);
      ++nnode;
      const uint32_t c[4] = {cw.x, cw.y, cw.z, cw.w};
      uint32_t k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double tn = slab_entry(slab, pl[0][j], pl[2][j], pl[4][j], pl[1][j], pl[3][j], pl[5][j], lim);
        const bool h = c[j] != kRefNone && tn < kNoSweep;
        k[j] = h ? ((sweep_key(tn) & ~3u) | (uint32_t)j) : 0xffffffffu;
      }
      const uint32_t kmin = min(min(k[0], k[1]), min(k[2], k[3]));
      const uint32_t s = kmin & 3u;
      cur = kmin == 0xffffffffu ? kRefPop : c[s];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k[j] != 0xffffffffu && (uint32_t)j != s) {
          const uint32_t e = ((k[j] >> 20) << 21) | c[j];
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
          bool ov;
          const double t = sweep_triangle<true>(ray, V3d{t0.x, t0.y, t1.x}, V3d{t1.y, t2.x, t2.y}, V3d{t3.x, t3.y, t4.x},
                                                V3d{t4.y, t5.x, t5.y}, ov);
          best.take(t, ov, (int)(first + j), map);
        }
      }
      q0 = q1;
      q1 = kRefNone;
      lim = best.bound();
      klim = sq_key_up(lim);
      if (!any_walking && !__any(q0 != kRefNone)) break;
    }
  }
}

// ---- a query, and its record ----
// {ox, oy} {oz, time} {dx, dy} {dz, tmax} {radius, pad}: five 16-byte loads
__device__ __forceinline__ void load_sweep(const unsigned char *queries, uint32_t i, SweepRay &r, double &tmax) {
  const vd2 *p = reinterpret_cast<const vd2 *>(queries + (size_t)i * kSweepBytes);
  const vd2 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3], r4 = p[4];
  r.o = {r0.x, r0.y, r1.x};
  r.time = r1.y;
  r.d = {r2.x, r2.y, r3.x};
  tmax = r3.y;
  r.rho = r4.x;
}
// One 80-byte rtow_sweep_hit_t: five 16-byte stores
__device__ __forceinline__ void store_sweep_hit(unsigned char *dst, double t, double dist, V3d c, V3d q, int32_t prim,
                                                int32_t kind, int32_t mi, int32_t ov) {
  vd2 *h = reinterpret_cast<vd2 *>(dst);
  h[0] = vd2{t, dist};
  h[1] = vd2{c.x, c.y};
  h[2] = vd2{c.z, q.x};
  h[3] = vd2{q.y, q.z};
  reinterpret_cast<int4 *>(h + 4)[0] = make_int4(prim, kind, mi, ov);
}
