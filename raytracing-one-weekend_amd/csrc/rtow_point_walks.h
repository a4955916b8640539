// rtow_point_walks.h — the per-primitive distance formulas and the three pruned point walks, written once for the two
// point queries: closest point (rtow_pointq.h, sink PBest: one entry) and k nearest (rtow_nearest.h, sink NearestSink:
// a sorted list of k).  Included inside namespace rtow { namespace { ... } } after the trace headers.
//
// A SINK is what a walk hands every tested primitive to, and what tells it how far to look:
//   void take(double d, int id)   the computed distance of walk id `id` (tested once per visit);
//   double bound() const          the search radius: no primitive farther than this can enter the answer any more.
//                                 It starts at the query's max_dist and only shrinks; a primitive AT the bound may
//                                 still enter (inclusive), so the walks visit every member of a tie at the bound.
//   static constexpr bool kSerial  the sink needs the registers: the tree walks evaluate a triangle's four candidates
//                                 one after the other (point_triangle<Q, SERIAL>).  The values are the same either way.
// The walks read bound() where they recompute their pruning terms: after every leaf phase.
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
//   * BVH (2): the threaded binary walk; a box whose lower bound cannot beat the sink's bound takes `skip`;
//   * BVH4 (4): nearest child first by box distance with the per-lane LDS stack (and spill) of the 4-wide ray walk; an
//     entry carries 11 bits of its box's squared distance, rounded down, and a popped entry beyond the bound is dropped.
// Pruning is conservative with respect to the per-primitive distance computed here: the box bound is
// evaluated in binary64 from the binary32 / binary16 planes (decoded c + h * is), compared against
// (bound + sigma)^2 with sigma = 2^-40 (|p|_1 + M), M the root box's magnitude — above every rounding of a primitive's
// computed distance for any finite p.

constexpr uint32_t kPQueryBytes = 48u, kPHitBytes = 48u;  // rtow_point_query_t, rtow_point_hit_t (include/rtow.h)

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

// SERIAL: the four candidates are evaluated one after the other (a scheduling barrier between them) instead of
// interleaved: the same operations and values with fewer registers live, for a sink that needs them.
template <bool SERIAL>
__device__ __forceinline__ void candidate_fence() {
  if constexpr (SERIAL) __builtin_amdgcn_sched_barrier(0);
}
template <bool Q, bool SERIAL = false>
__device__ __forceinline__ double point_triangle(V3d p, V3d a, V3d e1, V3d e2, V3d n, V3d &q) {
  // (the statements are ordered so that as little as possible is live at each candidate: a and n die first, the plane
  // candidate is evaluated before the third edge — whose f and g replace w, e1 and e2 — and compared after it)
  const V3d w = p - a;
  const double nn = dot(n, n);
  candidate_fence<SERIAL>();
  const double d1 = dot(w, e1), ee1 = dot(e1, e1);
  const double s1 = ee1 > 0.0 ? clamp01(pq_div(d1, ee1)) : 0.0;
  const V3d r1 = w - e1 * s1;
  double best = dot(r1, r1);
  int which = 0;
  candidate_fence<SERIAL>();
  const double d2 = dot(w, e2), ee2 = dot(e2, e2);
  const double t2 = ee2 > 0.0 ? clamp01(pq_div(d2, ee2)) : 0.0;
  const V3d r2 = w - e2 * t2;
  const double b2 = dot(r2, r2);
  if (b2 < best) best = b2, which = 1;
  candidate_fence<SERIAL>();
  const double e12 = dot(e1, e2);
  const double sn = ee2 * d1 - e12 * d2, tn = ee1 * d2 - e12 * d1;
  double s = 0.0, t = 0.0, b0 = __builtin_huge_val();  // (+inf: never below best)
  if (nn > 0.0 && sn >= 0.0 && tn >= 0.0 && sn + tn <= nn) {
    s = pq_div(sn, nn);
    t = pq_div(tn, nn);
    const V3d r0 = (w - e1 * s) - e2 * t;
    b0 = dot(r0, r0);
  }
  candidate_fence<SERIAL>();
  const V3d f = e2 - e1, g = w - e1;
  const double ff = dot(f, f), dg = dot(g, f);
  const double u3 = ff > 0.0 ? clamp01(pq_div(dg, ff)) : 0.0;
  const V3d r3 = g - f * u3;
  const double b3 = dot(r3, r3);
  if (b3 < best) best = b3, which = 2;
  if (b0 < best) best = b0, which = 3;
  if constexpr (Q) {
    q = which == 0   ? a + e1 * s1
        : which == 1 ? a + e2 * t2
        : which == 2 ? (a + e1) + f * u3
                     : (a + e1 * s) + e2 * t;
  }
  return pq_sqrt(best);
}

// The squared search radius a box must exceed to be pruned: (bound + sigma)^2.
__device__ __forceinline__ double prune_sq(double bound, double sigma) {
  const double r = bound + sigma;
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
template <bool LDS, bool Q, bool SERIAL = false>
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
  return point_triangle<Q, SERIAL>(p, V3d{q0.x, q0.y, q1.x}, V3d{q1.y, q2.x, q2.y}, V3d{q3.x, q3.y, q4.x},
                                   V3d{q4.y, q5.x, q5.y}, q);
}

// ---- BRUTE: every primitive from the class record arrays (wave-uniform loop: scalar loads) ----
template <bool Q, bool SERIAL = false>
__device__ __forceinline__ double point_class_prim(const DevScene &sc, int id, V3d p, double time, V3d &q) {
  if (id < sc.n_sph) {
    const double *g = sc.sph + 4 * (size_t)id;
    return point_sphere<Q>(p, g[0], g[1], g[2], g[3], q);
  } else if (id < sc.n_sph + sc.n_mov) {
    const double *g = sc.mov + 8 * (size_t)(id - sc.n_sph);
    return point_sphere<Q>(p, g[0] + time * g[3], g[1] + time * g[4], g[2] + time * g[5], g[6], q);
  }
  const double *g = sc.tri + 12 * (size_t)(id - sc.n_sph - sc.n_mov);
  return point_triangle<Q, SERIAL>(p, V3d{g[0], g[1], g[2]}, V3d{g[3], g[4], g[5]}, V3d{g[6], g[7], g[8]},
                                   V3d{g[9], g[10], g[11]}, q);
}

template <class Sink>
__device__ __forceinline__ void closest_brute(const DevScene &sc, V3d p, double time, bool active, Sink &best,
                                              uint32_t &nprim) {
  V3d q;
  {
    cdptr g = (cdptr)sc.sph;
    for (int k = 0; k < sc.n_sph; ++k)
      if (active) best.take(point_sphere<false>(p, g[4 * k + 0], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3], q), k);
  }
  {
    cdptr g = (cdptr)sc.mov;
    for (int k = 0; k < sc.n_mov; ++k)
      if (active)
        best.take(point_sphere<false>(p, g[8 * k + 0] + time * g[8 * k + 3], g[8 * k + 1] + time * g[8 * k + 4],
                                      g[8 * k + 2] + time * g[8 * k + 5], g[8 * k + 6], q),
                  sc.n_sph + k);
  }
  {
    cdptr g = (cdptr)sc.tri;
    const int base = sc.n_sph + sc.n_mov;
    for (int k = 0; k < sc.n_tri; ++k)
      if (active)
        best.take(point_triangle<false>(p, V3d{g[12 * k + 0], g[12 * k + 1], g[12 * k + 2]},
                                        V3d{g[12 * k + 3], g[12 * k + 4], g[12 * k + 5]},
                                        V3d{g[12 * k + 6], g[12 * k + 7], g[12 * k + 8]},
                                        V3d{g[12 * k + 9], g[12 * k + 10], g[12 * k + 11]}, q),
                  base + k);
  }
  if (active) nprim += (uint32_t)(sc.n_sph + sc.n_mov + sc.n_tri);
}

// ---- BVH: the threaded walk of closest_hit_bvh (rtow_trace_bvh.h) with box distances instead of slabs ----
template <bool LDS, class Sink>
__device__ __forceinline__ void closest_bvh(const Image<LDS> &im, const DevScene &sc, V3d p, double time, bool active,
                                            Sink &best, uint32_t &nnode, uint32_t &nprim) {
  const uint32_t END = (uint32_t)sc.n_nodes;
  double sigma = 0.0;
  if (active) {  // the root box bounds every primitive: its magnitude scales the slack
    const float4 r0 = im.f4(0u), r1 = im.f4(16u);
    sigma = pq_sigma(p, box_mag(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y));
  }
  double lim = prune_sq(best.bound(), sigma);
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
          best.take(point_image_prim<LDS, false, Sink::kSerial>(im, sc, id, p, time, q), id);
        }
      }
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = 0u;
      lim = prune_sq(best.bound(), sigma);
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

template <bool FULL, class Sink>
__device__ __forceinline__ void closest_bvh4(const Bvh4Reader<FULL> &im, const DevScene &sc, const TraceParams &P, V3d p,
                                             bool active, uint32_t lane_g, Sink &best, uint32_t &nnode,
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
  double lim = prune_sq(best.bound(), sigma);
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
          best.take(point_triangle<false, Sink::kSerial>(p, V3d{t0.x, t0.y, t1.x}, V3d{t1.y, t2.x, t2.y},
                                                         V3d{t3.x, t3.y, t4.x}, V3d{t4.y, t5.x, t5.y}, q),
                    (int)(first + j));
        }
      }
      q0 = q1;
      q1 = kRefNone;
      lim = prune_sq(best.bound(), sigma);
      klim = sq_key_up(lim);
      if (!any_walking && !__any(q0 != kRefNone)) break;
    }
  }
}

// ---- a query, and the record of one answered primitive ----
// {px, py} {pz, time} {max_dist, pad}: three 16-byte loads
__device__ __forceinline__ void load_point_query(const unsigned char *queries, uint32_t i, V3d &p, double &time,
                                                 double &max_dist) {
  const vd2 *r = reinterpret_cast<const vd2 *>(queries + (size_t)i * kPQueryBytes);
  const vd2 r0 = r[0], r1 = r[1], r2 = r[2];
  p = {r0.x, r0.y, r1.x};
  time = r1.y;
  max_dist = r2.x;
}
// The fields of walk id `pid` under KERNEL's image: its distance and point recomputed by the same formulas, kind, material.
template <int KERNEL, bool LDS, bool SERIAL = false>
__device__ __forceinline__ double point_record(const Image<LDS> &im, const Bvh4Reader<LDS> &im4, const DevScene &sc, int pid,
                                               V3d p, double time, V3d &q, int32_t &kind, int32_t &mi) {
  if constexpr (KERNEL == 4) {
    const uint32_t r = sc.b4_off_tri + 96u * (uint32_t)pid;
    const vd2 t0 = im4.t2(r), t1 = im4.t2(r + 16u), t2 = im4.t2(r + 32u), t3 = im4.t2(r + 48u), t4 = im4.t2(r + 64u),
              t5 = im4.t2(r + 80u);
    const double dist = point_triangle<true, SERIAL>(p, V3d{t0.x, t0.y, t1.x}, V3d{t1.y, t2.x, t2.y},
                                                     V3d{t3.x, t3.y, t4.x}, V3d{t4.y, t5.x, t5.y}, q);
    kind = 2;  // (a 4-wide image is a triangle mesh)
    mi = (int)im4.u32(sc.b4_off_pmat + 4u * (uint32_t)pid);
    return dist;
  } else {
    kind = pid < sc.n_sph ? 0 : (pid < sc.n_sph + sc.n_mov ? 1 : 2);
    if constexpr (KERNEL == 2) {
      const double dist = point_image_prim<LDS, true, SERIAL>(im, sc, pid, p, time, q);
      mi = (int)im.u32(sc.off_pmat + 4u * (uint32_t)pid);
      return dist;
    } else {
      const double dist = point_class_prim<true, SERIAL>(sc, pid, p, time, q);
      mi = sc.prim_mat[pid];
      return dist;
    }
  }
}
// One 48-byte rtow_point_hit_t: three 16-byte stores
__device__ __forceinline__ void store_point_hit(unsigned char *dst, double dist, V3d q, int32_t prim, int32_t kind,
                                                int32_t mi) {
  vd2 *h = reinterpret_cast<vd2 *>(dst);
  h[0] = vd2{dist, q.x};
  h[1] = vd2{q.y, q.z};
  reinterpret_cast<int4 *>(h + 2)[0] = make_int4(prim, kind, mi, 0);
}
