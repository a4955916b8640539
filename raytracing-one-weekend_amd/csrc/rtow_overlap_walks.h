// rtow_overlap_walks.h — the box-overlap predicates and the three walks of the overlap query (rtow_overlap.h).  Included
// inside namespace rtow { namespace { ... } } after rtow_point_walks.h, whose node reader (bvh4_node), box magnitude and
// slack (box_mag, pq_sigma) it uses.
//
// Predicates (written once, in a fixed operation order: the strict build compiles them with -ffp-contract=off and
// tests/overlap_ref.py mirrors them bit for bit; no division, square root or reciprocal; every comparison inclusive —
// an axis separates only when a gap is > 0).  They work on the inputs as given, lo and hi and the record's fields, not
// on a box centre: every monomial of a gap is then rounded a counted number of times and nothing else enters the error,
// which is what the band of include/rtow.h is stated in (a centre would bring |hi| into a gap that only lo bounds).
//   * overlap_sphere (fixed and moving spheres: the SURFACE, centre s, radius^2 = |r2|), per component
//     near = max(max(lo - s, s - hi), 0) and far = max(s - lo, hi - s); dmin^2 = (near.x^2 + near.y^2) + near.z^2 (to the
//     box), dmax^2 = (far.x^2 + far.y^2) + far.z^2 (to its farthest corner); overlap iff dmin^2 <= |r2| and |r2| <= dmax^2.
//   * overlap_triangle (a, e1, e2 and the stored n = e1 x e2): v0 = a, v1 = a + e1, v2 = a + e2, f = e2 - e1, and the
//     thirteen separating axes of a triangle and a box:
//       the three box normals: min(v0, v1, v2) > hi or max(v0, v1, v2) < lo, per component;
//       an axis L otherwise: the box projects onto [sum_k min(L_k lo_k, L_k hi_k), sum_k max(L_k lo_k, L_k hi_k)] (summed
//       x, y, z; a zero component adds nothing), the triangle onto the span of its projections, and L separates when the
//       triangle's least projection is above the box's greatest or its greatest below the box's least;
//       the stored normal: the triangle's one projection (n.x a.x + n.y a.y) + n.z a.z (n = 0, a zero-area triangle:
//         0 against [0, 0], no axis);
//       edge x box axis, for the edges e1 (vertices v0, v2: v1 projects where v0 does), e2 (v0, v1) and f (v0, v1): with g
//         the edge, X x g: p(v) = v.z g.y - v.y g.z; Y x g: p(v) = v.x g.z - v.z g.x; Z x g: p(v) = v.y g.x - v.x g.y, the
//         box's ends the same differences of the greater and the lesser products.  The axis components are copies of the
//         edge's: nothing is rounded but f.
//     A zero-area triangle is its segment or point: the box normals and the nine cross axes are the complete axis set of
//     a segment and a box.
//
// Walks: BRUTE reads every record of the class arrays with scalar loads; BVH is the threaded walk with the leaf queue of
// closest_bvh; BVH4 the per-lane LDS stack with spill of closest_bvh4, children taken in slot order (there is no bound
// to shrink, so no order is better than another).  A node is entered iff per axis node.lo <= hi + sigma and
// node.hi >= lo - sigma (inclusive), sigma = pq_sigma(max(|lo|, |hi|), root magnitude) = 2^-40 (|box|_1 + M).
// Pruning is conservative with respect to the computed predicate: a reported primitive passed the
// predicate's own bounding-box test (the box-normal axes on the very sums a + e1, a + e2 the builders bound; for a sphere
// dmin^2 <= |r2|), and the node planes bound those vertices (sphere: centre -+ radius over the shutter) with a pad of
// 1e-9 and outward rounding; sigma covers the sphere test's few roundings a million times over.
//
// Every image holds every primitive in exactly one leaf (both builders; the refit keeps the topology), so a walk meets a
// primitive once and the count needs no list of what was seen; the binary walk keeps its one-entry mailbox all the same.

constexpr uint32_t kBoxQueryBytes = 64u;  // rtow_box_query_t (include/rtow.h)

struct OvBox {
  V3d lo, hi;
  double time;  // moving spheres: centre c0 + time (c1 - c0)
};

// ---- predicates ----
__device__ __forceinline__ bool overlap_sphere(const OvBox &b, double sx, double sy, double sz, double r2) {
  const double nx = fmax(fmax(b.lo.x - sx, sx - b.hi.x), 0.0), fx = fmax(sx - b.lo.x, b.hi.x - sx);
  const double ny = fmax(fmax(b.lo.y - sy, sy - b.hi.y), 0.0), fy = fmax(sy - b.lo.y, b.hi.y - sy);
  const double nz = fmax(fmax(b.lo.z - sz, sz - b.hi.z), 0.0), fz = fmax(sz - b.lo.z, b.hi.z - sz);
  const double dmin2 = (nx * nx + ny * ny) + nz * nz;
  const double dmax2 = (fx * fx + fy * fy) + fz * fz;
  const double R2 = fabs(r2);
  return dmin2 <= R2 && R2 <= dmax2;
}

// One cross axis: the triangle's two distinct projections p, q against the box's interval.  The axis has the components
// (+gp along axis P, -gm along axis M): the box's ends are differences of the greater and the lesser products.
__device__ __forceinline__ bool ov_separated(double p, double q, double gp, double lo_p, double hi_p, double gm, double lo_m,
                                             double hi_m) {
  const double a0 = gp * lo_p, a1 = gp * hi_p, b0 = gm * lo_m, b1 = gm * hi_m;
  const double bmax = fmax(a0, a1) - fmin(b0, b1), bmin = fmin(a0, a1) - fmax(b0, b1);
  return fmin(p, q) > bmax || fmax(p, q) < bmin;
}
// the three axes X x g, Y x g, Z x g for edge g and the two vertices u, w that project apart
__device__ __forceinline__ bool ov_edge_axes(const OvBox &b, V3d g, V3d u, V3d w) {
  bool sep = ov_separated(u.z * g.y - u.y * g.z, w.z * g.y - w.y * g.z, g.y, b.lo.z, b.hi.z, g.z, b.lo.y, b.hi.y);
  sep |= ov_separated(u.x * g.z - u.z * g.x, w.x * g.z - w.z * g.x, g.z, b.lo.x, b.hi.x, g.x, b.lo.z, b.hi.z);
  sep |= ov_separated(u.y * g.x - u.x * g.y, w.y * g.x - w.x * g.y, g.x, b.lo.y, b.hi.y, g.y, b.lo.x, b.hi.x);
  return sep;
}
__device__ __forceinline__ bool overlap_triangle(const OvBox &b, V3d a, V3d e1, V3d e2, V3d n) {
  const V3d v1 = {a.x + e1.x, a.y + e1.y, a.z + e1.z};
  const V3d v2 = {a.x + e2.x, a.y + e2.y, a.z + e2.z};
  bool sep = fmin(fmin(a.x, v1.x), v2.x) > b.hi.x || fmax(fmax(a.x, v1.x), v2.x) < b.lo.x;
  sep |= fmin(fmin(a.y, v1.y), v2.y) > b.hi.y || fmax(fmax(a.y, v1.y), v2.y) < b.lo.y;
  sep |= fmin(fmin(a.z, v1.z), v2.z) > b.hi.z || fmax(fmax(a.z, v1.z), v2.z) < b.lo.z;
  const double d = (n.x * a.x + n.y * a.y) + n.z * a.z;
  const double x0 = n.x * b.lo.x, x1 = n.x * b.hi.x, y0 = n.y * b.lo.y, y1 = n.y * b.hi.y, z0 = n.z * b.lo.z,
               z1 = n.z * b.hi.z;
  const double bmax = (fmax(x0, x1) + fmax(y0, y1)) + fmax(z0, z1);
  const double bmin = (fmin(x0, x1) + fmin(y0, y1)) + fmin(z0, z1);
  sep |= d > bmax || d < bmin;
  const V3d f = {e2.x - e1.x, e2.y - e1.y, e2.z - e1.z};
  sep |= ov_edge_axes(b, e1, a, v2);
  sep |= ov_edge_axes(b, e2, a, v1);
  sep |= ov_edge_axes(b, f, a, v1);
  return !sep;
}

// ---- the sink: the count and, when ids are asked for, the eight lowest insertion indices, ascending ----
// Eight named slots (registers; rtow_sorted_list.h says why not an array); an empty slot holds INT32_MAX.
#define RTOW_OV_SLOTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
struct OverlapSink {
  int32_t count;
  int32_t s0, s1, s2, s3, s4, s5, s6, s7;
  int32_t min_prim;    // (already max(min_prim, 0))
  bool keep;           // ids are asked for (wave-uniform)
  const int32_t *map;  // walk's primitive id -> insertion index
  __device__ __forceinline__ void clear() {
    count = 0;
#define RTOW_OV_X(j) s##j = 0x7fffffff;
    RTOW_OV_SLOTS(RTOW_OV_X)
#undef RTOW_OV_X
  }
  // min_prim, before the primitive's test: the map is read only when some primitive can fail it
  __device__ __forceinline__ bool takes_part(int id) const { return min_prim <= 0 || map[id] >= min_prim; }
  // a primitive that overlaps
  __device__ __forceinline__ void take(int id) {
    ++count;
    if (keep) {
      const int32_t v = map[id];
#define RTOW_OV_SHIFT(j, jm) s##j = v < s##jm ? s##jm : (v < s##j ? v : s##j);
      RTOW_OV_SHIFT(7, 6)
      RTOW_OV_SHIFT(6, 5)
      RTOW_OV_SHIFT(5, 4)
      RTOW_OV_SHIFT(4, 3)
      RTOW_OV_SHIFT(3, 2)
      RTOW_OV_SHIFT(2, 1)
      RTOW_OV_SHIFT(1, 0)
#undef RTOW_OV_SHIFT
      s0 = v < s0 ? v : s0;
    }
  }
  // slot j (wave-uniform j), -1 for an empty one
  __device__ __forceinline__ int32_t entry(int j) const {
    int32_t v = s7;
#define RTOW_OV_X(k) if (j == k) v = s##k;
    RTOW_OV_SLOTS(RTOW_OV_X)
#undef RTOW_OV_X
    return v == 0x7fffffff ? -1 : v;
  }
};

// ---- the primitives of a BVH image (class by id range, as point_image_prim) ----
template <bool LDS>
__device__ __forceinline__ bool overlap_image_prim(const Image<LDS> &im, const DevScene &sc, int id, const OvBox &b) {
  if (id < sc.n_sph) {
    const uint32_t r = sc.off_sph + 32u * (uint32_t)id;
    const double2 p0 = im.d2(r), p1 = im.d2(r + 16u);
    return overlap_sphere(b, p0.x, p0.y, p1.x, p1.y);
  } else if (id < sc.n_sph + sc.n_mov) {
    const uint32_t r = sc.off_mov + 64u * (uint32_t)(id - sc.n_sph);
    const double2 p0 = im.d2(r), p1 = im.d2(r + 16u), p2 = im.d2(r + 32u), p3 = im.d2(r + 48u);
    return overlap_sphere(b, p0.x + b.time * p1.y, p0.y + b.time * p2.x, p1.x + b.time * p2.y, p3.x);
  }
  const uint32_t r = sc.off_tri + 96u * (uint32_t)(id - sc.n_sph - sc.n_mov);
  const double2 q0 = im.d2(r), q1 = im.d2(r + 16u), q2 = im.d2(r + 32u), q3 = im.d2(r + 48u), q4 = im.d2(r + 64u),
                q5 = im.d2(r + 80u);
  return overlap_triangle(b, V3d{q0.x, q0.y, q1.x}, V3d{q1.y, q2.x, q2.y}, V3d{q3.x, q3.y, q4.x}, V3d{q4.y, q5.x, q5.y});
}

// ---- BRUTE: every primitive from the class record arrays (wave-uniform loop: scalar loads) ----
__device__ __forceinline__ void overlap_brute(const DevScene &sc, const OvBox &b, bool active, OverlapSink &out,
                                              uint32_t &nprim) {
  {
    cdptr g = (cdptr)sc.sph;
    for (int k = 0; k < sc.n_sph; ++k)
      if (active && out.takes_part(k) && overlap_sphere(b, g[4 * k + 0], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]))
        out.take(k);
  }
  {
    cdptr g = (cdptr)sc.mov;
    for (int k = 0; k < sc.n_mov; ++k)
      if (active && out.takes_part(sc.n_sph + k) &&
          overlap_sphere(b, g[8 * k + 0] + b.time * g[8 * k + 3], g[8 * k + 1] + b.time * g[8 * k + 4],
                         g[8 * k + 2] + b.time * g[8 * k + 5], g[8 * k + 6]))
        out.take(sc.n_sph + k);
  }
  {
    cdptr g = (cdptr)sc.tri;
    const int base = sc.n_sph + sc.n_mov;
    for (int k = 0; k < sc.n_tri; ++k)
      if (active && out.takes_part(base + k) &&
          overlap_triangle(b, V3d{g[12 * k + 0], g[12 * k + 1], g[12 * k + 2]}, V3d{g[12 * k + 3], g[12 * k + 4], g[12 * k + 5]},
                           V3d{g[12 * k + 6], g[12 * k + 7], g[12 * k + 8]}, V3d{g[12 * k + 9], g[12 * k + 10], g[12 * k + 11]}))
        out.take(base + k);
  }
  if (active) nprim += (uint32_t)(sc.n_sph + sc.n_mov + sc.n_tri);
}

// ---- the node test: the node's box against the query box inflated by sigma (OvBox I), inclusive ----
__device__ __forceinline__ bool ov_node(const OvBox &I, double lx, double ly, double lz, double hx, double hy, double hz) {
  return lx <= I.hi.x && hx >= I.lo.x && ly <= I.hi.y && hy >= I.lo.y && lz <= I.hi.z && hz >= I.lo.z;
}
__device__ __forceinline__ OvBox ov_inflate(const OvBox &b, double mag) {
  const double sigma = pq_sigma(V3d{fmax(fabs(b.lo.x), fabs(b.hi.x)), fmax(fabs(b.lo.y), fabs(b.hi.y)),
                                    fmax(fabs(b.lo.z), fabs(b.hi.z))}, mag);
  return OvBox{{b.lo.x - sigma, b.lo.y - sigma, b.lo.z - sigma}, {b.hi.x + sigma, b.hi.y + sigma, b.hi.z + sigma}, b.time};
}

// ---- BVH: the threaded walk and leaf queue of closest_bvh (rtow_point_walks.h) with the box test ----
template <bool LDS>
__device__ __forceinline__ void overlap_bvh(const Image<LDS> &im, const DevScene &sc, const OvBox &b, bool active,
                                            OverlapSink &out, uint32_t &nnode, uint32_t &nprim) {
  const uint32_t END = (uint32_t)sc.n_nodes;
  OvBox I = b;
  if (active) {  // the root box bounds every primitive: its magnitude scales the slack
    const float4 r0 = im.f4(0u), r1 = im.f4(16u);
    I = ov_inflate(b, box_mag(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y));
  }
  int last_id = -1;
  uint32_t node = active ? 0u : END;
  uint32_t q0 = 0u, q1 = 0u, q2 = 0u, q3 = 0u;  // queued leaves (0 = empty), oldest first
  for (;;) {
    if (node < END) {
      const float4 r0 = im.f4(node * 32u), r1 = im.f4(node * 32u + 16u);
      ++nnode;
      const bool meets = ov_node(I, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y);
      const uint32_t skip = __float_as_uint(r1.z), leaf = __float_as_uint(r1.w);
      if (meets && leaf != 0u) {
        if (q0 == 0u)
          q0 = leaf;
        else if (q1 == 0u)
          q1 = leaf;
        else if (q2 == 0u)
          q2 = leaf;
        else
          q3 = leaf;
      }
      node = (meets && leaf == 0u) ? node + 1u : skip;
    }
    const bool any_walking = __any(node < END);
    if (__any(q3 != 0u) || !any_walking) {
      if (q0 != 0u) {
        const uint32_t first = q0 >> 3, count = q0 & 7u;
        for (uint32_t k = 0; k < count; ++k) {
          const int id = sc.leaf_direct ? (int)(first + k) : (int)im.u32(sc.off_ids + 4u * (first + k));
          if (id == last_id) continue;
          last_id = id;
          if (!out.takes_part(id)) continue;
          ++nprim;
          if (overlap_image_prim<LDS>(im, sc, id, b)) out.take(id);
        }
      }
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = 0u;
      if (!any_walking && !__any(q0 != 0u)) break;
    }
  }
}

// ---- BVH4: the per-lane stack (and spill) of closest_bvh4; the first child that meets the box next, the others pushed ----
template <bool FULL>
__device__ __forceinline__ void overlap_bvh4(const Bvh4Reader<FULL> &im, const DevScene &sc, const TraceParams &P,
                                             const OvBox &b, bool active, uint32_t lane_g, OverlapSink &out,
                                             uint32_t &nnode, uint32_t &nprim) {
  const Bvh4Stack st = bvh4_stack(sc);
  OvBox I = b;
  if (active) {  // the root's children bound every primitive
    double pl[6][4];
    vu4 cw;
    bvh4_node<FULL>(im, sc, 0u, pl, cw);
    const uint32_t c[4] = {cw.x, cw.y, cw.z, cw.w};
    double mag = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c[j] != kRefNone) mag = fmax(mag, box_mag(pl[0][j], pl[2][j], pl[4][j], pl[1][j], pl[3][j], pl[5][j]));
    I = ov_inflate(b, mag);
  }
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
    // (2) next entry from the stack
    if (cur == kRefPop) {
      if (sa == st.lds) {
        cur = kRefNone;
      } else {
        sa -= kBvh4StackStride;
        if (sa < st.end)
          cur = lds_read<uint32_t>(sa);
        else
          cur = P.spill[(size_t)((sa - st.end) >> kBvh4StackStrideLog2) * P.n_lanes + lane_g];
      }
    }
    // (3) one node: four box tests, the first child that meets the box next, the others to the stack
    if (cur < kRefLeaf) {
      double pl[6][4];
      vu4 cw;
      bvh4_node<FULL>(im, sc, cur, pl, cw);
      ++nnode;
      const uint32_t c[4] = {cw.x, cw.y, cw.z, cw.w};
      cur = kRefPop;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c[j] != kRefNone && ov_node(I, pl[0][j], pl[2][j], pl[4][j], pl[1][j], pl[3][j], pl[5][j])) {
          if (cur == kRefPop) {
            cur = c[j];
          } else {
            if (sa < st.end)
              lds_write<uint32_t>(sa, c[j]);
            else
              P.spill[(size_t)((sa - st.end) >> kBvh4StackStrideLog2) * P.n_lanes + lane_g] = c[j];
            sa += kBvh4StackStride;
          }
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
          const int id = (int)(first + j);
          if (!out.takes_part(id)) continue;
          const uint32_t r = sc.b4_off_tri + 96u * (first + j);
          const vd2 t0 = im.t2(r), t1 = im.t2(r + 16u), t2 = im.t2(r + 32u), t3 = im.t2(r + 48u), t4 = im.t2(r + 64u),
                    t5 = im.t2(r + 80u);
          ++nprim;
          if (overlap_triangle(b, V3d{t0.x, t0.y, t1.x}, V3d{t1.y, t2.x, t2.y}, V3d{t3.x, t3.y, t4.x},
                               V3d{t4.y, t5.x, t5.y}))
            out.take(id);
        }
      }
      q0 = q1;
      q1 = kRefNone;
      if (!any_walking && !__any(q0 != kRefNone)) break;
    }
  }
}

// ---- a query ----
// {lo.x, lo.y} {lo.z, hi.x} {hi.y, hi.z} {time, (min_prim, pad)}: four 16-byte loads
__device__ __forceinline__ void load_box_query(const unsigned char *queries, uint32_t i, V3d &lo, V3d &hi, double &time,
                                               int32_t &min_prim) {
  const vd2 *r = reinterpret_cast<const vd2 *>(queries + (size_t)i * kBoxQueryBytes);
  const vd2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
  lo = {r0.x, r0.y, r1.x};
  hi = {r1.y, r2.x, r2.y};
  time = r3.x;
  min_prim = (int32_t)(uint32_t)(unsigned long long)__double_as_longlong(r3.y);
}
