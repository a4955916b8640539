// rtow_any_hit.h — "does anything lie within [0.001, tmax] of this ray?", written once for the two query families that
// ask it: the occlusion query (rtow_occlude.h: one caller ray per lane) and the ambient query (rtow_ambient.h: a loop of
// hemisphere samples per lane).  The any-hit sink of the tmax-bounded walks (rtow_bounded_walks.h), the three wrappers
// that run a walk with it, and the BRUTE strategy's stream over the class arrays.  Included inside `namespace rtow {
// namespace {` after rtow_kernel_frame.h and rtow_bounded_walks.h; the render units do not see it.
#pragma once

// The closest-so-far value a walk starts from: the ray's tmax (+inf: no bound).
__device__ __forceinline__ Closest seeded(double tmax) {
  Closest best;
  best.t = (real)tmax;
  best.prim = -1;
  return best;
}

// ---- the any-hit sink of the bounded walks (rtow_bounded_walks.h) ----
// A whole leaf, cell or list per call, against one Closest seeded with tmax.  The culling bound stays tmax: the walk ends
// at the lane's first hit, so a smaller one could never be observed.  One mailbox for the whole walk.
struct AnyHitSink {
  static constexpr bool kFold = true;
  Closest best;
  float tmax32;
  int last_id;
  __device__ __forceinline__ void seed(double tmax) {
    best = seeded(tmax);
    tmax32 = round_up_f32(best.t);
    last_id = -1;
  }
  __device__ __forceinline__ float bound32() const { return tmax32; }
  __device__ __forceinline__ bool done() const { return best.prim >= 0; }  // occluded: this lane is finished
  template <bool LDS, bool CELL>
  __device__ __forceinline__ void list(const Image<LDS> &im, const DevScene &sc, const ImgOffsets &off, uint32_t first,
                                       uint32_t count, const RayForms &ray, uint32_t &nprim) {
    leaf_test<LDS, CELL>(im, sc, off, first, count, ray, best, nprim, last_id);
  }
  // as closest_hit_grid tests them (static spheres four, then two at a time: all records loaded and all discriminants
  // computed before any hit branch).  A copy of that walk's block: lifting it into a function both call changed the
  // render kernels' code objects, and those stay as they are.
  template <bool LDS>
  __device__ __forceinline__ void large(const Image<LDS> &im, const DevScene &sc, const ImgOffsets &off, uint32_t lf,
                                        uint32_t n_large, const RayForms &ray, uint32_t &nprim) {
    uint32_t k = 0;
    for (; k + 3 < n_large; k += 4) {
      int id[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) id[j] = (int)im.u32(off.ids + 4u * (lf + k + j));
      if (id[0] < sc.n_sph && id[1] < sc.n_sph && id[2] < sc.n_sph && id[3] < sc.n_sph) {
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
        leaf_test<LDS, false, 0, true>(im, sc, off, lf + k, 4u, ray, best, nprim, last_id);
      }
    }
    for (; k + 1 < n_large; k += 2) {
      const int ia = (int)im.u32(off.ids + 4u * (lf + k)), ib = (int)im.u32(off.ids + 4u * (lf + k + 1));
      if (ia < sc.n_sph && ib < sc.n_sph) {
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
        leaf_test<LDS, false, 0, true>(im, sc, off, lf + k, 2u, ray, best, nprim, last_id);
      }
    }
    if (k < n_large) leaf_test<LDS, false, 0, true>(im, sc, off, lf + k, n_large - k, ray, best, nprim, last_id);
  }
  template <bool FULL>
  __device__ __forceinline__ void leaf4(const Bvh4Reader<FULL> &im, const DevScene &sc, uint32_t leaf, V3d o64, V3d d64,
                                        uint32_t &nprim) {
    bvh4_leaf<FULL>(im, sc, leaf, o64, d64, best, nprim);
  }
};

template <bool LDS>
__device__ __forceinline__ bool any_hit_bvh(const Image<LDS> &im, const DevScene &sc, V3 o, V3 d, real time, double tmax,
                                            bool active, uint32_t &nnode, uint32_t &nprim) {
  AnyHitSink sink;
  bounded_walk_bvh<LDS>(im, sc, o, d, time, tmax, active, sink, nnode, nprim);
  return sink.done();
}
template <bool LDS>
__device__ __forceinline__ bool any_hit_grid(const Image<LDS> &im, const DevScene &sc, V3 o, V3 d, real time,
                                             double tmax, bool active, uint32_t &nnode, uint32_t &nprim,
                                             uint32_t leaf_votes) {
  AnyHitSink sink;
  bounded_walk_grid<LDS>(im, sc, o, d, time, tmax, active, sink, nnode, nprim, leaf_votes);
  return sink.done();
}
template <bool FULL>
__device__ __forceinline__ bool any_hit_bvh4(const Bvh4Reader<FULL> &im, const DevScene &sc, const TraceParams &P, V3 o,
                                             V3 d, double tmax, bool active, uint32_t lane_g, uint32_t &nnode,
                                             uint32_t &nprim) {
  AnyHitSink sink;
  bounded_walk_bvh4<FULL>(im, sc, P, o, d, tmax, active, lane_g, sink, nnode, nprim);
  return sink.done();
}

// ---- STREAM: closest_hit_stream (rtow_trace_hit.h), seeded; the wave leaves when every active lane has a hit ----
// `open`: the lane has a ray and no hit yet.  The votes are wave-level (one per block of four spheres, per pair of
// scalar-loaded triangles, per tile): the tiled triangle loop stages its tiles with all 64 lanes, so a lane that is
// done stays in the loop until the whole wave is.
__device__ __forceinline__ bool any_hit_stream(const DevScene &sc, V3d o, V3d d, double time, double tmax, bool active,
                                               uint32_t &nprim) {
  Closest best = seeded(tmax);
  const double tmin = RTOW_TMIN;
  const double a = dot(d, d);
  const double inv_a = fast_rcp(a);  // used by the fast build only
  bool open = active;
  {
    cdptr g = (cdptr)sc.sph;
    const int n = sc.n_sph;
    for (int i = 0; i < n; i += 4) {
      if (!__any(open)) break;
      const int e = i + 4 < n ? i + 4 : n;
      if (open) {
        for (int k = i; k < e; ++k)
          sphere_test<double>(o, d, a, inv_a, g[4 * k + 0], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3], k, tmin, best);
        nprim += (uint32_t)(e - i);
      }
      open = open && best.prim < 0;
    }
  }
  {
    cdptr g = (cdptr)sc.mov;
    const int n = sc.n_mov;
    const int base = sc.n_sph;
    for (int i = 0; i < n; i += 2) {
      if (!__any(open)) break;
      const int e = i + 2 < n ? i + 2 : n;
      if (open) {
        for (int k = i; k < e; ++k) {
          const double cx = g[8 * k + 0] + time * g[8 * k + 3];
          const double cy = g[8 * k + 1] + time * g[8 * k + 4];
          const double cz = g[8 * k + 2] + time * g[8 * k + 5];
          sphere_test<double>(o, d, a, inv_a, cx, cy, cz, g[8 * k + 6], base + k, tmin, best);
        }
        nprim += (uint32_t)(e - i);
      }
      open = open && best.prim < 0;
    }
  }
  if (sc.stream_tile_lds != 0u) {
    // the tiled loop of closest_hit_stream: the same staging (two 3 KB tiles per wave, coalesced fetch, broadcast reads)
    const int n = sc.n_tri;
    const int base = sc.n_sph + sc.n_mov;
    if (__any(open)) {
      const unsigned lane = lane_id();
      const uint32_t slice = (threadIdx.x >> 6) * (2u * kStreamTileBytes);
      const unsigned char *src = (const unsigned char *)sc.tri;
      const uint32_t total = (uint32_t)n * 96u;
      const uint32_t ntiles = ((uint32_t)n + kStreamTile - 1u) / kStreamTile;
      vu4 r0, r1, r2;
      auto fetch = [&](uint32_t tile) {
        const uint32_t p = tile * kStreamTileBytes + 16u * lane;
        const vu4 z = {0u, 0u, 0u, 0u};
        r0 = p < total ? glb_read<vu4>(src, p) : z;
        r1 = p + 1024u < total ? glb_read<vu4>(src, p + 1024u) : z;
        r2 = p + 2048u < total ? glb_read<vu4>(src, p + 2048u) : z;
      };
      auto park = [&](uint32_t buf) {
        const uint32_t q = slice + buf * kStreamTileBytes + 16u * lane;
        lds_write<vu4>(q, r0);
        lds_write<vu4>(q + 1024u, r1);
        lds_write<vu4>(q + 2048u, r2);
      };
      fetch(0u);
      park(0u);
      for (uint32_t tile = 0; tile < ntiles; ++tile) {
        if (tile + 1u < ntiles) fetch(tile + 1u);
        const uint32_t tb = slice + (tile & 1u) * kStreamTileBytes;
        const int first = (int)(tile * kStreamTile);
        const int cnt = n - first < (int)kStreamTile ? n - first : (int)kStreamTile;
        if (open) {
          for (int k = 0; k < cnt; ++k) {
            const uint32_t r = tb + 96u * (uint32_t)k;
            const vd2 p0 = lds_read<vd2>(r), p1 = lds_read<vd2>(r + 16u), p2 = lds_read<vd2>(r + 32u),
                      p3 = lds_read<vd2>(r + 48u), p4 = lds_read<vd2>(r + 64u), p5 = lds_read<vd2>(r + 80u);
            triangle_test<double>(o, d, V3d{p0.x, p0.y, p1.x}, V3d{p1.y, p2.x, p2.y}, V3d{p3.x, p3.y, p4.x},
                                  V3d{p4.y, p5.x, p5.y}, base + first + k, tmin, best);
          }
          nprim += (uint32_t)cnt;
        }
        open = open && best.prim < 0;
        if (!__any(open)) break;  // (wave-uniform: the tile fetched for the next round is not parked)
        if (tile + 1u < ntiles) park((tile + 1u) & 1u);
      }
    }
  } else {
    cdptr g = (cdptr)sc.tri16;
    const int n = sc.n_tri;
    const int base = sc.n_sph + sc.n_mov;
    for (int i = 0; i < n; i += 2) {
      if (!__any(open)) break;
      const int e = i + 2 < n ? i + 2 : n;
      if (open) {
        for (int k = i; k < e; ++k)
          triangle_test<double>(o, d, V3d{g[16 * k + 0], g[16 * k + 1], g[16 * k + 2]},
                                V3d{g[16 * k + 3], g[16 * k + 4], g[16 * k + 5]},
                                V3d{g[16 * k + 6], g[16 * k + 7], g[16 * k + 8]},
                                V3d{g[16 * k + 9], g[16 * k + 10], g[16 * k + 11]}, base + k, tmin, best);
        nprim += (uint32_t)(e - i);
      }
      open = open && best.prim < 0;
    }
  }
  return best.prim >= 0;
}
