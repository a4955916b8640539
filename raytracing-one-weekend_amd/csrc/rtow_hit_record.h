// rtow_hit_record.h — the rtow_hit_t record (include/rtow.h) of one accepted (t, primitive), shared by the query units
// that report hits: the closest-hit query (rtow_query.h) and the first-k-hits query (rtow_first_hits.h).  Included
// inside `namespace rtow { namespace {` after the walk headers and rtow_kernel_frame.h; the render units do not see it.
//
// The expressions are the trace kernel's (rtow_trace_body.h, the `do_scat` block): Ray::at, the sphere normal faced
// against the ray, the triangle's un-normalised e1 x e2, the material index from the scene image the walk read.
#pragma once

constexpr uint32_t kHitBytes = 72u;  // rtow_hit_t, include/rtow.h

// Writes the record of ray (ro, rd, rtime) at `dst` (8-byte aligned): of the walk's primitive `pid` accepted at `t` when
// `hit`, else the miss record (t = +inf, zeros, -1, -1, -1, 0).  KERNEL / LDS: the walk whose ids `pid` is (1 STREAM and
// 5 REFTREE: the class-major arrays; 2 / 3: the BVH / grid image behind `im`; 4: the 4-wide image behind `im4`).
// `map`: walk id -> insertion index.
template <int KERNEL, bool LDS>
__device__ __forceinline__ void write_hit_record(const Image<LDS> &im, const Bvh4Reader<LDS> &im4, const DevScene &sc,
                                                 const int32_t *map, V3 ro, V3 rd, real rtime, bool hit, int pid, real t_hit,
                                                 unsigned char *dst) {
  double t = __builtin_huge_val();
  V3 p = {0, 0, 0}, normal = {0, 0, 0};
  int32_t prim = -1, kind = -1, mi = -1, front = 0;
  if (hit) {
    t = t_hit;
    p = ro + rd * t_hit;  // Ray::at (the trace kernel's scattered origin)
    bool ff = true;       // triangles: front_facing is always true (src/common-model.cpp:121)
    kind = pid < sc.n_sph ? 0 : (pid < sc.n_sph + sc.n_mov ? 1 : 2);
    if constexpr (KERNEL == 4) {
      const uint32_t r = sc.b4_off_tri + 96u * (uint32_t)pid;
      const vd2 q4 = im4.t2(r + 64u), q5 = im4.t2(r + 80u);
      normal = {(real)q4.y, (real)q5.x, (real)q5.y};
      mi = (int)im4.u32(sc.b4_off_pmat + 4u * (uint32_t)pid);
    } else if constexpr (KERNEL == 2 || KERNEL == 3) {
      const uint32_t o_sph = KERNEL == 3 ? sc.g_off_sph : sc.off_sph;
      const uint32_t o_mov = KERNEL == 3 ? sc.g_off_mov : sc.off_mov;
      const uint32_t o_tri = KERNEL == 3 ? sc.g_off_tri : sc.off_tri;
      const uint32_t o_pmat = KERNEL == 3 ? sc.g_off_pmat : sc.off_pmat;
      if (pid < sc.n_sph + sc.n_mov) {
        V3 center;
        bool inward;
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
        ff = (dot(rd, normal) < real(0.0)) ^ inward;
        normal = ff ? normal : -normal;
      } else {
        const uint32_t r = o_tri + 96u * (uint32_t)(pid - sc.n_sph - sc.n_mov);
        const double2 q4 = im.d2(r + 64u), q5 = im.d2(r + 80u);
        normal = {q4.y, q5.x, q5.y};
      }
      mi = (int)im.u32(o_pmat + 4u * (uint32_t)pid);
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
        ff = (dot(rd, normal) < real(0.0)) ^ inward;
        normal = ff ? normal : -normal;
      } else {
        const double *q = sc.tri + 12 * (size_t)(pid - sc.n_sph - sc.n_mov);
        normal = {(real)q[9], (real)q[10], (real)q[11]};
      }
      mi = sc.prim_mat[pid];
    }
    prim = map[pid];
    front = ff ? 1 : 0;
  }
  double *h = reinterpret_cast<double *>(dst);
  h[0] = t;
  h[1] = p.x;
  h[2] = p.y;
  h[3] = p.z;
  h[4] = normal.x;
  h[5] = normal.y;
  h[6] = normal.z;
  int32_t *hi = reinterpret_cast<int32_t *>(h + 7);
  reinterpret_cast<int2 *>(hi)[0] = make_int2(prim, kind);
  reinterpret_cast<int2 *>(hi)[1] = make_int2(mi, front);
}
