// rtow_scatter.h — what a path does after a closest hit, shared by the two query units that scatter: the radiance
// query (rtow_radiance.h) and the path-step query (rtow_step.h).  The shading surface of the winner and its material
// (rtow_trace_body.h, the `do_scat` block), Material::scatter (scatter_dir) and the sky, restated from the trace kernel
// expression for expression; the strict radiance query's comparison with the oracle (tests/test_gpu_radiance.py) is what
// proves the copy, and the path step's (tests/test_gpu_path_step.py) proves it segment by segment.  Included inside
// `namespace rtow { namespace {` after the walk headers, rtow_trace_rng.h and rtow_kernel_frame.h; the render units do
// not see it.
#pragma once

// -0.0 -> +0.0, every other value unchanged (rtow_query.h: the grid walk's DDA takes its step direction from `d >= 0`
// and its increments from rcp(d), which disagree for -0.0; the hit tests give the same t and primitive either way).
__device__ __forceinline__ double plus_zero(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return __longlong_as_double((long long)(b == 0x8000000000000000ull ? 0ull : b));
}

// The Hit of the winner (src/common-model.cpp:83-90, :121) and what scatter reads of its material.  `p`: Ray::at of the
// hit; `pid`: the walk's primitive id.  KERNEL / LDS: the walk whose ids `pid` is (1 STREAM and 5 REFTREE: the
// class-major arrays; 2 / 3: the BVH / grid image behind `im`; 4: the 4-wide image behind `im4`).
struct Surface {
  V3 normal;      // spheres: unit, faced against the ray; triangles: the un-normalised e1 x e2
  bool front;     // triangles: always true
  int mi, kind;   // material index and DevMaterial::kind (0 Lambertian, 1 metal, 2 dielectric)
  real fuzz, ir;
};
template <int KERNEL, bool LDS>
__device__ __forceinline__ Surface surface_at(const Image<LDS> &im, const Bvh4Reader<LDS> &im4, const DevScene &sc, V3 p,
                                              V3 rd, real rtime, int pid) {
  Surface s;
  s.front = true;
  if constexpr (KERNEL == 4) {
    const uint32_t r = sc.b4_off_tri + 96u * (uint32_t)pid;
    const vd2 q4 = im4.t2(r + 64u), q5 = im4.t2(r + 80u);
    s.normal = {(real)q4.y, (real)q5.x, (real)q5.y};
    s.mi = (int)im4.u32(sc.b4_off_pmat + 4u * (uint32_t)pid);
    const uint32_t mr = sc.b4_off_mats + 48u * (uint32_t)s.mi;
    const vd2 m1 = im4.d2(mr + 16u), m2 = im4.d2(mr + 32u);  // {att.z, fuzz}, {ir, kind|pad}
    s.fuzz = (real)m1.y;
    s.ir = (real)m2.x;
    s.kind = (int)(__double_as_longlong(m2.y) & 0xffffffffll);
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
      s.normal = normalize(p - center);
      s.front = (dot(rd, s.normal) < real(0.0)) ^ inward;
      s.normal = s.front ? s.normal : -s.normal;
    } else {
      const uint32_t r = o_tri + 96u * (uint32_t)(pid - sc.n_sph - sc.n_mov);
      const double2 q4 = im.d2(r + 64u), q5 = im.d2(r + 80u);
      s.normal = {q4.y, q5.x, q5.y};
    }
    s.mi = (int)im.u32(o_pmat + 4u * (uint32_t)pid);
    const uint32_t mr = o_mats + 48u * (uint32_t)s.mi;
    const double2 m1 = im.d2(mr + 16u), m2 = im.d2(mr + 32u);  // {att.z, fuzz}, {ir, kind|pad}
    s.fuzz = (real)m1.y;
    s.ir = (real)m2.x;
    s.kind = (int)(__double_as_longlong(m2.y) & 0xffffffffll);
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
      s.normal = normalize(p - center);
      s.front = (dot(rd, s.normal) < real(0.0)) ^ inward;
      s.normal = s.front ? s.normal : -s.normal;
    } else {
      const double *q = sc.tri + 12 * (size_t)(pid - sc.n_sph - sc.n_mov);
      s.normal = {(real)q[9], (real)q[10], (real)q[11]};
    }
    s.mi = sc.prim_mat[pid];
    const DevMaterial *m = sc.mats + s.mi;
    s.kind = m->kind;
    s.fuzz = (real)m->fuzz;
    s.ir = (real)m->ir;
  }
  return s;
}

// The attenuation of material `mi` as uploaded, from the image the walk read (the strict radiance query folds a path's
// attenuations by index from the end; everything else reads it beside surface_at, whose loads it shares).
template <int KERNEL, bool LDS>
__device__ __forceinline__ V3 material_att(const Image<LDS> &im, const Bvh4Reader<LDS> &im4, const DevScene &sc,
                                           uint32_t mi) {
  if constexpr (KERNEL == 4) {
    const uint32_t mr = sc.b4_off_mats + 48u * mi;
    const vd2 a0 = im4.d2(mr), a1 = im4.d2(mr + 16u);  // {att.x, att.y}, {att.z, fuzz}
    return V3{(real)a0.x, (real)a0.y, (real)a1.x};
  } else if constexpr (KERNEL == 2 || KERNEL == 3) {
    const uint32_t mr = (KERNEL == 3 ? sc.g_off_mats : sc.off_mats) + 48u * mi;
    const double2 a0 = im.d2(mr), a1 = im.d2(mr + 16u);
    return V3{(real)a0.x, (real)a0.y, (real)a1.x};
  } else {
    const DevMaterial *m = sc.mats + mi;
    return V3{(real)m->att[0], (real)m->att[1], (real)m->att[2]};
  }
}

// Material::scatter (src/common-model.cpp:13-62): rtow_trace_body.h's scatter_dir, restated — the new direction, or
// absorbed; the point of the unit ball and the dielectric coin come from the bounce's one Philox block.
__device__ __forceinline__ bool scatter_dir(Rng &g, uint32_t k0, uint32_t k1, int kind, real m_fuzz, real m_ir, V3 rd,
                                            V3 normal, bool front, V3 &dir) {
  uint32_t o0, o1, o2, o3;
  philox4x32(g.r, g.sample, g.pixel, 0u, k0, k1, o0, o1, o2, o3);
  g.r += 1u;
  V3 dirbase = {0, 0, 0};
  if (kind == 2) {
    const real ir = m_ir;
    const V3 unit = normalize(rd);
    const real cos_theta = dot(-unit, normal);
    const real sin_theta = fast_sqrt(real(1.0) - cos_theta * cos_theta);
    const real ratio = front ? fast_rcp(ir) : ir;
    bool refl = ratio * sin_theta > real(1.0);
    if (!refl) {  // src/common-model.cpp:53-54: the coin is drawn only if refraction is possible
      real r0 = fast_div(real(1.0) - ratio, real(1.0) + ratio);
      r0 = r0 * r0;
      const real x = real(1.0) - cos_theta;
      const real x2 = x * x;
      const real R = r0 + (real(1.0) - r0) * (x2 * x2 * x);
      refl = R > coin_from_block(o0, o1, o3);
    }
    dirbase = refl ? reflect(unit, normal) : refract(unit, normal, ratio);
  } else if (kind == 1) {
    dirbase = reflect(rd, normal);
  }
  // random_unit_vector() (random-utils.cpp:31-33): the point of the unit ball's positive octant, un-normalised
  const V3 rnd = ball_from_block(o0, o1, o2, o3);
  bool absorbed = false;
  if (kind == 0) {
    absorbed = rabs(normal.x - rnd.x) < real(1e-8) && rabs(normal.y - rnd.y) < real(1e-8) &&
               rabs(normal.z - rnd.z) < real(1e-8);
    dir = normal + rnd;
  } else {
    dir = dirbase + m_fuzz * rnd;
  }
  return !absorbed;
}

// The reference's background for a ray of direction `rd` (src/render.cpp:122-128)
__device__ __forceinline__ V3 sky_color(V3 rd) {
  const V3 unit = normalize(rd);
  const real t = real(0.5) * (unit.y + real(+1.0));
  return (real(1.0) - t) * V3{1, 1, 1} + t * V3{real(0.5), real(0.7), real(1.0)};
}
