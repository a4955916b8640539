// rtow_scene_records.h — the ray-independent record of every primitive, from the scene as the caller gives it.
//
// Pure host arithmetic without HIP (the sanitizer harness tests/tools/builders_sanitize.cpp calls it).  Each term is
// computed with the reference's operations; every translation unit that includes this is built with
// -ffp-contract=off, so each is one IEEE operation, as on the CPU.  csrc/rtow_refit.hip has the device twin.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rtow {

// sphere [n][4] cx cy cz copysign(r*r, r) and its radius; moving [n][8] c0 (c1 - c0) copysign(r*r, r) r;
// triangle [n][12] a e1 e2 n; material index per primitive (class-major) and the device material records as bytes
struct SceneRecords {
  std::vector<double> sph, sph_r, mov, tri;
  std::vector<int32_t> pmat;
  std::vector<unsigned char> mats_bytes;
};

// radius * radius (src/common-model.cpp:73), carrying the radius' sign: the tests take |.|
// for free (VOP3 input modifier), the shading step reads the sign (front_facing, :88)
inline double signed_r2(double r) { return std::copysign(r * r, r); }

// g: c0 xyz, c1 xyz, r, pad
inline void moving_record(const double *g, double *d) {
  for (int k = 0; k < 3; ++k) {
    d[k] = g[k];
    d[3 + k] = g[3 + k] - g[k];  // center1 - center0, src/oo-primitives.h:65
  }
  d[6] = signed_r2(g[6]);
  d[7] = g[6];
}

// g: a, b, c
inline void triangle_record(const double *g, double *d) {
  const double e1[3] = {g[3] - g[0], g[4] - g[1], g[5] - g[2]};  // b - a
  const double e2[3] = {g[6] - g[0], g[7] - g[1], g[8] - g[2]};  // c - a
  for (int k = 0; k < 3; ++k) {
    d[k] = g[k];
    d[3 + k] = e1[k];
    d[6 + k] = e2[k];
  }
  // n = cross(e1, e2), src/common-model.cpp:108
  d[9] = e1[1] * e2[2] - e2[1] * e1[2];
  d[10] = e1[2] * e2[0] - e2[2] * e1[0];
  d[11] = e1[0] * e2[1] - e2[0] * e1[1];
}

// geom: [ns][4] cx cy cz r.  (A refit needs no other records on the host: they decide the grid's fat-list format.)
inline void sphere_records(const double *geom, int ns, std::vector<double> &sph, std::vector<double> &sph_r) {
  sph.assign(geom, geom + 4 * (size_t)ns);
  sph_r.resize((size_t)ns);
  for (size_t i = 0; i < (size_t)ns; ++i) {
    sph_r[i] = geom[4 * i + 3];
    sph[4 * i + 3] = signed_r2(sph_r[i]);
  }
}

// sph, sph_r, mov and tri of `out` (pmat and mats_bytes are the caller's: make_scene_records, rtow_scene.cpp)
inline void geometry_records(const double *sphere_geom, int ns, const double *moving_geom, int nm,
                             const double *triangle_geom, int nt, SceneRecords &out) {
  sphere_records(sphere_geom, ns, out.sph, out.sph_r);
  out.mov.resize((size_t)nm * 8);
  for (int i = 0; i < nm; ++i) moving_record(moving_geom + 8 * (size_t)i, &out.mov[8 * (size_t)i]);
  out.tri.resize((size_t)nt * 12);
  for (int i = 0; i < nt; ++i) triangle_record(triangle_geom + 9 * (size_t)i, &out.tri[12 * (size_t)i]);
}

}  // namespace rtow
