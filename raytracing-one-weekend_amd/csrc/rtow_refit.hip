// rtow_refit.hip — in-place refit of the resident scene (rtow_scene_refit): new geometry under the trees' old topology.
//
// Everything derived from geometry is recomputed here with the host builder's own formulas, each one IEEE binary64
// operation (this file is built with -ffp-contract=off, like rtow_build.hip), so that an unchanged refit reproduces a
// host-built image byte for byte:
//   records     copysign(r*r, r), c1 - c0, e1, e2, n = e1 x e2 in scene_upload's operation order (rtow_capi.cpp)
//   prim boxes  build_bvh's rules (rtow_bvh.h): sphere c +- |r|, moving sphere over the widened shutter, triangle min/max
//               of a, a + e1, a + e2; then pad_box
//   node boxes  unions by min / max, bottom-up with arrival counters (the k_refit pattern of rtow_build.hip)
//   planes      make_scene_image's / make_bvh4_image's pad and outward rounding, scale = max(1, |root box|, |camera|);
//               binary16 planes in a frame recomputed from the new root box
// Topology words (skip links, leaf words, child words) are never written.  Every kernel is index-checked against its
// count; the links it follows were validated when the image was built.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace rtow {

namespace {

constexpr uint32_t kRefNone = 0x1fffffu;  // rtow_bvh4.h
constexpr uint32_t kRefLeaf = 1u << 20;
constexpr int kB = 256;

// std::min / std::max of the host code (the first argument on ties)
__device__ __forceinline__ double hmin(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double hmax(double a, double b) { return a < b ? b : a; }

__device__ __forceinline__ void box_empty(double b[6]) {
  for (int k = 0; k < 3; ++k) {
    b[k] = INFINITY;
    b[3 + k] = -INFINITY;
  }
}
__device__ __forceinline__ void box_grow(double b[6], const double o[6]) {
  for (int k = 0; k < 3; ++k) {
    b[k] = hmin(b[k], o[k]);
    b[3 + k] = hmax(b[3 + k], o[3 + k]);
  }
}
// a box another workgroup wrote just before its arrival: read past this CU's L1
__device__ __forceinline__ void box_load_agent(double b[6], const double *src) {
  for (int k = 0; k < 6; ++k)
    b[k] = __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(src + k),
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ double half_area(const double *b) {  // bvh_detail::Box::half_area
  const double dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
  if (!(dx >= 0) || !(dy >= 0) || !(dz >= 0)) return 0.0;
  return dx * dy + dy * dz + dz * dx;
}
// max(1, |root box|, |camera origin|): the pad scale of make_scene_image / make_bvh4_image
__device__ __forceinline__ double pad_scale(const double *root, double ox, double oy, double oz) {
  double s = 1.0;
  for (int k = 0; k < 3; ++k) s = hmax(s, fabs(root[k]));
  for (int k = 0; k < 3; ++k) s = hmax(s, fabs(root[3 + k]));
  s = hmax(s, fabs(ox));
  s = hmax(s, fabs(oy));
  return hmax(s, fabs(oz));
}
__device__ __forceinline__ double plane_pad(double scale, double lo, double hi) {
  return 2e-6 * scale + 2e-6 * hmax(fabs(lo), fabs(hi));
}

// rtow_bvh4.h half_directed, as it is: the largest binary16 <= x (dir < 0) or the smallest >= x (dir > 0)
__device__ uint16_t half_directed(double x, int dir) {
  if (isnan(x)) return 0x7e00;
  const bool neg = signbit(x);
  const double a = fabs(x);
  const bool mag_up = (dir > 0) != neg;
  const uint16_t sign = neg ? 0x8000 : 0;
  if (a == 0.0) return sign;
  if (isinf(a)) return sign | 0x7c00;
  if (a > 65504.0) return sign | (mag_up ? 0x7c00 : 0x7bff);
  const uint64_t b = (uint64_t)__double_as_longlong(a);
  const int be = (int)(b >> 52);
  if (be == 0) return sign | (uint16_t)(mag_up ? 1 : 0);
  const int e = be - 1023;
  const uint64_t m = (b & ((1ull << 52) - 1ull)) | (1ull << 52);
  const int E = e > -14 ? e : -14;
  const int sh = 42 + (E - e);
  const uint64_t q = sh >= 64 ? 0ull : (m >> sh);
  const bool inexact = sh >= 64 ? true : (m & ((1ull << sh) - 1ull)) != 0ull;
  const uint32_t qi = (uint32_t)q + ((mag_up && inexact) ? 1u : 0u);
  const uint32_t bits = (E == -14 && qi < 1024u) ? qi : (((uint32_t)(E + 15) << 10) + (qi - 1024u));
  return sign | (uint16_t)(bits < 0x7c00u ? bits : 0x7c00u);
}

// ---- records from raw geometry (scene_upload's precompute) ------------------------------------------------------------
__global__ void kr_records(const double *gs, const double *gm, const double *gt, int ns, int nm, int nt, double *sph,
                           double *sph_r, double *mov, double *tri, double *tri16) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns + nm + nt) return;
  if (i < ns) {
    const double *g = gs + (size_t)i * 4;
    double *d = sph + (size_t)i * 4;
    d[0] = g[0];
    d[1] = g[1];
    d[2] = g[2];
    d[3] = copysign(g[3] * g[3], g[3]);
    sph_r[i] = g[3];
  } else if (i < ns + nm) {
    const int j = i - ns;
    const double *g = gm + (size_t)j * 8;
    double *d = mov + (size_t)j * 8;
    d[0] = g[0];
    d[1] = g[1];
    d[2] = g[2];
    d[3] = g[3] - g[0];
    d[4] = g[4] - g[1];
    d[5] = g[5] - g[2];
    d[6] = copysign(g[6] * g[6], g[6]);
    d[7] = g[6];
  } else {
    const int j = i - ns - nm;
    const double *g = gt + (size_t)j * 9;
    const double e1[3] = {g[3] - g[0], g[4] - g[1], g[5] - g[2]};
    const double e2[3] = {g[6] - g[0], g[7] - g[1], g[8] - g[2]};
    double r[12];
    r[0] = g[0];
    r[1] = g[1];
    r[2] = g[2];
    for (int k = 0; k < 3; ++k) {
      r[3 + k] = e1[k];
      r[6 + k] = e2[k];
    }
    r[9] = e1[1] * e2[2] - e2[1] * e1[2];
    r[10] = e1[2] * e2[0] - e2[2] * e1[0];
    r[11] = e1[0] * e2[1] - e2[0] * e1[1];
    for (int k = 0; k < 12; ++k) tri[(size_t)j * 12 + k] = r[k];
    if (tri16)
      for (int k = 0; k < 12; ++k) tri16[(size_t)j * 16 + k] = r[k];
  }
}

// padded binary64 primitive boxes from the records, class-major (build_bvh's bounds, then pad_box)
__global__ void kr_prim_boxes(const double *sph, const double *sph_r, const double *mov, const double *tri, int ns, int nm,
                              int nt, double time0, double time1, double *pbox) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns + nm + nt) return;
  double b[6];
  if (i < ns) {
    const double r = fabs(sph_r[i]);
    for (int k = 0; k < 3; ++k) {
      b[k] = sph[(size_t)i * 4 + k] - r;
      b[3 + k] = sph[(size_t)i * 4 + k] + r;
    }
  } else if (i < ns + nm) {
    const double *m = mov + (size_t)(i - ns) * 8;
    const double r = fabs(m[7]);
    const double w = 1e-6 * (1.0 + fabs(time0) + fabs(time1));
    const double ta = hmin(time0, time1) - w, tb = hmax(time0, time1) + w;
    for (int k = 0; k < 3; ++k) {
      const double a0 = m[k] + ta * m[3 + k], a1 = m[k] + tb * m[3 + k];
      b[k] = hmin(a0, a1) - r;
      b[3 + k] = hmax(a0, a1) + r;
    }
  } else {
    const double *t = tri + (size_t)(i - ns - nm) * 12;
    for (int k = 0; k < 3; ++k) {
      const double a = t[k], bb = t[k] + t[3 + k], c = t[k] + t[6 + k];
      b[k] = hmin(a, hmin(bb, c));
      b[3 + k] = hmax(a, hmax(bb, c));
    }
  }
  for (int k = 0; k < 3; ++k) {  // bvh_detail::pad_box
    const double ext = hmax(fabs(b[k]), fabs(b[3 + k]));
    const double pad = 1e-9 * (1.0 + ext);
    b[k] -= pad;
    b[3 + k] += pad;
  }
  for (int k = 0; k < 6; ++k) pbox[(size_t)i * 6 + k] = b[k];
}

// ---- record sections of the images ---------------------------------------------------------------------------------
// triangle records (binary64, or binary32 for the f32 build's images) and their material indices, slot s holding
// triangle map[s] (NULL: class order); off_pmat == ~0u: no material section to write
__global__ void kr_tri_section(int nt, const double *tri, const int32_t *pmat_tri, const int32_t *map, unsigned char *dst,
                               uint32_t off_tri, uint32_t off_pmat, int f32) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nt) return;
  const int src = map ? map[s] : s;
  if (src < 0 || src >= nt) return;
  const double *r = tri + (size_t)src * 12;
  if (f32) {
    float *d = reinterpret_cast<float *>(dst + off_tri) + (size_t)s * 12;
    for (int k = 0; k < 12; ++k) d[k] = (float)r[k];
  } else {
    double *d = reinterpret_cast<double *>(dst + off_tri) + (size_t)s * 12;
    for (int k = 0; k < 12; ++k) d[k] = r[k];
  }
  if (off_pmat != ~0u) reinterpret_cast<int32_t *>(dst + off_pmat)[s] = pmat_tri[src];
}
// the f32 build's binary32 sphere and moving records (make_image32 in rtow_capi.cpp)
__global__ void kr_spheres32(int ns, int nm, const double *sph, const double *mov, unsigned char *dst, uint32_t off_sph32,
                             uint32_t off_mov32) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns + nm) return;
  if (i < ns) {
    float *d = reinterpret_cast<float *>(dst + off_sph32) + (size_t)i * 4;
    for (int k = 0; k < 4; ++k) d[k] = (float)sph[(size_t)i * 4 + k];
  } else {
    const int j = i - ns;
    float *d = reinterpret_cast<float *>(dst + off_mov32) + (size_t)j * 8;
    for (int k = 0; k < 7; ++k) d[k] = (float)mov[(size_t)j * 8 + k];
    d[7] = 0.0f;
  }
}

// ---- binary BVH (threaded depth-first: inner node i has children i + 1 and skip(i + 1)) ---------------------------
__device__ __forceinline__ uint32_t node_word(const unsigned char *blob, int i, int w) {
  return reinterpret_cast<const uint32_t *>(blob + (size_t)i * 32)[6 + w];  // 0 skip, 1 leaf
}
__global__ void kr_bvh2_links(const unsigned char *blob, int n, int32_t *parent) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == 0) parent[0] = -1;
  if (node_word(blob, i, 1) != 0u || i + 1 >= n) return;
  const uint32_t r = node_word(blob, i + 1, 0);
  parent[i + 1] = i;
  if (r < (uint32_t)n) parent[r] = i;
}
// leaf boxes from the primitive boxes, then up: the second arrival at a node unions its two children
__global__ void kr_bvh2_up(const unsigned char *blob, int n, uint32_t off_ids, int n_ids, const int32_t *map, int cls_base,
                           const double *pbox, const int32_t *parent, uint32_t *flags, double *nbox) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t leaf = node_word(blob, i, 1);
  if (leaf == 0u) return;
  const int32_t *ids = reinterpret_cast<const int32_t *>(blob + off_ids);
  double b[6];
  box_empty(b);
  const uint32_t first = leaf >> 3, cnt = leaf & 7u;
  for (uint32_t k = 0; k < cnt && first + k < (uint32_t)n_ids; ++k) {
    const int id = ids[first + k];
    box_grow(b, pbox + (size_t)(map ? cls_base + map[id] : id) * 6);
  }
  for (int k = 0; k < 6; ++k) nbox[(size_t)i * 6 + k] = b[k];
  int node = parent[i];
  while (node >= 0) {
    __threadfence();
    const uint32_t old = atomicAdd(&flags[node], 1u);
    if (old == 0u) return;  // first arrival: the sibling's thread finishes this node
    __threadfence();
    const int l = node + 1, r = (int)node_word(blob, l, 0);
    double bl[6], br[6];
    box_load_agent(bl, nbox + (size_t)l * 6);
    box_load_agent(br, nbox + (size_t)r * 6);
    box_grow(bl, br);
    for (int k = 0; k < 6; ++k) nbox[(size_t)node * 6 + k] = bl[k];
    node = parent[node];
  }
}
// make_scene_image's planes: pad, round to binary32, one more step outwards; skip and leaf words untouched
__global__ void kr_bvh2_emit(unsigned char *blob, int n, const double *nbox, double ox, double oy, double oz) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double scale = pad_scale(nbox, ox, oy, oz);
  float *rec = reinterpret_cast<float *>(blob + (size_t)i * 32);
  for (int k = 0; k < 3; ++k) {
    const double lo = nbox[(size_t)i * 6 + k], hi = nbox[(size_t)i * 6 + 3 + k];
    const double pad = plane_pad(scale, lo, hi);
    rec[k] = nextafterf((float)(lo - pad), -INFINITY);
    rec[3 + k] = nextafterf((float)(hi + pad), INFINITY);
  }
}
// sum of the inner nodes' half-areas: per-block partials in a fixed order, then one block divides by the root's
__global__ void kr_area_partial(const unsigned char *blob, int n, const double *nbox, double *partials) {
  __shared__ double sh[kB];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  sh[threadIdx.x] = (i < n && node_word(blob, i, 1) == 0u) ? half_area(nbox + (size_t)i * 6) : 0.0;
  __syncthreads();
  for (int w = kB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}
__global__ void kr_area_final(const double *partials, int n_part, const double *nbox, double *out) {
  __shared__ double sh[kB];
  double s = 0.0;
  for (int j = threadIdx.x; j < n_part; j += kB) s += partials[j];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = kB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double root = half_area(nbox);
    out[0] = root > 0.0 ? sh[0] / root : 0.0;
  }
}

// ---- 4-wide BVH (breadth-first: a child's index is larger than its parent's) ---------------------------------------
__device__ __forceinline__ const uint32_t *child_words(const unsigned char *blob4, int j, uint32_t node_bytes,
                                                       uint32_t child_off) {
  return reinterpret_cast<const uint32_t *>(blob4 + (size_t)j * node_bytes + child_off);
}
__global__ void kr_bvh4_links(const unsigned char *blob4, int n4, uint32_t node_bytes, uint32_t child_off, int32_t *parent,
                              int32_t *need) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n4) return;
  if (j == 0) parent[0] = -1;
  const uint32_t *cw = child_words(blob4, j, node_bytes, child_off);
  int cnt = 0;
  for (int c = 0; c < 4; ++c) {
    const uint32_t w = cw[c];
    if (w == kRefNone || (w & kRefLeaf) || w >= (uint32_t)n4) continue;
    parent[w] = j;
    ++cnt;
  }
  need[j] = cnt;  // inner children to wait for
}
// the box of every child slot (sbox) and of every node (nbox): nodes without inner children start, the last arrival
// at a node finishes it
__global__ void kr_bvh4_up(const unsigned char *blob4, int n4, uint32_t node_bytes, uint32_t child_off, int n_rec,
                           const int32_t *map, int cls_base, const double *pbox, const int32_t *parent, const int32_t *need,
                           uint32_t *flags, double *nbox, double *sbox) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n4 || need[j] != 0) return;
  for (;;) {
    const uint32_t *cw = child_words(blob4, j, node_bytes, child_off);
    double u[6];
    box_empty(u);
    for (int c = 0; c < 4; ++c) {
      const uint32_t w = cw[c];
      if (w == kRefNone) continue;
      double b[6];
      if (w & kRefLeaf) {
        box_empty(b);
        const uint32_t first = (w & (kRefLeaf - 1u)) >> 2, cnt = (w & 3u) + 1u;
        for (uint32_t k = 0; k < cnt && first + k < (uint32_t)n_rec; ++k)
          box_grow(b, pbox + (size_t)(cls_base + map[first + k]) * 6);
      } else {
        box_load_agent(b, nbox + (size_t)w * 6);
      }
      for (int k = 0; k < 6; ++k) sbox[((size_t)j * 4 + c) * 6 + k] = b[k];
      box_grow(u, b);
    }
    for (int k = 0; k < 6; ++k) nbox[(size_t)j * 6 + k] = u[k];
    const int p = parent[j];
    if (p < 0) return;
    __threadfence();
    const uint32_t old = atomicAdd(&flags[p], 1u);
    if ((int)old + 1 < need[p]) return;
    __threadfence();
    j = p;
  }
}
// make_bvh4_image's frame of the binary16 planes, from the new root box: frame = map_c[3], map_s[3]
__global__ void kr_bvh4_frame(const double *nbox, int half, double *frame) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double *b = nbox;
  for (int k = 0; k < 3; ++k) {
    frame[k] = 0.0;
    frame[3 + k] = 1.0;
  }
  if (!half) return;
  const double widest = hmax(hmax(b[3] - b[0], b[4] - b[1]), b[5] - b[2]);
  for (int k = 0; k < 3; ++k) {
    const double lo = b[k], hi = b[3 + k];
    const double half_k = hmax(hmax(0.5 * (hi - lo), 1e-4 * widest), 1e-30);
    frame[k] = 0.5 * (lo + hi);
    frame[3 + k] = 1000.0 / half_k;
  }
}
__global__ void kr_bvh4_emit(unsigned char *blob4, int n4, uint32_t node_bytes, uint32_t child_off, int half,
                             const double *nbox, const double *sbox, const double *frame, double ox, double oy, double oz) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n4) return;
  const double scale = pad_scale(nbox, ox, oy, oz);
  unsigned char *node = blob4 + (size_t)j * node_bytes;
  const uint32_t *cw = reinterpret_cast<const uint32_t *>(node + child_off);
  float *f = reinterpret_cast<float *>(node);
  uint16_t *h = reinterpret_cast<uint16_t *>(node);
  for (int c = 0; c < 4; ++c) {
    if (cw[c] == kRefNone) continue;
    const double *b = sbox + ((size_t)j * 4 + c) * 6;
    for (int k = 0; k < 3; ++k) {
      const double lo = b[k], hi = b[3 + k];
      const double pad = plane_pad(scale, lo, hi);
      if (half) {
        h[k * 8 + c] = half_directed((lo - pad - frame[k]) * frame[3 + k], -1);
        h[k * 8 + 4 + c] = half_directed((hi + pad - frame[k]) * frame[3 + k], +1);
      } else {
        f[k * 8 + c] = nextafterf((float)(lo - pad), -INFINITY);
        f[k * 8 + 4 + c] = nextafterf((float)(hi + pad), INFINITY);
      }
    }
  }
}

inline unsigned blocks(long long n) { return (unsigned)((n + kB - 1) / kB); }
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

}  // namespace

// Host entry points (rtow_capi.cpp): every one enqueues on `stream` and returns 0 or 1 (a launch failed).
int refit_records(const double *g_sph, const double *g_mov, const double *g_tri, int ns, int nm, int nt, double *sph,
                  double *sph_r, double *mov, double *tri, double *tri16, void *stream) {
  hipLaunchKernelGGL(kr_records, dim3(blocks(ns + nm + nt)), dim3(kB), 0, (hipStream_t)stream, g_sph, g_mov, g_tri, ns, nm,
                     nt, sph, sph_r, mov, tri, tri16);
  return launched();
}

int refit_prim_boxes(const double *sph, const double *sph_r, const double *mov, const double *tri, int ns, int nm, int nt,
                     double time0, double time1, double *pbox, void *stream) {
  hipLaunchKernelGGL(kr_prim_boxes, dim3(blocks(ns + nm + nt)), dim3(kB), 0, (hipStream_t)stream, sph, sph_r, mov, tri, ns,
                     nm, nt, time0, time1, pbox);
  return launched();
}

int refit_tri_section(int nt, const double *tri, const int32_t *pmat_tri, const int32_t *map, unsigned char *dst,
                      uint32_t off_tri, uint32_t off_pmat, int f32, void *stream) {
  if (nt <= 0) return 0;
  hipLaunchKernelGGL(kr_tri_section, dim3(blocks(nt)), dim3(kB), 0, (hipStream_t)stream, nt, tri, pmat_tri, map, dst, off_tri,
                     off_pmat, f32);
  return launched();
}

int refit_spheres32(int ns, int nm, const double *sph, const double *mov, unsigned char *dst, uint32_t off_sph32,
                    uint32_t off_mov32, void *stream) {
  if (ns + nm <= 0) return 0;
  hipLaunchKernelGGL(kr_spheres32, dim3(blocks(ns + nm)), dim3(kB), 0, (hipStream_t)stream, ns, nm, sph, mov, dst, off_sph32,
                     off_mov32);
  return launched();
}

int refit_bvh2_links(const unsigned char *blob, int n_nodes, int32_t *parent, void *stream) {
  hipLaunchKernelGGL(kr_bvh2_links, dim3(blocks(n_nodes)), dim3(kB), 0, (hipStream_t)stream, blob, n_nodes, parent);
  return launched();
}

// Node boxes of the binary BVH (nbox [n][6]); with `emit`, its planes; the area sum into area_out[0].  flags: n words,
// partials: blocks(n) doubles.
int refit_bvh2(unsigned char *blob, int n_nodes, uint32_t off_ids, int n_ids, const int32_t *map, int cls_base,
               const double *pbox, const int32_t *parent, uint32_t *flags, double *nbox, double *partials, int emit,
               const double cam_origin[3], double *area_out, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(flags, 0, (size_t)n_nodes * 4, st) != hipSuccess) return 1;
  hipLaunchKernelGGL(kr_bvh2_up, dim3(blocks(n_nodes)), dim3(kB), 0, st, blob, n_nodes, off_ids, n_ids, map, cls_base, pbox,
                     parent, flags, nbox);
  if (emit)
    hipLaunchKernelGGL(kr_bvh2_emit, dim3(blocks(n_nodes)), dim3(kB), 0, st, blob, n_nodes, nbox, cam_origin[0],
                       cam_origin[1], cam_origin[2]);
  hipLaunchKernelGGL(kr_area_partial, dim3(blocks(n_nodes)), dim3(kB), 0, st, blob, n_nodes, nbox, partials);
  hipLaunchKernelGGL(kr_area_final, dim3(1), dim3(kB), 0, st, partials, (int)blocks(n_nodes), nbox, area_out);
  return launched();
}

int refit_bvh4_links(const unsigned char *blob4, int n4, uint32_t node_bytes, uint32_t child_off, int32_t *parent,
                     int32_t *need, void *stream) {
  hipLaunchKernelGGL(kr_bvh4_links, dim3(blocks(n4)), dim3(kB), 0, (hipStream_t)stream, blob4, n4, node_bytes, child_off,
                     parent, need);
  return launched();
}

// Boxes and planes of the 4-wide image; frame (6 doubles) receives map_c, map_s of the binary16 planes (0 / 1 for
// binary32 planes).  flags: n4 words; nbox [n4][6]; sbox [n4][4][6].
int refit_bvh4(unsigned char *blob4, int n4, uint32_t node_bytes, uint32_t child_off, int half, int n_rec, const int32_t *map,
               int cls_base, const double *pbox, const int32_t *parent, const int32_t *need, uint32_t *flags, double *nbox,
               double *sbox, const double cam_origin[3], double *frame, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(flags, 0, (size_t)n4 * 4, st) != hipSuccess) return 1;
  hipLaunchKernelGGL(kr_bvh4_up, dim3(blocks(n4)), dim3(kB), 0, st, blob4, n4, node_bytes, child_off, n_rec, map, cls_base,
                     pbox, parent, need, flags, nbox, sbox);
  hipLaunchKernelGGL(kr_bvh4_frame, dim3(1), dim3(64), 0, st, nbox, half, frame);
  hipLaunchKernelGGL(kr_bvh4_emit, dim3(blocks(n4)), dim3(kB), 0, st, blob4, n4, node_bytes, child_off, half, nbox, sbox,
                     frame, cam_origin[0], cam_origin[1], cam_origin[2]);
  return launched();
}

}  // namespace rtow
