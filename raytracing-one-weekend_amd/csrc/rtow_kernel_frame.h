// rtow_kernel_frame.h — what the render kernels (rtow_trace_body.h, rtow_trace_sm4.h) and the query kernels
// (rtow_query.h, rtow_occlude.h, rtow_first_hits.h, rtow_pointq.h, rtow_radiance.h, rtow_guides.h) share around their
// walks: the lane index, the scene image staged in LDS, the read of a caller's ray and the two test counters every
// query reports.  Device pieces only, every one __forceinline__; included inside
// `namespace rtow { namespace {` after rtow_trace_math.h, rtow_trace_bvh.h and rtow_trace_bvh4.h, the way the walk
// headers are.  The host side of the frame is rtow_kernel_launch.h.
#pragma once

// how many of the lanes in `mask` lie below this one
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ unsigned lane_id() { return lanes_below(~0ull); }

// The 4-wide image: its first b4_lds_limit bytes go to LDS offset 0 (the whole image when FULL, else the top of its
// tree), its end (materials, material indices: 16-byte aligned sections) to b4_aux_lds.  Coalesced 16-byte loads,
// 16-byte LDS stores; ends in the workgroup's barrier.
template <bool FULL>
__device__ __forceinline__ void stage_bvh4(const DevScene &sc, Bvh4Reader<FULL> &im4) {
  im4.g = sc.blob4;
  im4.lds_limit = sc.b4_lds_limit;
  im4.aux_src = sc.b4_aux_src;
  im4.aux_lds = sc.b4_aux_lds;
  const uint4 *src = reinterpret_cast<const uint4 *>(sc.blob4);
  uint4 *dst = reinterpret_cast<uint4 *>(rtow_lds);
  const uint32_t n16 = sc.b4_lds_limit / 16u;
  for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
  if (sc.b4_aux_src < sc.blob4_bytes) {
    const uint4 *asrc = reinterpret_cast<const uint4 *>(sc.blob4 + sc.b4_aux_src);
    uint4 *adst = reinterpret_cast<uint4 *>(rtow_lds + sc.b4_aux_lds);
    const uint32_t a16 = (sc.blob4_bytes - sc.b4_aux_src) / 16u;
    for (uint32_t i = threadIdx.x; i < a16; i += blockDim.x) adst[i] = asrc[i];
  }
  __syncthreads();
}

// Points the readers at the scene and stages what the strategy keeps in LDS, from LDS offset 0 (where every walk reads
// it): KERNEL 4 the 4-wide image (above), KERNEL 2 / 3 with LDS the binary BVH / grid blob whole, otherwise nothing.
// A kernel family without a GRID or STREAM variant simply never instantiates those.
template <int KERNEL, bool LDS>
__device__ __forceinline__ void stage_scene(const DevScene &sc, Image<LDS> &im, Bvh4Reader<LDS> &im4) {
  im.g = KERNEL == 3 ? sc.gblob : sc.blob;
  if constexpr (KERNEL == 4) {
    stage_bvh4(sc, im4);
  } else if constexpr ((KERNEL == 2 || KERNEL == 3) && LDS) {
    const uint4 *src = reinterpret_cast<const uint4 *>(im.g);
    uint4 *dst = reinterpret_cast<uint4 *>(rtow_lds);
    const uint32_t n16 = (KERNEL == 3 ? sc.gblob_bytes : sc.blob_bytes) / 16u;
    for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
  }
}

constexpr uint32_t kRayBytes = 64u;  // rtow_ray_t, include/rtow.h

// (rtow_query.h keeps its own ray read and counter epilogue, the same statements written out: with these two helpers its
// code objects were no longer the measured ones — a few moves and waits reordered, two registers fewer and a fifth
// wave per SIMD in the fast GRID variant — and scripts/bench_query.py's sum came out 0.2 to 0.6 % slower, three calls
// out of three; profiles/README.md.)
// Ray `i` of a caller's array (16-byte aligned): four 16-byte loads, {ox, oy} {oz, time} {dx, dy} {dz, tmax} — the
// loads of a wave that reads 64 consecutive rays cover one contiguous 4 KiB run.
__device__ __forceinline__ void load_ray(const unsigned char *rays, size_t i, V3 &o, V3 &d, real &time, double &tmax) {
  const vd2 *r = reinterpret_cast<const vd2 *>(rays + i * kRayBytes);
  const vd2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
  o = {(real)r0.x, (real)r0.y, (real)r1.x};
  time = (real)r1.y;
  d = {(real)r2.x, (real)r2.y, (real)r3.x};
  tmax = r3.y;
}

// The wave's sum of v, in lane 0 (the kernels' statistics: one atomic per wave and counter).
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
  return v;
}

// The queries' statistics: counters[0] += primitive tests, counters[1] += node tests, one atomic per wave and counter.
__device__ __forceinline__ void flush_counters(unsigned long long *counters, uint32_t nprim, uint32_t nnode) {
  const unsigned long long c0 = wave_sum(nprim), c1 = wave_sum(nnode);
  if (lane_id() == 0) {
    atomicAdd(&counters[0], c0);
    atomicAdd(&counters[1], c1);
  }
}
