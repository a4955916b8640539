// rtow_kernel_launch.h — the host side of the kernel frame (rtow_kernel_frame.h): how one instantiation of a render or
// query kernel is launched, and how many of its workgroups stay resident per CU.  Included inside `namespace rtow {`,
// after the kernels' anonymous namespace, by rtow_trace_body.h and by every query family's header (rtow_query.h,
// rtow_occlude.h, rtow_pointq.h, rtow_first_hits.h, rtow_nearest.h, rtow_radiance.h, rtow_step.h, rtow_guides.h).
#pragma once

// The kernels address the dynamic LDS block from 0 (lds_read / lds_write, rtow_trace_math.h): an instantiation that had
// static LDS of its own would read the wrong bytes.
static int no_static_lds(const void *fn) {
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, fn);
  if (e != hipSuccess) return (int)e;
  return fa.sharedSizeBytes == 0 ? 0 : (int)hipErrorInvalidValue;
}

// Launches the instantiation `Kernel`: 0 or a hipError_t.  The static LDS check is made once per instantiation, on the
// kernel that is actually launched (the kernel is a template argument: one static each).
template <auto Kernel, class Params>
static int launch_kernel(const Params &p, int grid, int block, unsigned lds_bytes, hipStream_t st) {
  const void *fn = reinterpret_cast<const void *>(Kernel);
  static const int lds_ok = no_static_lds(fn);
  if (lds_ok != 0) return lds_ok;
  if (lds_bytes > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds_bytes, st, p);
  return (int)hipGetLastError();
}

// One instantiation of a kernel family as its `switch (kernel)` picked it, for the launch and for the occupancy
// question alike: `lds_bytes` is the dynamic LDS it is launched with (0 for a variant that uses none).
template <class Params>
struct KernelVariant {
  const void *fn = nullptr;  // nullptr: no such kernel
  int (*launch)(const Params &, int grid, int block, unsigned lds_bytes, hipStream_t) = nullptr;
  unsigned lds_bytes = 0;
};
template <auto Kernel, class Params>
static KernelVariant<Params> kernel_variant(unsigned lds_bytes) {
  return {reinterpret_cast<const void *>(Kernel), &launch_kernel<Kernel, Params>, lds_bytes};
}

// The end of every launcher: launches `v` as its family's `switch (kernel)` picked it, or fails where it picked none.
template <class Params>
static int launch_variant(const KernelVariant<Params> &v, const Params &p, int grid, int block, void *stream) {
  return v.fn ? v.launch(p, grid, block, v.lds_bytes, (hipStream_t)stream) : (int)hipErrorInvalidValue;
}

// Workgroups per CU that stay resident, or -1: min over the register file (512 VGPRs per SIMD lane, allocated in
// granules of 8; at most 8 waves per SIMD), the four SIMDs and the 160 KiB of LDS.  `*vgprs` (optional) receives the
// kernel's register count.
// (The runtime's occupancy query ignores LDS above 64 KiB per CU on this stack; a grid that turns out larger than
// resident only queues the surplus workgroups, which then find no work left — there is no inter-workgroup dependency.)
static int resident_blocks(const void *fn, int block, unsigned lds_bytes, int *vgprs) {
  if (fn == nullptr) return -1;
  if (lds_bytes > 48 * 1024) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return -1;
  if (fa.sharedSizeBytes != 0) return -1;
  const int regs = fa.numRegs > 0 ? fa.numRegs : 128;
  if (vgprs) *vgprs = regs;
  const int alloc = ((regs + 7) / 8) * 8;
  int waves_per_simd = 512 / alloc;
  if (waves_per_simd > 8) waves_per_simd = 8;
  if (waves_per_simd < 1) waves_per_simd = 1;
  int nb = (waves_per_simd * 4) / (block / 64);
  if (lds_bytes > 0) {
    const int by_lds = (int)((160u * 1024u) / lds_bytes);
    if (by_lds < nb) nb = by_lds;
  }
  return nb < 1 ? 1 : nb;
}
