// DeepCache (Ma, Fang, Wang 2024, "DeepCache: Accelerating Diffusion Models for Free"; the upstream DeepCacheSDHelper [upstream-knowledge]): the
// capture of a full evaluation.  The hidden state that enters up layer U_{b+1} and its GroupNorm partial sums leave the activation arena -- which
// the next walk releases -- for the context's persistent slot.  The shallow walk reads the slot in place; everything else it runs is the UNet
// walk's own launches.
#include "kernels.h"

// Two byte regions, one launch: words [0, w0) of region 0, then words [0, w1) of region 1, one 16-byte load and store per thread and trip,
// grid-stride over w0 + w1 words; the up to 15 bytes behind each region's last whole word go one byte per thread of workgroup 0.  Nothing is
// converted: the slot holds the source's bits.
__global__ __launch_bounds__(256) void deepcache_capture_kernel(const uint4* __restrict__ s0, uint4* __restrict__ d0, long long w0, int t0,
                                                                const uint4* __restrict__ s1, uint4* __restrict__ d1, long long w1, int t1) {
  const long long total = w0 + w1;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (i < w0) d0[i] = s0[i];
    else d1[i - w0] = s1[i - w0];
  }
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < t0) ((unsigned char*)(d0 + w0))[t] = ((const unsigned char*)(s0 + w0))[t];
    else if (t >= 16 && t - 16 < t1) ((unsigned char*)(d1 + w1))[t - 16] = ((const unsigned char*)(s1 + w1))[t - 16];
  }
}

int launch_deepcache_capture(const void* src0, void* dst0, long long bytes0, const void* src1, void* dst1, long long bytes1, hipStream_t st) {
  if (bytes0 < 0 || bytes1 < 0 || bytes0 + bytes1 < 1) { agd_set_error("deepcache_capture: %lld + %lld bytes", bytes0, bytes1); return -1; }
  if ((bytes0 > 0 && (!src0 || !dst0)) || (bytes1 > 0 && (!src1 || !dst1))) { agd_set_error("deepcache_capture: null argument"); return -1; }
  if (bytes0 == 0) src0 = dst0 = nullptr;
  if (bytes1 == 0) src1 = dst1 = nullptr;
  if ((((uintptr_t)src0 | (uintptr_t)dst0 | (uintptr_t)src1 | (uintptr_t)dst1) & 15) != 0) {
    agd_set_error("deepcache_capture: every region must start on a 16-byte boundary"); return -1; }
  const long long w0 = bytes0 / 16, w1 = bytes1 / 16, total = w0 + w1;
  long long g = (total + 255) / 256; g = g < 1 ? 1 : (g > 8192 ? 8192 : g);
  hipLaunchKernelGGL(deepcache_capture_kernel, dim3((int)g), dim3(256), 0, st, (const uint4*)src0, (uint4*)dst0, w0, (int)(bytes0 - w0 * 16),
                     (const uint4*)src1, (uint4*)dst1, w1, (int)(bytes1 - w1 * 16));
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
