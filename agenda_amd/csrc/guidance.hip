// guidance_rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4; diffusers 0.21.2
// rescale_noise_cfg [upstream-knowledge]): the per-image factor that brings the CFG-combined prediction back to the text branch's spread,
//   m = eps_u + g (eps_c - eps_u),   f_b = phi std(eps_c[b]) / std(m[b]) + (1 - phi),   std over (C, H, W) jointly, unbiased.
// The step kernels (misc.hip) multiply m by f_b; this unit only computes f.
#include "kernels.h"

#define GR_THREADS 1024
#define GR_WAVES (GR_THREADS / 64)

// sum of one value per thread over the workgroup, the same bits in every thread: xor butterflies inside each wave, then the GR_WAVES wave
// sums added in wave order by every thread.  `red` is reused by the next call: the leading barrier waits for the previous call's readers.
__device__ __forceinline__ float gr_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < GR_WAVES; ++w) s += red[w];
  return s;
}

// One workgroup per image, two passes over that image's two eps halves (the second comes from L2: the UNet's last conv has just written
// them): pass 1 the means of m and eps_c, pass 2 the squared deviations from those means.  Thread t owns pixels t, t + 1024, ... and walks
// each one's C channels in order, so the order of every sum depends on (C, HW) alone -- not on B, on the grid or on timing.
// VEC: C == 4 with 16-B aligned rows, read as one float4 per half (the same values in the same order as the scalar walk).
template <bool VEC>
__global__ __launch_bounds__(GR_THREADS) void guidance_factor_kernel(const float* __restrict__ eps, int ldc, int B, int C, int HW, float guidance,
                                                                      float phi, float* __restrict__ factor) {
  __shared__ float red[GR_WAVES];
  const int b = blockIdx.x;
  const float* eu = eps + (long long)b * HW * ldc;
  const float* ec = eps + (long long)(b + B) * HW * ldc;
  const float n = (float)C * (float)HW;
  float sm = 0.f, sc = 0.f;
  for (int p = threadIdx.x; p < HW; p += GR_THREADS) {
    if (VEC) {
      const float4 u = *reinterpret_cast<const float4*>(eu + (long long)p * ldc), v = *reinterpret_cast<const float4*>(ec + (long long)p * ldc);
      const float uu[4] = {u.x, u.y, u.z, u.w}, vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) { sm += uu[c] + guidance * (vv[c] - uu[c]); sc += vv[c]; }
    } else {
      for (int c = 0; c < C; ++c) { const float u = eu[(long long)p * ldc + c], v = ec[(long long)p * ldc + c]; sm += u + guidance * (v - u); sc += v; }
    }
  }
  const float mean_m = gr_block_sum(sm, red) / n, mean_c = gr_block_sum(sc, red) / n;
  float qm = 0.f, qc = 0.f;
  for (int p = threadIdx.x; p < HW; p += GR_THREADS) {
    if (VEC) {
      const float4 u = *reinterpret_cast<const float4*>(eu + (long long)p * ldc), v = *reinterpret_cast<const float4*>(ec + (long long)p * ldc);
      const float uu[4] = {u.x, u.y, u.z, u.w}, vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) { const float dm = uu[c] + guidance * (vv[c] - uu[c]) - mean_m, dc = vv[c] - mean_c; qm += dm * dm; qc += dc * dc; }
    } else {
      for (int c = 0; c < C; ++c) {
        const float u = eu[(long long)p * ldc + c], v = ec[(long long)p * ldc + c];
        const float dm = u + guidance * (v - u) - mean_m, dc = v - mean_c; qm += dm * dm; qc += dc * dc;
      }
    }
  }
  const float M2m = gr_block_sum(qm, red), M2c = gr_block_sum(qc, red);
  // the (n - 1) of both unbiased variances cancels.  1 + phi (r - 1): exactly 1 at phi == 0 and at equal spreads; a constant m (std 0, where
  // diffusers divides by zero) gives 1 as well
  if (threadIdx.x == 0) factor[b] = M2m > 0.f ? 1.f + phi * (sqrtf(M2c / M2m) - 1.f) : 1.f;
}

int launch_guidance_factor(const float* eps, int ldc, int B, int C, int HW, float guidance, float phi, float* factor, hipStream_t st) {
  if (!eps || !factor) { agd_set_error("guidance rescale: null argument"); return -1; }
  if (B < 1 || C < 1 || HW < 1 || ldc < C || (long long)2 * B * HW * ldc >= (1ll << 40)) { agd_set_error("guidance rescale: %d images of %d x %d values in rows of %d", B, HW, C, ldc); return -1; }
  if ((long long)C * HW < 2) { agd_set_error("guidance rescale: an image of %d value has no standard deviation (C * HW >= 2)", C * HW); return -1; }
  if (!std::isfinite(guidance) || !std::isfinite(phi) || phi < 0.f || phi > 1.f) { agd_set_error("guidance rescale: guidance %g, phi %g (phi in [0, 1])", (double)guidance, (double)phi); return -1; }
  if (C == 4 && (ldc & 3) == 0 && ((uintptr_t)eps & 15) == 0)
    hipLaunchKernelGGL(guidance_factor_kernel<true>, dim3(B), dim3(GR_THREADS), 0, st, eps, ldc, B, C, HW, guidance, phi, factor);
  else
    hipLaunchKernelGGL(guidance_factor_kernel<false>, dim3(B), dim3(GR_THREADS), 0, st, eps, ldc, B, C, HW, guidance, phi, factor);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
