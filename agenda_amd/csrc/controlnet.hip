// ControlNet byte movers (agd_controlnet_set_cond / the per-evaluation scale): the conditioning image's layout change and the
// scaled zero-conv biases.  The ControlNet's convs, resnets and transformers are the UNet's igemm / GroupNorm / attention launches.
#include "kernels.h"

static inline int grid_for(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// cond fp32 NCHW [B][3][HW] -> bf16 NHWC [B][HW][Cpad], channels zero-padded (the igemm steps K in 64-channel chunks); bgr: channel c reads
// source channel 2 - c
__global__ void controlnet_cond_prep_kernel(const float* __restrict__ cond, bf16_t* __restrict__ out, int B, int HW, int Cpad, int bgr) {
  const long long total = (long long)B * HW * Cpad;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cpad);
    const long long px = i / Cpad;
    const int p = (int)(px % HW);
    const int b = (int)(px / HW);
    const int sc = bgr ? 2 - c : c;
    out[i] = f2bf(c < 3 ? cond[((long long)b * 3 + sc) * HW + p] : 0.f);
  }
}
int launch_controlnet_cond_prep(const float* cond, bf16_t* out, int B, int HW, int Cpad, int bgr, hipStream_t st) {
  if (Cpad < 3) return -1;
  hipLaunchKernelGGL(controlnet_cond_prep_kernel, dim3(grid_for((long long)B * HW * Cpad)), dim3(256), 0, st, cond, out, B, HW, Cpad, bgr);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// out[i] = s * in[i]: the zero convs' biases at this evaluation's conditioning scale (the igemm epilogue scales the accumulator by
// alpha and adds the bias as given)
__global__ void controlnet_scale_bias_kernel(const float* __restrict__ in, float* __restrict__ out, int n, float s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = s * in[i];
}
int launch_controlnet_scale_bias(const float* in, float* out, int n, float s, hipStream_t st) {
  if (n < 1) return 0;
  hipLaunchKernelGGL(controlnet_scale_bias_kernel, dim3((n + 255) / 256), dim3(256), 0, st, in, out, n, s);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
