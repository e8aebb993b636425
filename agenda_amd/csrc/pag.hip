// Perturbed-Attention Guidance (Ahn et al. 2024, "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance"; diffusers >= 0.30
// StableDiffusionPAGPipeline [upstream-knowledge]): the two byte movers of the third, perturbed branch.  In an applied self-attention layer the
// attention map is the identity, so the layer's "attention" is its value rows; the branch's output is folded into the [uncond | cond] pair the
// schedulers' two-way step kernels take.  The UNet walk and the step kernels are the txt2img launches.
#include "kernels.h"

static inline int grid_for(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// att[m][0:C] = qkv[m][2C:3C]: one 16-byte load and store (8 bf16) per thread and trip, grid-stride over M C / 8.  C % 8 == 0 keeps every
// row start of both tensors 16-byte aligned (rows of 6 C and 2 C bytes, a value block at 4 C bytes).
__global__ void pag_v_rows_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ att, long long total, int C8) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long m = i / C8; const int j = (int)(i - m * C8);
    const uint4 v = *reinterpret_cast<const uint4*>(qkv + (m * 3 + 2) * C8 * 8 + (long long)j * 8);
    *reinterpret_cast<uint4*>(att + i * 8) = v;
  }
}
int launch_pag_v_rows(const bf16_t* qkv, bf16_t* att, int M, int C, hipStream_t st) {
  if (!qkv || !att) { agd_set_error("pag_v_rows: null argument"); return -1; }
  if (M < 1 || C < 8 || C % 8) { agd_set_error("pag_v_rows: %d rows of %d channels (C a positive multiple of 8: 16-byte loads and stores)", M, C); return -1; }
  if (((uintptr_t)qkv & 15) || ((uintptr_t)att & 15)) { agd_set_error("pag_v_rows: rows must start on 16-byte boundaries"); return -1; }
  const long long total = (long long)M * (C / 8);
  hipLaunchKernelGGL(pag_v_rows_kernel, dim3(grid_for(total)), dim3(256), 0, st, qkv, att, total, C / 8);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// The three-way guidance folded into a two-way one, in place.  eps fp32 [3][n]: e_uncond | e_cond | e_perturbed.  d = p (e_c - e_p) is added
// to both rows, so a two-way step with the text scale s gives (e_u + d) + s ((e_c + d) - (e_u + d)) = e_u + s (e_c - e_u) + p (e_c - e_p) up
// to rounding.  The product is rounded on its own (no fused multiply-add): both rows receive the same d, e_p == e_c leaves them untouched
// (d = +0), and the result is the fp32 expression e + p * (e_c - e_p) of any IEEE host.
__global__ void pag_fold_kernel(float* __restrict__ eps, long long n, float p) {
  // HIP's __fmul_rn / __fadd_rn are plain operators to the compiler: once inlined, the default -ffp-contract=fast fuses them into v_fmac.
  // The operators are therefore written here, under contract(off): v_sub, v_mul and two v_add, each rounded to nearest even.
#pragma clang fp contract(off)
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float eu = eps[i], ec = eps[n + i], ep = eps[2 * n + i];
    const float d = p * (ec - ep);
    eps[i] = eu + d;
    eps[n + i] = ec + d;
  }
}
int launch_pag_fold(float* eps, long long n, float p, hipStream_t st) {
  if (!eps || n < 1) { agd_set_error("pag_fold: null argument or %lld values", n); return -1; }
  if (!std::isfinite(p) || p < 0.f) { agd_set_error("pag_fold: scale %g (a finite number >= 0)", (double)p); return -1; }
  hipLaunchKernelGGL(pag_fold_kernel, dim3(grid_for(n)), dim3(256), 0, st, eps, n, p);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
