// GLIGEN (diffusers PositionNet + GatedSelfAttentionDense): the PositionNet's input rows, once per call.  Its MLP, the fusers' linear / K / V
// projections and the gated self-attention are the UNet's igemm, LayerNorm and attention launches (attention.hip, EXTRA = 1).
#include "kernels.h"

static inline int grid_for(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// one row per object (rows = B2 * max_objs), ld >= P + 8 F columns:
//   [0, P)          m pos + (1 - m) null_pos                               (positive_embeddings, null replacement)
//   [P, P + 8 F)    m fourier + (1 - m) null_xyxy, fourier[f * 8 + s * 4 + k] = (s ? cos : sin)(100^(f / F) box[k])
//   [P + 8 F, ld)   0 (the igemm reads whole 64-column chunks)
__global__ void gligen_posnet_input_kernel(const float* __restrict__ boxes, const float* __restrict__ pos, const float* __restrict__ masks,
                                           const float* __restrict__ null_pos, const float* __restrict__ null_xyxy, bf16_t* __restrict__ out,
                                           int rows, int P, int F, int ld) {
  const long long total = (long long)rows * ld;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(i % ld);
    const int r = (int)(i / ld);
    const float m = masks[r];
    float v = 0.f;
    if (col < P) {
      v = pos[(long long)r * P + col] * m + (1.f - m) * null_pos[col];
    } else if (col < P + 8 * F) {
      const int j = col - P, f = j >> 3, s = (j >> 2) & 1, k = j & 3;
      const float e = powf(100.f, (float)f / (float)F) * boxes[(long long)r * 4 + k];
      v = (s ? cosf(e) : sinf(e)) * m + (1.f - m) * null_xyxy[j];
    }
    out[i] = f2bf(v);
  }
}
int launch_gligen_posnet_input(const float* boxes, const float* pos, const float* masks, const float* null_pos, const float* null_xyxy,
                               bf16_t* out, int rows, int P, int F, int ld, hipStream_t st) {
  if (rows < 1 || P < 1 || F < 1 || ld < P + 8 * F) return -1;
  hipLaunchKernelGGL(gligen_posnet_input_kernel, dim3(grid_for((long long)rows * ld)), dim3(256), 0, st, boxes, pos, masks, null_pos, null_xyxy,
                     out, rows, P, F, ld);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
