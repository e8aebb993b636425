// LoRA merge (agd_lora_set_scale, model.hip): W = bf16(float(W_base) + s * (alpha / r) * up @ down), written straight into the
// engine's packed raw layout [N][Cpad] (1x1: taps = 1) with a zero Cpad tail, and for ff.net.0.proj in convert_weight_kernel's
// [8 values | 8 gates] row interleave (geglu_bn = 16).  up @ down is summed in fp32 from the fp32 factors (VALU fmaf, r in order);
// the rounding is f2bf, as launch_convert_weight's.  One launch covers every target of a group: 64 x 64 output tiles, numbered
// target after target (LoraMergeD::tile0), so every touched matrix is read once (W_base) and written once (W).
#include "kernels.h"

namespace {
constexpr int kT = 64;      // output tile: kT rows x kT columns, 256 threads of 4 x 4 outputs
constexpr int kR = 16;      // rank steps staged in LDS at a time
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraMergeD* __restrict__ d, int n_desc, float s, int copy_only) {
  // the target of this tile: the last descriptor whose first tile is <= blockIdx.x
  int lo = 0, hi = n_desc - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (d[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
  const LoraMergeD t = d[lo];
  const int tile = (int)blockIdx.x - t.tile0, ctiles = (t.Cpad + kT - 1) / kT;
  const int n0 = (tile / ctiles) * kT, c0 = (tile % ctiles) * kT;
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  float acc[4][4] = {};
  if (!copy_only) {
    __shared__ float sU[kT][kR + 1];
    __shared__ float sD[kR][kT];
    for (int r0 = 0; r0 < t.r; r0 += kR) {
      for (int e = tid; e < kT * kR; e += 256) {
        const int i = e / kR, k = e % kR, n = n0 + i, rk = r0 + k;
        float v = 0.f;
        if (n < t.N && rk < t.r) {
          int src = n;                                            // convert_weight_kernel's GEGLU interleave
          if (t.geglu) { const int half = t.geglu / 2, j = n / t.geglu, wi = n % t.geglu; src = wi < half ? j * half + wi : t.N / 2 + j * half + (wi - half); }
          v = t.up[(long long)src * t.r + rk];
        }
        sU[i][k] = v;
      }
      for (int e = tid; e < kR * kT; e += 256) {
        const int k = e / kT, j = e % kT, col = c0 + j, rk = r0 + k;
        sD[k][j] = (rk < t.r && col < t.Cin) ? t.down[(long long)rk * t.Cin + col] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kR; ++k) {
        float u[4], w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = sU[tr * 4 + i][k];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = sD[k][tc * 4 + j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(u[i], w[j], acc[i][j]);
      }
      __syncthreads();
    }
  }
  const float k = s * t.coef;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + tr * 4 + i;
    if (n >= t.N) continue;
    const long long row = (long long)n * t.Cpad;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c0 + tc * 4 + j;
      if (col >= t.Cpad) continue;
      if (col >= t.Cin) { t.dst[row + col] = f2bf(0.f); continue; }
      const bf16_t b = t.base[row + col];
      t.dst[row + col] = copy_only ? b : f2bf(bf2f(b) + k * acc[i][j]);
    }
  }
}

int lora_merge_tiles(int N, int Cpad) { return ((N + kT - 1) / kT) * ((Cpad + kT - 1) / kT); }

int launch_lora_merge(const LoraMergeD* d, int n_desc, int total_tiles, float s, int copy_only, hipStream_t st) {
  if (n_desc <= 0 || total_tiles <= 0) return 0;
  hipLaunchKernelGGL(lora_merge_kernel, dim3(total_tiles), dim3(256), 0, st, d, n_desc, s, copy_only);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
