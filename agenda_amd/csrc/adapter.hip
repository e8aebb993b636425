// T2I-Adapter (diffusers T2IAdapter "full_adapter" + StableDiffusionAdapterPipeline) kernels: the once-per-call front end (pixel unshuffle of
// the conditioning image), the 2x2 average pool and the ReLU of the adapter network, and the per-evaluation add of a feature map to a UNet
// down block's output.  The adapter's convolutions are the UNet's igemm launches.
#include "kernels.h"

static inline int grid_for(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// PixelUnshuffle(r) of the conditioning image into the model input, one thread per output element: out bf16 NHWC [B][H/r * W/r][Cpad],
// channel c r^2 + i r + j of pixel (h, w) = image channel c at (h r + i, w r + j), zero above C r^2.  image: uint8 NHWC [B][H][W][C]
// (x / 255 in fp32) or, image_f32, fp32 NCHW [B][C][H][W] already in [0,1].
__global__ void adapter_front_kernel(const void* __restrict__ image, int image_f32, int B, int H, int W, int C, int r, int Cpad,
                                     bf16_t* __restrict__ out) {
  const int Lh = H / r, Lw = W / r, r2 = r * r, Cu = C * r2;
  const long long total = (long long)B * Lh * Lw * Cpad;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % Cpad);
    const long long px = i / Cpad;
    float v = 0.f;
    if (k < Cu) {
      const int w = (int)(px % Lw), h = (int)((px / Lw) % Lh), b = (int)(px / ((long long)Lw * Lh));
      const int c = k / r2, ij = k - c * r2, ii = ij / r, jj = ij - ii * r;
      const long long y = (long long)h * r + ii, x = (long long)w * r + jj;
      if (image_f32) v = ((const float*)image)[(((long long)b * C + c) * H + y) * W + x];
      else v = (float)((const unsigned char*)image)[(((long long)b * H + y) * W + x) * C + c] / 255.0f;
    }
    out[i] = f2bf(v);
  }
}
int launch_adapter_front(const void* image, int image_f32, int B, int H, int W, int C, int r, int Cpad, bf16_t* out, hipStream_t st) {
  if (B < 1 || C < 1 || r < 1 || H < r || W < r || H % r || W % r || C * r * r > Cpad) {
    agd_set_error("adapter front end: batch %d, %d channels, size %d x %d, downscale factor %d, %d padded channels", B, C, H, W, r, Cpad); return -1; }
  hipLaunchKernelGGL(adapter_front_kernel, dim3(grid_for((long long)B * (H / r) * (W / r) * Cpad)), dim3(256), 0, st, image, image_f32, B, H, W, C, r,
                     Cpad, out);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// AvgPool2d(2, 2) on bf16 NHWC [B][H][W][C] -> [B][H/2][W/2][C]: one thread per 8 channels of an output pixel, the four inputs summed in
// fp32 and rounded once
__global__ void adapter_avgpool_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int B, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, nv = C / 8;
  const long long total = (long long)B * Ho * Wo * nv;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int v = (int)(i % nv);
    const long long px = i / nv;
    const int wo = (int)(px % Wo), ho = (int)((px / Wo) % Ho), b = (int)(px / ((long long)Wo * Ho));
    const bf16_t* s = x + (((long long)b * H + 2 * ho) * W + 2 * wo) * C + v * 8;
    const s16x8 a0 = *(const s16x8*)s, a1 = *(const s16x8*)(s + C), a2 = *(const s16x8*)(s + (long long)W * C), a3 = *(const s16x8*)(s + (long long)W * C + C);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.25f * ((bf2f((bf16_t)a0[e]) + bf2f((bf16_t)a1[e])) + (bf2f((bf16_t)a2[e]) + bf2f((bf16_t)a3[e])));
    u32x4 pk;
    pk[0] = pack_bf2(o[0], o[1]); pk[1] = pack_bf2(o[2], o[3]); pk[2] = pack_bf2(o[4], o[5]); pk[3] = pack_bf2(o[6], o[7]);
    *(u32x4*)(y + px * C + v * 8) = pk;
  }
}
int launch_adapter_avgpool(const bf16_t* x, bf16_t* y, int B, int H, int W, int C, hipStream_t st) {
  if (B < 1 || H < 2 || W < 2 || H % 2 || W % 2 || C < 8 || C % 8) { agd_set_error("adapter avgpool: batch %d map %d x %d x %d", B, H, W, C); return -1; }
  hipLaunchKernelGGL(adapter_avgpool_kernel, dim3(grid_for((long long)B * (H / 2) * (W / 2) * (C / 8))), dim3(256), 0, st, x, y, B, H, W, C);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// x = max(x, 0) in place over n8 vectors of 8 bf16 (a set sign bit -> +0)
__global__ void adapter_relu_kernel(bf16_t* __restrict__ x, long long n8) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    u32x4 v = *(u32x4*)(x + i * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned w = v[e];
      if (w & 0x00008000u) w &= 0xFFFF0000u;
      if (w & 0x80000000u) w &= 0x0000FFFFu;
      v[e] = w;
    }
    *(u32x4*)(x + i * 8) = v;
  }
}
int launch_adapter_relu(bf16_t* x, long long n, hipStream_t st) {
  if (n < 8 || n % 8) { agd_set_error("adapter relu: %lld elements (a multiple of 8)", n); return -1; }
  hipLaunchKernelGGL(adapter_relu_kernel, dim3(grid_for(n / 8)), dim3(256), 0, st, x, n / 8);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// The per-evaluation add: y = bf16(h + s f) for h bf16 NHWC [M = B2 HW][C] and f fp32 [Bf][HW][C], row m of image b = m / HW reading
// feature image b % Bf.  A workgroup owns a tile of bm rows x VC vectors of 8 channels; thread (rg, vc) walks the tile's rows rg, rg + RG, ..
// (RG = 256 / VC) with 16-byte loads and stores.  STATS: the workgroup also leaves the GroupNorm partial sums of its tile, part [M / bm][C]
// float2 = (sum, sum of squares) of the bf16-ROUNDED outputs -- the igemm epilogue's colstat_out layout.  Each thread sums its rows in row
// order, then one thread per channel sums the RG row groups in ascending order out of LDS: a fixed order, no atomics, bit-identical runs.
template <bool STATS>
__global__ __launch_bounds__(256) void adapter_add_kernel(const bf16_t* __restrict__ h, const float* __restrict__ f, bf16_t* __restrict__ y,
                                                          float* __restrict__ part, int M, int HW, int C, int Bf, int bm, int VC, float s) {
  __shared__ float red[STATS ? 256 * 16 : 1];
  const int tid = threadIdx.x, vc = tid % VC, rg = tid / VC, RG = 256 / VC;
  const int ch = (blockIdx.y * VC + vc) * 8;
  const int r0 = blockIdx.x * bm, r1 = min(M, r0 + bm);
  float sum[8], sq[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sum[e] = 0.f; sq[e] = 0.f; }
  for (int r = r0 + rg; r < r1; r += RG) {
    const int b = r / HW, p = r - b * HW;
    const float* fp = f + ((long long)(b % Bf) * HW + p) * C + ch;
    const s16x8 hv = *(const s16x8*)(h + (long long)r * C + ch);
    const f32x4 f0 = *(const f32x4*)fp, f1 = *(const f32x4*)(fp + 4);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(s, e < 4 ? f0[e & 3] : f1[e & 3], bf2f((bf16_t)hv[e]));
    u32x4 pk;
    pk[0] = pack_bf2(o[0], o[1]); pk[1] = pack_bf2(o[2], o[3]); pk[2] = pack_bf2(o[4], o[5]); pk[3] = pack_bf2(o[6], o[7]);
    *(u32x4*)(y + (long long)r * C + ch) = pk;
    if constexpr (STATS) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float v = __uint_as_float(e & 1 ? pk[e >> 1] & 0xFFFF0000u : pk[e >> 1] << 16); sum[e] += v; sq[e] += v * v; }
    }
  }
  if constexpr (STATS) {
    // red[rg][vc * 8 + e] as (sum, sum of squares): the final pass reads consecutive words across its threads
    const int W8 = VC * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[2 * (rg * W8 + vc * 8 + e)] = sum[e]; red[2 * (rg * W8 + vc * 8 + e) + 1] = sq[e]; }
    __syncthreads();
    if (tid < W8) {
      float a = 0.f, q = 0.f;
      for (int k = 0; k < RG; ++k) { a += red[2 * (k * W8 + tid)]; q += red[2 * (k * W8 + tid) + 1]; }
      float* dst = part + ((long long)blockIdx.x * C + blockIdx.y * W8 + tid) * 2;
      dst[0] = a; dst[1] = q;
    }
  }
}
int launch_adapter_add(const bf16_t* h, const float* f, bf16_t* y, float* part, int bm, int B2, int HW, int C, int Bf, float s, hipStream_t st) {
  const long long M = (long long)B2 * HW;
  if (B2 < 1 || HW < 1 || Bf < 1 || C < 8 || C % 8 || M >= (1ll << 30)) { agd_set_error("adapter add: %d rows of %d pixels x %d channels, %d feature images", B2, HW, C, Bf); return -1; }
  if (part && (bm < 1 || HW % bm)) { agd_set_error("adapter add: %d-row statistics tiles on maps of %d pixels", bm, HW); return -1; }
  const int nvec = C / 8, VC = nvec % 8 == 0 ? 8 : nvec % 4 == 0 ? 4 : nvec % 2 == 0 ? 2 : 1;
  const int tile = part ? bm : 64;
  const dim3 grid((unsigned)((M + tile - 1) / tile), (unsigned)(nvec / VC));
  if (part) hipLaunchKernelGGL(adapter_add_kernel<true>, grid, dim3(256), 0, st, h, f, y, part, (int)M, HW, C, Bf, tile, VC, s);
  else hipLaunchKernelGGL(adapter_add_kernel<false>, grid, dim3(256), 0, st, h, f, y, part, (int)M, HW, C, Bf, tile, VC, s);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
