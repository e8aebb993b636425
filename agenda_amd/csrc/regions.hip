// Region-based MultiDiffusion (Bar-Tal et al. 2023, the MultiDiffusion repository's region_based.py [upstream-knowledge]) byte movers: the
// mask front end that brings pixel masks to the latent size, the spread that hands the one canvas to every region (bootstrapped against a
// constant-colour background for the first steps), and the masked mean that fuses the stepped regions back into the canvas.  The UNet,
// the CFG + DDIM step and the per-region DAAM states are the txt2img launches.
//
// Row (region r, image p) is image r * B + p everywhere: masks [R][B][Lh * Lw] (one value per latent pixel, shared by the channels), the
// region buffer x [R][B][C][Lh * Lw], both fp32.  Region 0 is the background.
#include "kernels.h"

// The spread and the mean state their roundings (tests/_regions_restated.py does the same sums in torch, bit for bit): no product is
// contracted into the sum that follows it.  The pragma governs the operators written in this file (not the bodies of header intrinsics),
// so the sums below are written with * and +.
#pragma clang fp contract(off)

static inline int grid_for(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g)); }

template <int VEC> struct VecT { typedef float type; };
template <> struct VecT<4> { typedef f32x4 type; };

__device__ inline float mask_bit(unsigned char v) { return v > 127 ? 1.f : 0.f; }
__device__ inline float mask_bit(float v) { return v > 0.5f ? 1.f : 0.f; }

// One thread per latent pixel of one image: latent (y, x) reads pixel (fy y, fx x) of every foreground mask (torch's nearest sample at an
// integer ratio), thresholds it, writes row r * B + p, and writes the background row max(0, 1 - their sum).  px [Bm][R - 1][H][W] with
// Bm = 1 (shared by the images) or B.
template <typename T>
__global__ void region_masks_kernel(const T* __restrict__ px, float* __restrict__ masks, int R, int B, int per_image, int H, int W, int Lh,
                                    int Lw, int fy, int fx) {
  const long long HW = (long long)Lh * Lw, total = (long long)B * HW;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long i = t % HW;
    const int p = (int)(t / HW), y = (int)(i / Lw), x = (int)(i - (long long)y * Lw);
    float sum = 0.f;
    for (int r = 1; r < R; ++r) {
      const long long img = (long long)(per_image ? p : 0) * (R - 1) + (r - 1);
      const float m = mask_bit(px[(img * H + (long long)y * fy) * W + (long long)x * fx]);
      masks[((long long)r * B + p) * HW + i] = m;
      sum += m;
    }
    masks[(long long)p * HW + i] = fmaxf(0.f, 1.f - sum);
  }
}

// One thread per VEC elements of x [R][B][C][HW].  Region 0, and every region of a step that is not bootstrapped, is the canvas; otherwise
//   x = canvas m + (sa bg[idx[r]] + sb noise) (1 - m),
// every product and sum rounded on its own (no contraction), so a covered element (m = 1) is the canvas bit for bit.
template <int VEC>
__global__ void region_spread_kernel(const float* __restrict__ canvas, float* __restrict__ x, const float* __restrict__ masks,
                                     const float* __restrict__ noise, const float* __restrict__ bgs, int R, int B, int C, long long HW,
                                     int boot, RegionIdx idx, float sa, float sb) {
  typedef typename VecT<VEC>::type V;
  const long long hwv = HW / VEC, total = (long long)R * B * C * hwv;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long i = (t % hwv) * VEC;
    long long q = t / hwv;
    const int c = (int)(q % C); q /= C;
    const int p = (int)(q % B), r = (int)(q / B);
    const long long src = ((long long)p * C + c) * HW + i;
    V v = *(const V*)(canvas + src);
    if (boot && r > 0) {
      const V m = *(const V*)(masks + ((long long)r * B + p) * HW + i);
      const V n = *(const V*)(noise + src);
      const V g = *(const V*)(bgs + ((long long)idx.v[r] * C + c) * HW + i);
      auto one = [&](float cv, float mv, float nv, float gv) {
        const float bgn = sa * gv + sb * nv;
        return cv * mv + bgn * (1.f - mv);
      };
      if constexpr (VEC == 4) { for (int k = 0; k < 4; ++k) v[k] = one(v[k], m[k], n[k], g[k]); }
      else v = one(v, m, n, g);
    }
    *(V*)(x + t * VEC) = v;
  }
}

// One thread per VEC canvas elements: sum_r m_r x_r / sum_r m_r, both sums in ascending r in fp32 with every product and sum rounded on its
// own, one division per element -- no atomics, no value / count buffers.  Where no mask covers the element the result is the sum itself, 0
// (upstream's `where(count > 0, value / count, value)`).
template <int VEC>
__global__ void region_mean_kernel(const float* __restrict__ x, const float* __restrict__ masks, float* __restrict__ canvas, int R, int B,
                                   int C, long long HW) {
  typedef typename VecT<VEC>::type V;
  const long long hwv = HW / VEC, total = (long long)B * C * hwv;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long i = (t % hwv) * VEC;
    long long q = t / hwv;
    const int c = (int)(q % C), p = (int)(q / C);
    V sum = {}, den = {};
    for (int r = 0; r < R; ++r) {
      const long long row = (long long)r * B + p;
      const V m = *(const V*)(masks + row * HW + i);
      const V v = *(const V*)(x + (row * C + c) * HW + i);
      if constexpr (VEC == 4) { for (int k = 0; k < 4; ++k) { sum[k] = sum[k] + m[k] * v[k]; den[k] = den[k] + m[k]; } }
      else { sum = sum + m * v; den = den + m; }
    }
    if constexpr (VEC == 4) { for (int k = 0; k < 4; ++k) if (den[k] > 0.f) sum[k] = __fdiv_rn(sum[k], den[k]); }
    else { if (den > 0.f) sum = __fdiv_rn(sum, den); }
    *(V*)(canvas + t * VEC) = sum;
  }
}

static bool vec4_ok(long long HW, std::initializer_list<const void*> ptrs) {
  if (HW % 4) return false;
  for (const void* p : ptrs) if ((uintptr_t)p & 15) return false;
  return true;
}

static int check_shape(const char* what, int R, int B, int C, long long HW) {
  if (R < 1 || R > AGD_MAX_REGIONS || B < 1 || C < 1 || HW < 1) {
    agd_set_error("%s: %d regions (1 .. %d), batch %d, channels %d, %lld latent pixels", what, R, AGD_MAX_REGIONS, B, C, HW);
    return -1;
  }
  return 0;
}

int launch_region_masks(const void* px, int px_f32, int per_image, float* masks, int R, int B, int H, int W, int Lh, int Lw, hipStream_t st) {
  if (Lh < 1 || Lw < 1) { agd_set_error("region_masks: latent size %d x %d", Lh, Lw); return -1; }
  if (check_shape("region_masks", R, B, 1, (long long)Lh * Lw)) return -1;
  if (!masks || (R > 1 && !px)) { agd_set_error("region_masks: null argument"); return -1; }
  if (R > 1 && (H < Lh || W < Lw || H % Lh || W % Lw)) { agd_set_error("region_masks: pixel size %d x %d is no whole multiple of the latent size %d x %d", H, W, Lh, Lw); return -1; }
  const int fy = R > 1 ? H / Lh : 1, fx = R > 1 ? W / Lw : 1;
  const int grid = grid_for((long long)B * Lh * Lw);
  if (px_f32) hipLaunchKernelGGL(region_masks_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)px, masks, R, B, per_image, H, W, Lh, Lw, fy, fx);
  else hipLaunchKernelGGL(region_masks_kernel<unsigned char>, dim3(grid), dim3(256), 0, st, (const unsigned char*)px, masks, R, B, per_image, H, W, Lh, Lw, fy, fx);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

int launch_region_spread(const float* canvas, float* x, const float* masks, const float* noise, const float* bgs, int R, int B, int C,
                         long long HW, int n_bg, int boot, RegionIdx idx, float sa, float sb, hipStream_t st) {
  if (check_shape("region_spread", R, B, C, HW)) return -1;
  boot = boot && R > 1;
  if (!canvas || !x || (boot && (!masks || !noise || !bgs))) { agd_set_error("region_spread: null argument"); return -1; }
  if (boot) for (int r = 1; r < R; ++r) if (idx.v[r] < 0 || idx.v[r] >= n_bg) {
    agd_set_error("region_spread: background index %d of region %d outside 0 .. %d", idx.v[r], r, n_bg - 1); return -1; }
  const long long total = (long long)R * B * C * HW;
  if (vec4_ok(HW, {canvas, x, masks, noise, bgs}))
    hipLaunchKernelGGL(region_spread_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, st, canvas, x, masks, noise, bgs, R, B, C, HW, boot, idx, sa, sb);
  else
    hipLaunchKernelGGL(region_spread_kernel<1>, dim3(grid_for(total)), dim3(256), 0, st, canvas, x, masks, noise, bgs, R, B, C, HW, boot, idx, sa, sb);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

int launch_region_mean(const float* x, const float* masks, float* canvas, int R, int B, int C, long long HW, hipStream_t st) {
  if (check_shape("region_mean", R, B, C, HW)) return -1;
  if (!x || !masks || !canvas) { agd_set_error("region_mean: null argument"); return -1; }
  const long long total = (long long)B * C * HW;
  if (vec4_ok(HW, {x, masks, canvas}))
    hipLaunchKernelGGL(region_mean_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, st, x, masks, canvas, R, B, C, HW);
  else
    hipLaunchKernelGGL(region_mean_kernel<1>, dim3(grid_for(total)), dim3(256), 0, st, x, masks, canvas, R, B, C, HW);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
