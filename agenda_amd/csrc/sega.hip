// Semantic Guidance (Brack et al. 2023, "SEGA: Instructing Text-to-Image Models using Semantic Guidance"; diffusers 0.21.2
// SemanticStableDiffusionPipeline [upstream-knowledge]): the two device pieces of a SEGA evaluation.  eps is fp32 NHWC
// [(2 + K) B][HW][4]: uncond x B | cond x B | concept_0 x B | ... | concept_{K-1} x B.  Per (image b, concept k) v = (e_k - e_u) coef_k, the
// threshold is the exact q_k-quantile of |v| over the HW pixels of every channel, and the fold adds the thresholded, weighted directions (and
// the momentum) to both rows the schedulers' two-way step kernels read.  The UNet walks and the step kernels are the txt2img launches.
#include "kernels.h"

#define SEGA_TPB 1024                 // 16 waves: the (image, concept) pairs of a call are few, so one pair's passes are what takes time
#define SEGA_HIST (4 * 256)           // one 256-bin histogram per channel
#define SEGA_CTL 16                   // [0, 4) the selected bit pattern, [4, 8) whether b is the minimum above a, [8, 12) that minimum
#define SEGA_HEAD_BYTES ((SEGA_HIST + SEGA_CTL) * 4)

void sega_rank(double q, int HW, int* lo, float* f) {
  const double p = q * (double)(HW - 1);
  double l = floor(p);
  if (l < 0) l = 0;
  if (l > HW - 1) l = HW - 1;
  *lo = (int)l; *f = (float)(p - l);
}
int sega_staged(int HW) { return HW <= SEGA_STAGE_MAX_HW; }

// |v| of one pixel's four channels as bit patterns: non-negative floats order as unsigned integers (NaN above +inf)
__device__ __forceinline__ uint4 sega_abs_bits(const float4 ek, const float4 eu, const float coef) {
#pragma clang fp contract(off)
  uint4 r;
  r.x = __float_as_uint((ek.x - eu.x) * coef) & 0x7fffffffu; r.y = __float_as_uint((ek.y - eu.y) * coef) & 0x7fffffffu;
  r.z = __float_as_uint((ek.z - eu.z) * coef) & 0x7fffffffu; r.w = __float_as_uint((ek.w - eu.w) * coef) & 0x7fffffffu;
  return r;
}

// One workgroup per (image, concept).  Radix select, 8 bits a pass from the top: per channel the histogram of the next digit among the values
// that share the digits selected so far (integer LDS atomics only: the counts, so the result, do not depend on the order of arrival), then
// wave c scans channel c's 256 bins for the one that holds rank lo.  After four passes the pattern of a (the lo-th smallest) is complete and
// the last bin's count says how many values equal a: b (the next rank) is a itself while the tie reaches it, else the minimum of the values
// above a (one more pass, a wave-reduced minimum and one integer atomic per wave).  STAGED: the patterns sit in LDS after the first read;
// otherwise every pass reads the two rows again (through L2) and recomputes them.
template <bool STAGED>
__global__ __launch_bounds__(SEGA_TPB) void sega_threshold_kernel(const float* __restrict__ eps, int B, int K, int HW, SegaEvalP p, float* __restrict__ thr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* hist = reinterpret_cast<unsigned*>(smem);
  unsigned* ctl = hist + SEGA_HIST;
  uint4* slab = reinterpret_cast<uint4*>(smem + SEGA_HEAD_BYTES);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x / K, k = blockIdx.x - b * K;
  float coef = 0.f, frac = 0.f; int lo = 0;
#pragma unroll
  for (int j = 0; j < AGD_MAX_EDIT_CONCEPTS; ++j) if (j == k) { coef = p.coef[j]; frac = p.f[j]; lo = p.lo[j]; }
  float* out = thr + (long long)blockIdx.x * 4;
  if (coef == 0.f) {                                              // an inactive concept: its rows may be stale and are not read
    if (tid < 4) out[tid] = 0.f;
    return;
  }
  const float4* eu = reinterpret_cast<const float4*>(eps) + (long long)b * HW;
  const float4* ek = reinterpret_cast<const float4*>(eps) + ((long long)(2 + k) * B + b) * HW;
  if (STAGED) for (int px = tid; px < HW; px += SEGA_TPB) slab[px] = sega_abs_bits(ek[px], eu[px], coef);
  unsigned pre = 0, r = (unsigned)lo, cnt = 0;                    // waves 0 .. 3: channel `wave`'s selected digits, rank among what shares them, last bin's count
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    hist[tid] = 0;                                                // SEGA_TPB == SEGA_HIST
    __syncthreads();                                              // (also: the slab is written, ctl of the pass before is visible)
    const unsigned p0 = ctl[0] & himask, p1 = ctl[1] & himask, p2 = ctl[2] & himask, p3 = ctl[3] & himask;   // (pass 0: masked to 0, ctl not yet written)
    for (int px = tid; px < HW; px += SEGA_TPB) {
      const uint4 v = STAGED ? slab[px] : sega_abs_bits(ek[px], eu[px], coef);
      if ((v.x & himask) == p0) atomicAdd(&hist[0 * 256 + ((v.x >> shift) & 255u)], 1u);
      if ((v.y & himask) == p1) atomicAdd(&hist[1 * 256 + ((v.y >> shift) & 255u)], 1u);
      if ((v.z & himask) == p2) atomicAdd(&hist[2 * 256 + ((v.z >> shift) & 255u)], 1u);
      if ((v.w & himask) == p3) atomicAdd(&hist[3 * 256 + ((v.w >> shift) & 255u)], 1u);
    }
    __syncthreads();
    if (wave < 4) {
      const unsigned* h = hist + wave * 256 + lane * 4;
      const unsigned h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
      const unsigned s = h0 + h1 + h2 + h3;
      unsigned incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
      const unsigned excl = incl - s;
      const unsigned long long hit = __ballot(excl <= r && r < incl);   // exactly one lane: the bins' counts sum to more than r
      const int sel = hit ? __ffsll((long long)hit) - 1 : 63;
      unsigned bin = lane * 4, nr = r - excl, c = h0;
      if (nr >= h0) { nr -= h0; bin++; c = h1;
        if (nr >= h1) { nr -= h1; bin++; c = h2;
          if (nr >= h2) { nr -= h2; bin++; c = h3; } } }
      bin = __shfl(bin, sel, 64); r = __shfl(nr, sel, 64); cnt = __shfl(c, sel, 64);
      pre |= bin << shift;
      if (lane == 0) ctl[wave] = pre;
    }
    __syncthreads();
  }
  // b: rank min(lo + 1, HW - 1).  It is a while lo is the last rank or the values equal to a reach rank lo + 1.
  if (wave < 4 && lane == 0) { ctl[4 + wave] = (lo < HW - 1 && r + 1 >= cnt) ? 1u : 0u; ctl[8 + wave] = 0xffffffffu; }
  __syncthreads();
  const unsigned a0 = ctl[0], a1 = ctl[1], a2 = ctl[2], a3 = ctl[3];
  const bool n0 = ctl[4] != 0, n1 = ctl[5] != 0, n2 = ctl[6] != 0, n3 = ctl[7] != 0;
  if (n0 || n1 || n2 || n3) {                                     // (uniform over the workgroup)
    unsigned m0 = 0xffffffffu, m1 = 0xffffffffu, m2 = 0xffffffffu, m3 = 0xffffffffu;
    for (int px = tid; px < HW; px += SEGA_TPB) {
      const uint4 v = STAGED ? slab[px] : sega_abs_bits(ek[px], eu[px], coef);
      if (v.x > a0 && v.x < m0) m0 = v.x;
      if (v.y > a1 && v.y < m1) m1 = v.y;
      if (v.z > a2 && v.z < m2) m2 = v.z;
      if (v.w > a3 && v.w < m3) m3 = v.w;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned t0 = __shfl_xor(m0, d, 64), t1 = __shfl_xor(m1, d, 64), t2 = __shfl_xor(m2, d, 64), t3 = __shfl_xor(m3, d, 64);
      m0 = t0 < m0 ? t0 : m0; m1 = t1 < m1 ? t1 : m1; m2 = t2 < m2 ? t2 : m2; m3 = t3 < m3 ? t3 : m3;
    }
    if (lane == 0) {
      if (n0) atomicMin(&ctl[8], m0);
      if (n1) atomicMin(&ctl[9], m1);
      if (n2) atomicMin(&ctl[10], m2);
      if (n3) atomicMin(&ctl[11], m3);
    }
    __syncthreads();
  }
  if (tid < 4) {
#pragma clang fp contract(off)
    const float a = __uint_as_float(ctl[tid]);
    const float bb = ctl[4 + tid] ? __uint_as_float(ctl[8 + tid]) : a;
    const float t = a + frac * (bb - a);
    out[tid] = a == bb ? a : fminf(bb, t);                        // (a == b: thr is a exactly, whatever frac)
  }
}

int launch_sega_threshold(const float* eps, int B, int K, int C, int HW, const SegaEvalP& p, float* thr, hipStream_t st) {
  if (!eps || !thr) { agd_set_error("sega_threshold: null argument"); return -1; }
  if (C != 4) { agd_set_error("sega_threshold: %d latent channels (the kernel reads rows of 4 fp32 channels, out_channels = 4)", C); return -1; }
  if (B < 1 || K < 1 || K > AGD_MAX_EDIT_CONCEPTS || HW < 1) { agd_set_error("sega_threshold: %d images, %d concepts (1 .. %d), %d pixels", B, K, AGD_MAX_EDIT_CONCEPTS, HW); return -1; }
  if ((long long)(2 + K) * B * HW > (1ll << 40)) { agd_set_error("sega_threshold: %d rows of %d pixels", (2 + K) * B, HW); return -1; }
  if (((uintptr_t)eps & 15) || ((uintptr_t)thr & 15)) { agd_set_error("sega_threshold: eps and thr must start on 16-byte boundaries"); return -1; }
  for (int k = 0; k < K; ++k) {
    if (!std::isfinite(p.coef[k])) { agd_set_error("sega_threshold: coef %d is %g (a finite number)", k, (double)p.coef[k]); return -1; }
    // f == 1 is a value sega_rank gives: float(p - lo) rounds up to 1 where q (HW - 1) in double lands a few ulp below an integer; thr is then b
    if (p.lo[k] < 0 || p.lo[k] > HW - 1 || !(p.f[k] >= 0.f && p.f[k] <= 1.f)) { agd_set_error("sega_threshold: concept %d: rank %d + %g of %d pixels", k, p.lo[k], (double)p.f[k], HW); return -1; }
  }
  if (sega_staged(HW)) {
    const size_t lds = SEGA_HEAD_BYTES + (size_t)HW * 16;
    static std::atomic<bool> attr[AGD_MAX_DEVICES] = {};
    int dev = 0; HIP_CHECK_RET(hipGetDevice(&dev));
    if (dev < 0 || dev >= AGD_MAX_DEVICES) { agd_set_error("sega_threshold: device ordinal %d out of range", dev); return -1; }
    if (!attr[dev]) { HIP_CHECK_RET(hipFuncSetAttribute((const void*)sega_threshold_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        SEGA_HEAD_BYTES + SEGA_STAGE_MAX_HW * 16)); attr[dev] = true; }
    hipLaunchKernelGGL(sega_threshold_kernel<true>, dim3(B * K), dim3(SEGA_TPB), lds, st, eps, B, K, HW, p, thr);
  } else {
    hipLaunchKernelGGL(sega_threshold_kernel<false>, dim3(B * K), dim3(SEGA_TPB), SEGA_HEAD_BYTES, st, eps, B, K, HW, p, thr);
  }
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// One thread per (image, pixel): the four channels of e_u, e_c, m and of every active concept's row with 16-byte loads.
//   G_k = v_k where |v_k| >= thr[b][k][c] else 0 (a NaN v_k: 0);   g = sum_k w_mom[k] G_k + mu m;   added = sum_k w_add[k] G_k + add_mom mu m
//   m <- beta m + (1 - beta) g;   e_u += added, e_c += added (left as they are, bit for bit, where added == 0)
// Every product and sum is rounded on its own (no fused multiply-add), in ascending k: the fp32 expressions of any IEEE host.
__global__ __launch_bounds__(256) void sega_fold_kernel(float* __restrict__ eps, float* __restrict__ mom, const float* __restrict__ thr, int B, int K, int HW,
                                                        SegaEvalP p, float mu, float beta, float add_mom) {
#pragma clang fp contract(off)
  const long long total = (long long)B * HW;
  float4* e4 = reinterpret_cast<float4*>(eps); float4* m4 = reinterpret_cast<float4*>(mom); const float4* t4 = reinterpret_cast<const float4*>(thr);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW);
    const float4 eu = e4[i], ec = e4[total + i], m = m4[i];
    float4 gm = make_float4(0.f, 0.f, 0.f, 0.f), ga = gm;
#pragma unroll
    for (int k = 0; k < AGD_MAX_EDIT_CONCEPTS; ++k) {
      if (k >= K || p.coef[k] == 0.f) continue;
      const float4 ek = e4[(long long)(2 + k) * total + i], t = t4[b * K + k];
      const float c = p.coef[k], wm = p.w_mom[k], wa = p.w_add[k];
      float v;
      v = (ek.x - eu.x) * c; v = fabsf(v) >= t.x ? v : 0.f; gm.x = gm.x + wm * v; ga.x = ga.x + wa * v;
      v = (ek.y - eu.y) * c; v = fabsf(v) >= t.y ? v : 0.f; gm.y = gm.y + wm * v; ga.y = ga.y + wa * v;
      v = (ek.z - eu.z) * c; v = fabsf(v) >= t.z ? v : 0.f; gm.z = gm.z + wm * v; ga.z = ga.z + wa * v;
      v = (ek.w - eu.w) * c; v = fabsf(v) >= t.w ? v : 0.f; gm.w = gm.w + wm * v; ga.w = ga.w + wa * v;
    }
    const float omb = 1.f - beta;
    const float4 mm = make_float4(mu * m.x, mu * m.y, mu * m.z, mu * m.w);
    const float4 g = make_float4(gm.x + mm.x, gm.y + mm.y, gm.z + mm.z, gm.w + mm.w);
    const float4 ad = make_float4(ga.x + add_mom * mm.x, ga.y + add_mom * mm.y, ga.z + add_mom * mm.z, ga.w + add_mom * mm.w);
    m4[i] = make_float4(beta * m.x + omb * g.x, beta * m.y + omb * g.y, beta * m.z + omb * g.z, beta * m.w + omb * g.w);
    if (ad.x != 0.f || ad.y != 0.f || ad.z != 0.f || ad.w != 0.f) {
      e4[i] = make_float4(ad.x != 0.f ? eu.x + ad.x : eu.x, ad.y != 0.f ? eu.y + ad.y : eu.y, ad.z != 0.f ? eu.z + ad.z : eu.z, ad.w != 0.f ? eu.w + ad.w : eu.w);
      e4[total + i] = make_float4(ad.x != 0.f ? ec.x + ad.x : ec.x, ad.y != 0.f ? ec.y + ad.y : ec.y, ad.z != 0.f ? ec.z + ad.z : ec.z, ad.w != 0.f ? ec.w + ad.w : ec.w);
    }
  }
}

int launch_sega_fold(float* eps, float* mom, const float* thr, int B, int K, int C, int HW, const SegaEvalP& p, float mu, float beta, float add_mom, hipStream_t st) {
  if (!eps || !mom || !thr) { agd_set_error("sega_fold: null argument"); return -1; }
  if (C != 4) { agd_set_error("sega_fold: %d latent channels (the kernel reads rows of 4 fp32 channels, out_channels = 4)", C); return -1; }
  if (B < 1 || K < 1 || K > AGD_MAX_EDIT_CONCEPTS || HW < 1) { agd_set_error("sega_fold: %d images, %d concepts (1 .. %d), %d pixels", B, K, AGD_MAX_EDIT_CONCEPTS, HW); return -1; }
  if (((uintptr_t)eps & 15) || ((uintptr_t)mom & 15) || ((uintptr_t)thr & 15)) { agd_set_error("sega_fold: eps, m and thr must start on 16-byte boundaries"); return -1; }
  if (!std::isfinite(mu) || !std::isfinite(beta) || !std::isfinite(add_mom)) { agd_set_error("sega_fold: momentum scale %g, beta %g, add_mom %g (finite numbers)", (double)mu, (double)beta, (double)add_mom); return -1; }
  for (int k = 0; k < K; ++k)
    if (!std::isfinite(p.coef[k]) || !std::isfinite(p.w_mom[k]) || !std::isfinite(p.w_add[k])) { agd_set_error("sega_fold: concept %d: coef %g, weights %g / %g (finite numbers)", k, (double)p.coef[k], (double)p.w_mom[k], (double)p.w_add[k]); return -1; }
  const long long total = (long long)B * HW;
  long long g = (total + 255) / 256; if (g > 8192) g = 8192;
  hipLaunchKernelGGL(sega_fold_kernel, dim3((int)g), dim3(256), 0, st, eps, mom, thr, B, K, HW, p, mu, beta, add_mom);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
