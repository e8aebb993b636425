// IP-Adapter (image prompts): the decoupled cross-attention of every UNet attn2 over the n_tok projected image tokens, as a rank
// (heads x n_tok) update of the residual stream beside the text attn2 launches.
//
// [upstream-knowledge] IP-Adapter (Ye et al. 2023) as diffusers >= 0.24 runs it (IPAdapterAttnProcessor, ImageProjection):
//     tokens = LayerNorm(Linear(image_embeds).reshape(B, n_tok, ctx_dim))
//     out    = to_out(attn(q, K_text, V_text) + s attn(q, to_k_ip(tokens), to_v_ip(tokens)))
// with q, the head split and 1 / sqrt(d) the text branch's own, and to_k_ip / to_v_ip without bias.
//
// The image tokens are fixed for a whole call, so (as xattn_pre.hip does for the text at C = 1280) everything that depends on them alone
// is multiplied out once per agd_ip_adapter_set; col = (head, token), cols = heads n_tok padded to a multiple of 16:
//     S[m][col]  = rstd_m (x[m] . K''[b][col] - mu_m cs[b][col]) + bs[b][col]          x = the raw attn2 input row (norm2 folded)
//         K''[b][col][c] = gamma2[c] scale sum_d k_ip[b][t][h D + d] Wq[h D + d][c]     cs = row sums of the bf16 K''
//         bs[b][col]     = scale sum_d k_ip[b][t][h D + d] (Wq beta2)[h D + d]
//     P          = softmax over each head's n_tok columns
//     h[m][n]   += s sum_col P[m][col] V''[b][n][col]        V''[b][n][col] = sum_d Wo[n][h D + d] v_ip[b][t][h D + d]
// to_out's bias belongs to the text branch (added once there).
//
// Kernels (gfx950, wave64):
//   ipa_linear_kernel / ipa_layernorm_kernel / ipa_kpp_kernel / ipa_csbs_kernel / ipa_vpp_kernel   once per call, a few thousand rows
//   ipa_scores_kernel   per forward and block: row statistics + S GEMM + softmax -> P (bf16)
//   ipa_add_kernel      per forward and block: h += s P V''^T in place
#include "kernels.h"

// y[r][n] = sum_k x[r][k] W[n][k] (+ bias[n]): fp32 rows against a bf16 matrix, one wave per output
__global__ __launch_bounds__(256) void ipa_linear_kernel(const float* __restrict__ x, const bf16_t* __restrict__ W, const float* __restrict__ bias,
                                                         float* __restrict__ y, int R, int N, int K) {
  const int lane = threadIdx.x & 63;
  const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= (long long)R * N) return;
  const int r = (int)(o / N), n = (int)(o - (long long)r * N);
  const float* xr = x + (long long)r * K; const bf16_t* wr = W + (long long)n * K;
  float a = 0.f;
  for (int k = lane; k < K; k += 64) a = fmaf(xr[k], bf2f(wr[k]), a);
  for (int s = 32; s >= 1; s >>= 1) a += __shfl_xor(a, s);
  if (lane == 0) y[o] = a + (bias ? bias[n] : 0.f);
}
int launch_ipa_linear(const float* x, const bf16_t* W, const float* bias, float* y, int R, int N, int K, hipStream_t st) {
  if (R < 1 || N < 1 || K < 1 || (long long)R * N >= (1ll << 31)) { agd_set_error("ipa linear: %d rows, [%d][%d]", R, N, K); return -1; }
  hipLaunchKernelGGL(ipa_linear_kernel, dim3((unsigned)(((long long)R * N + 3) / 4)), dim3(256), 0, st, x, W, bias, y, R, N, K);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// x[row] = LayerNorm(x[row]) in place, fp32, one wave per row (two passes: mean, then the centred variance)
__global__ __launch_bounds__(256) void ipa_layernorm_kernel(float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b, int rows, int C, float eps) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* xr = x + (long long)row * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  const float mu = s / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) { const float d = xr[c] - mu; q += d * d; }
  for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = rsqrtf(q / (float)C + eps);
  for (int c = lane; c < C; c += 64) xr[c] = (xr[c] - mu) * rstd * g[c] + b[c];
}
int launch_ipa_layernorm(float* x, const float* g, const float* b, int rows, int C, float eps, hipStream_t st) {
  if (rows < 1 || C < 1) { agd_set_error("ipa layernorm: %d rows of %d", rows, C); return -1; }
  hipLaunchKernelGGL(ipa_layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, g, b, rows, C, eps);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// K''[b][col][c] (bf16; rows col >= H nt: zeros).  One thread per element; consecutive threads read consecutive c of a Wq row.
__global__ __launch_bounds__(256) void ipa_kpp_kernel(const float* __restrict__ kip, const bf16_t* __restrict__ Wq, const float* __restrict__ gamma,
                                                      bf16_t* __restrict__ kpp, int C, int H, int nt, int colsP, float scale) {
  const int c = blockIdx.x * 256 + threadIdx.x, col = blockIdx.y, b = blockIdx.z;
  if (c >= C) return;
  float v = 0.f;
  if (col < H * nt) {
    const int h = col / nt, t = col - h * nt, D = C / H;
    const float* kr = kip + ((long long)b * nt + t) * C + h * D;
    const bf16_t* wq = Wq + (long long)h * D * C + c;
    for (int d = 0; d < D; ++d) v = fmaf(kr[d], bf2f(wq[(long long)d * C]), v);
    v *= gamma[c] * scale;
  }
  kpp[((long long)b * colsP + col) * C + c] = f2bf(v);
}
// cs[b][col] = sum_c bf16 K''[b][col][c];  bs[b][col] = scale k_ip[b][t][h D ..] . wqb[h D ..]  (padded columns: zeros).  One wave per (b, col).
__global__ __launch_bounds__(256) void ipa_csbs_kernel(const bf16_t* __restrict__ kpp, const float* __restrict__ kip, const float* __restrict__ wqb,
                                                       float* __restrict__ cs, float* __restrict__ bs, int B, int C, int H, int nt, int colsP, float scale) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * colsP) return;
  const int b = row / colsP, col = row - b * colsP;
  float s = 0.f, d_ = 0.f;
  if (col < H * nt) {
    const int h = col / nt, t = col - h * nt, D = C / H;
    const bf16_t* r = kpp + (long long)row * C;
    for (int c = lane; c < C; c += 64) s += bf2f(r[c]);
    const float* kr = kip + ((long long)b * nt + t) * C + h * D;
    for (int d = lane; d < D; d += 64) d_ = fmaf(kr[d], wqb[h * D + d], d_);
  }
  for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); d_ += __shfl_xor(d_, o); }
  if (lane == 0) { cs[row] = s; bs[row] = d_ * scale; }
}
// V''[b][n][col] (bf16; columns col >= H nt: zeros).  One thread per element.
__global__ __launch_bounds__(256) void ipa_vpp_kernel(const float* __restrict__ vip, const bf16_t* __restrict__ Wo, bf16_t* __restrict__ vpp, int C, int H,
                                                      int nt, int colsP) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= C * colsP) return;
  const int n = i / colsP, col = i - n * colsP;
  float v = 0.f;
  if (col < H * nt) {
    const int h = col / nt, t = col - h * nt, D = C / H;
    const float* vr = vip + ((long long)b * nt + t) * C + h * D;
    const bf16_t* wo = Wo + (long long)n * C + h * D;
    for (int d = 0; d < D; ++d) v = fmaf(vr[d], bf2f(wo[d]), v);
  }
  vpp[(long long)b * C * colsP + i] = f2bf(v);
}
int launch_ipa_premul(const IpaPremulP& p, hipStream_t st) {
  if (p.B < 1 || p.C < 8 || p.C % 8 || p.H < 1 || p.C % p.H || p.nt < 1 || p.colsP % 16 || p.colsP < p.H * p.nt || p.colsP > IPA_MAX_COLS) {
    agd_set_error("ipa premul: B %d C %d heads %d tokens %d cols %d", p.B, p.C, p.H, p.nt, p.colsP); return -1; }
  hipLaunchKernelGGL(ipa_kpp_kernel, dim3((p.C + 255) / 256, p.colsP, p.B), dim3(256), 0, st, p.kip, p.wq, p.gamma, p.kpp, p.C, p.H, p.nt, p.colsP, p.scale);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(ipa_csbs_kernel, dim3((p.B * p.colsP + 3) / 4), dim3(256), 0, st, p.kpp, p.kip, p.wqb, p.cs, p.bs, p.B, p.C, p.H, p.nt, p.colsP, p.scale);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(ipa_vpp_kernel, dim3((p.C * p.colsP + 255) / 256, p.B), dim3(256), 0, st, p.vip, p.wo, p.vpp, p.C, p.H, p.nt, p.colsP);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// P = softmax_head(rstd (h . K''^T - mu cs) + bs).  grid (row tiles of 64 of ONE image, image): rows of two images never meet in a
// workgroup, the ragged last tile of an image is masked.  A wave owns 16 rows: A fragments (the raw rows) and B fragments (this image's
// K'' rows, at most 80 x C bf16, shared by every workgroup of the image through L2) straight from global memory, no LDS ring; the row's
// sum / sum of squares are taken from the A fragments on the way.  MFMA operand roles swapped as premul_gemm_kernel: lane (q, px) ends
// with S[row px][16 j + 4 q + r].  The softmax groups (n_tok columns, any n_tok) are resolved through an LDS copy of the wave's S tile.
// ---------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void ipa_scores_kernel(const IpaScoreP p) {
  constexpr int LD = NT * 16 + 1;
  __shared__ float S[4][16][LD];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b = blockIdx.y, r0 = blockIdx.x * 64 + wid * 16;
  const int fr = lane & 15, qd = lane >> 4, kc = qd * 8;
  const int C = p.C, colsP = NT * 16;
  const bool a_ok = r0 + fr < p.HW;
  const bf16_t* hr = p.h + ((long long)b * p.HW + (a_ok ? r0 + fr : 0)) * C;
  const bf16_t* kp = p.kpp + (long long)b * colsP * C;
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sm = 0.f, sq = 0.f;
  for (int k0 = 0; k0 < C; k0 += 32) {
    const bool k_ok = k0 + kc < C;                       // C % 8 == 0: the last 32-deep step may be ragged
    u32x4 av = {0u, 0u, 0u, 0u};
    if (a_ok && k_ok) av = *(const u32x4*)(hr + k0 + kc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = __uint_as_float(av[e] << 16), hi = __uint_as_float(av[e] & 0xFFFF0000u);
      sm += lo + hi; sq = fmaf(lo, lo, fmaf(hi, hi, sq));
    }
    const bf16x8 a = __builtin_bit_cast(bf16x8, av);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bf16x8 w = {};
      if (k_ok) w = *(const bf16x8*)(kp + (long long)(j * 16 + fr) * C + k0 + kc);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, acc[j], 0, 0, 0);
    }
  }
  sm += __shfl_xor(sm, 16); sm += __shfl_xor(sm, 32);
  sq += __shfl_xor(sq, 16); sq += __shfl_xor(sq, 32);
  const float mu = sm / (float)C;
  float var = sq / (float)C - mu * mu; var = var < 0.f ? 0.f : var;
  const float rstd = rsqrtf(var + p.eps);
  const float* cs = p.cs + (long long)b * colsP; const float* bs = p.bs + (long long)b * colsP;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int col = j * 16 + 4 * qd + r; S[wid][fr][col] = rstd * (acc[j][r] - mu * cs[col]) + bs[col]; }
  __syncthreads();
  // (the padded columns hold rstd (0 - mu 0) + 0 = 0 and belong to no head: they stay zero)
  for (int i = lane; i < 16 * p.H; i += 64) {
    const int rr = i / p.H, hd = i - rr * p.H;
    float* sp = &S[wid][rr][hd * p.nt];
    float mx = sp[0];
    for (int t = 1; t < p.nt; ++t) mx = fmaxf(mx, sp[t]);
    float sum = 0.f;
    for (int t = 0; t < p.nt; ++t) { const float e = __builtin_amdgcn_exp2f((sp[t] - mx) * 1.44269504088896340736f); sp[t] = e; sum += e; }
    const float inv = 1.0f / sum;
    for (int t = 0; t < p.nt; ++t) sp[t] *= inv;
  }
  __syncthreads();
  constexpr int NV = NT * 2;                             // 16-byte vectors per row of P
  for (int i = lane; i < 16 * NV; i += 64) {
    const int rr = i / NV, v = i - rr * NV;
    if (r0 + rr >= p.HW) continue;
    const float* sp = &S[wid][rr][v * 8];
    u32x4 pk;
    pk[0] = pack_bf2(sp[0], sp[1]); pk[1] = pack_bf2(sp[2], sp[3]); pk[2] = pack_bf2(sp[4], sp[5]); pk[3] = pack_bf2(sp[6], sp[7]);
    *(u32x4*)(p.P + ((long long)b * p.HW + r0 + rr) * colsP + v * 8) = pk;
  }
}
int launch_ipa_scores(const IpaScoreP& p, hipStream_t st) {
  if (p.B < 1 || p.HW < 1 || p.C < 8 || p.C % 8 || p.H < 1 || p.nt < 1 || p.colsP % 16 || p.colsP < 16 || p.colsP > IPA_MAX_COLS || p.H * p.nt > p.colsP ||
      p.colsP - p.H * p.nt >= 16 || (long long)p.B * p.HW * p.C >= (1ll << 40)) {
    agd_set_error("ipa scores: %d images of %d rows x %d channels, %d heads x %d tokens in %d columns", p.B, p.HW, p.C, p.H, p.nt, p.colsP); return -1; }
  const dim3 grid((p.HW + 63) / 64, p.B);
  switch (p.colsP / 16) {
    case 1: hipLaunchKernelGGL(ipa_scores_kernel<1>, grid, dim3(256), 0, st, p); break;
    case 2: hipLaunchKernelGGL(ipa_scores_kernel<2>, grid, dim3(256), 0, st, p); break;
    case 3: hipLaunchKernelGGL(ipa_scores_kernel<3>, grid, dim3(256), 0, st, p); break;
    case 4: hipLaunchKernelGGL(ipa_scores_kernel<4>, grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL(ipa_scores_kernel<5>, grid, dim3(256), 0, st, p); break;
  }
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// ---------------------------------------------------------------------------------------
// h[m][n] += s sum_col P[m][col] V''[b][n][col], in place.  grid (row tiles of 64 of one image, 64-column groups, image); a wave owns
// 16 rows x 64 columns as two pairs of MFMA tiles.  Operand roles swapped, and the weight rows of a pair permuted -- tile 0 takes rows
// 8 (i >> 2) + (i & 3), tile 1 the same + 4 -- so that lane (q, px) ends with the EIGHT consecutive columns 8 q .. 8 q + 7 of row px: one
// 16-byte load and one 16-byte store of h per lane and pair, every element owned by exactly one lane, rounded to bf16 once.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ipa_add_kernel(const IpaAddP p) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b = blockIdx.z, r0 = blockIdx.x * 64 + wid * 16, n0 = blockIdx.y * 64;
  const int fr = lane & 15, qd = lane >> 4, kc = qd * 8;
  const int C = p.C, colsP = p.colsP;
  const bool a_ok = r0 + fr < p.HW;
  const long long row = (long long)b * p.HW + (a_ok ? r0 + fr : 0);
  const bf16_t* pr = p.P + row * colsP;
  const bf16_t* vp = p.vpp + (long long)b * C * colsP;
#pragma unroll
  for (int pi = 0; pi < 2; ++pi) {
    const int nb = n0 + 32 * pi;
    const int n_lo = nb + 8 * (fr >> 2) + (fr & 3), n_hi = n_lo + 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < colsP; k0 += 32) {
      const bool k_ok = k0 + kc < colsP;                 // colsP % 16 == 0: the last step may be ragged
      bf16x8 a = {}, w0 = {}, w1 = {};
      if (a_ok && k_ok) a = *(const bf16x8*)(pr + k0 + kc);
      if (k_ok && n_lo < C) w0 = *(const bf16x8*)(vp + (long long)n_lo * colsP + k0 + kc);
      if (k_ok && n_hi < C) w1 = *(const bf16x8*)(vp + (long long)n_hi * colsP + k0 + kc);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, a, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, a, acc1, 0, 0, 0);
    }
    const int n = nb + 8 * qd;                           // C % 8 == 0: the vector is whole or absent
    if (a_ok && n < C) {
      bf16_t* hp = p.h + row * C + n;
      const u32x4 hv = *(const u32x4*)hp;
      float o[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[2 * e] = __uint_as_float(hv[e] << 16); o[2 * e + 1] = __uint_as_float(hv[e] & 0xFFFF0000u); }
#pragma unroll
      for (int r = 0; r < 4; ++r) { o[r] = fmaf(p.s, acc0[r], o[r]); o[4 + r] = fmaf(p.s, acc1[r], o[4 + r]); }
      u32x4 pk;
      pk[0] = pack_bf2(o[0], o[1]); pk[1] = pack_bf2(o[2], o[3]); pk[2] = pack_bf2(o[4], o[5]); pk[3] = pack_bf2(o[6], o[7]);
      *(u32x4*)hp = pk;
    }
  }
}
int launch_ipa_add(const IpaAddP& p, hipStream_t st) {
  if (p.B < 1 || p.HW < 1 || p.C < 8 || p.C % 8 || p.colsP % 16 || p.colsP < 16 || p.colsP > IPA_MAX_COLS || (long long)p.B * p.HW * p.C >= (1ll << 40)) {
    agd_set_error("ipa add: %d images of %d rows x %d channels, %d columns", p.B, p.HW, p.C, p.colsP); return -1; }
  hipLaunchKernelGGL(ipa_add_kernel, dim3((p.HW + 63) / 64, (p.C + 63) / 64, p.B), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
