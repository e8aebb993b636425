// CLIP vision tower ends of the Stable-Diffusion safety checker (diffusers StableDiffusionSafetyChecker over transformers
// CLIPVisionModel): pixels -> patch rows, patch embeddings -> [CLS] + positions -> pre_layrnorm, and the pooled head
// (post_layernorm of the CLS row -> visual_projection -> L2 normalisation -> cosines against the concept rows).
// The 24 encoder layers between them are the text encoder's layer loop (model.hip clip_encoder_layers, causal = 0).
#include "kernels.h"

// sum over the workgroup (wave64 butterflies, then one LDS slot per wave); every thread gets the total.  `red` holds
// blockDim.x / 64 floats; the leading barrier lets a caller reuse `red` right after a previous call.
AGD_DEV float vis_wave_sum(float s) {
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}
AGD_DEV float vis_block_sum(float s, float* red) {
  s = vis_wave_sum(s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  return t;
}

// CLIPImageProcessor rescale + normalize, then the patch_embedding conv's im2col: u8 [B][S][S][3] (S = image_size, already resized)
// -> rows [B * g * g][Kpad] bf16 with g = S / ps, row = image * g * g + py * g + px, column k = ch * ps * ps + ky * ps + kx (the
// torch conv weight [hidden][3][ps][ps] flattened), zero for k >= 3 ps ps.  Patches tile the image exactly (S % ps == 0), so
// every pixel is visited once: pix (optional) receives pixel_values fp32 [B][3][S][S].
__global__ __launch_bounds__(256) void vis_patchify_kernel(const unsigned char* __restrict__ img, int S, int ps, int Kpad, long long total,
                                                            VisNorm nm, bf16_t* __restrict__ rows, float* __restrict__ pix) {
  const int g = S / ps, np = g * g, pp = ps * ps, K = 3 * pp;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % Kpad);
    float v = 0.f;
    if (k < K) {
      const long long r = i / Kpad;
      const int b = (int)(r / np), p = (int)(r % np), py = p / g, px = p - py * g;
      const int ch = k / pp, t = k - ch * pp, ky = t / ps, kx = t - ky * ps;
      const int y = py * ps + ky, x = px * ps + kx;
      const float mean = ch == 0 ? nm.mean0 : (ch == 1 ? nm.mean1 : nm.mean2);
      const float sd = ch == 0 ? nm.std0 : (ch == 1 ? nm.std1 : nm.std2);
      const float u = (float)img[(((long long)b * S + y) * S + x) * 3 + ch] / 255.0f;
      v = (u - mean) / sd;
      if (pix) pix[(((long long)b * 3 + ch) * S + y) * S + x] = v;
    }
    rows[i] = f2bf(v);
  }
}
int launch_vis_patchify(const unsigned char* img, int B, int S, int ps, int Kpad, VisNorm nm, bf16_t* rows, float* pix, hipStream_t st) {
  if (ps < 1 || S % ps || Kpad < 3 * ps * ps) { agd_set_error("vision: image %d / patch %d / Kpad %d inconsistent", S, ps, Kpad); return -1; }
  const long long total = (long long)B * (S / ps) * (S / ps) * Kpad;
  const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  hipLaunchKernelGGL(vis_patchify_kernel, dim3(grid), dim3(256), 0, st, img, S, ps, Kpad, total, nm, rows, pix);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// CLIPVisionEmbeddings + pre_layrnorm: row r = image * (np + 1) + t of x (bf16 [B (np + 1)][H]) is
// LayerNorm((t == 0 ? class_embedding : patch row t - 1 of pe) + position_embedding[t]); pe fp32 [B np][H] (the patch GEMM).
// One workgroup per row, H <= 2048 held in registers (8 per thread).
__global__ __launch_bounds__(256) void vis_embed_ln_kernel(const float* __restrict__ pe, const float* __restrict__ cls, const float* __restrict__ pos,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int np, int H, float eps,
                                                            bf16_t* __restrict__ x) {
  __shared__ float red[4];
  const int r = blockIdx.x, T = np + 1, b = r / T, t = r - b * T;
  const float* src = t == 0 ? cls : pe + ((long long)b * np + t - 1) * H;
  float v[8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = threadIdx.x + j * 256;
    v[j] = k < H ? src[k] + pos[(long long)t * H + k] : 0.f;
    s += v[j];
  }
  const float mean = vis_block_sum(s, red) / H;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) { const int k = threadIdx.x + j * 256; const float d = k < H ? v[j] - mean : 0.f; q += d * d; }
  const float rstd = rsqrtf(vis_block_sum(q, red) / H + eps);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = threadIdx.x + j * 256;
    if (k < H) x[(long long)r * H + k] = f2bf((v[j] - mean) * rstd * gamma[k] + beta[k]);
  }
}
int launch_vis_embed_ln(const float* pe, const float* cls, const float* pos, const float* gamma, const float* beta, int B, int np, int H,
                        float eps, bf16_t* x, hipStream_t st) {
  if (H < 1 || H > 2048) { agd_set_error("vision: hidden %d unsupported (<= 2048)", H); return -1; }
  hipLaunchKernelGGL(vis_embed_ln_kernel, dim3(B * (np + 1)), dim3(256), 0, st, pe, cls, pos, gamma, beta, np, H, eps, x);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// The pooled head, one workgroup per image: y = post_layernorm(x[CLS row]) (CLIPVisionModel pooler_output), e = visual_projection(y)
// (Wp fp32 [P][H], no bias), cos[i] = e . E[i] / max(|e|, 1e-12) for the n pre-normalised concept rows E fp32 [n][P]
// (cosine_distance(image_embeds, concept_embeds) of the checker; the concept side was normalised at finalize).
__global__ __launch_bounds__(256) void vis_pooled_head_kernel(const bf16_t* __restrict__ x, int T, int H, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, const float* __restrict__ Wp, int P,
                                                               const float* __restrict__ E, int n, float* __restrict__ cos_out,
                                                               float* __restrict__ emb_out) {
  extern __shared__ float sm[];                    // [H] y, [P] e, [4] reduction slots
  float* y = sm; float* e = sm + H; float* red = e + P;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bf16_t* xr = x + (long long)b * T * H;
  float s = 0.f;
  for (int k = tid; k < H; k += 256) { const float v = bf2f(xr[k]); y[k] = v; s += v; }
  const float mean = vis_block_sum(s, red) / H;
  float q = 0.f;
  for (int k = tid; k < H; k += 256) { const float d = y[k] - mean; q += d * d; }
  const float rstd = rsqrtf(vis_block_sum(q, red) / H + eps);
  for (int k = tid; k < H; k += 256) y[k] = (y[k] - mean) * rstd * gamma[k] + beta[k];
  __syncthreads();
  for (int j = w; j < P; j += 4) {                 // one wave per projection row: coalesced reads of Wp
    const float* wr = Wp + (long long)j * H;
    float a = 0.f;
    for (int k = lane; k < H; k += 64) a += wr[k] * y[k];
    a = vis_wave_sum(a);
    if (lane == 0) e[j] = a;
  }
  __syncthreads();
  if (emb_out) for (int j = tid; j < P; j += 256) emb_out[(long long)b * P + j] = e[j];      // image_embeds as projected (not normalised)
  float ss = 0.f;
  for (int j = tid; j < P; j += 256) ss += e[j] * e[j];
  const float inv = 1.0f / fmaxf(sqrtf(vis_block_sum(ss, red)), 1e-12f);
  for (int i = w; i < n; i += 4) {
    const float* er = E + (long long)i * P;
    float a = 0.f;
    for (int k = lane; k < P; k += 64) a += e[k] * er[k];
    a = vis_wave_sum(a);
    if (lane == 0) cos_out[(long long)b * n + i] = a * inv;
  }
}
int launch_vis_pooled_head(const bf16_t* x, int B, int T, int H, const float* gamma, const float* beta, float eps, const float* Wp, int P,
                           const float* E, int n, float* cos_out, float* emb_out, hipStream_t st) {
  const size_t lds = (size_t)(H + P + 4) * sizeof(float);
  if (lds > 65536) { agd_set_error("vision: pooled head of hidden %d + projection %d exceeds the LDS", H, P); return -1; }
  hipLaunchKernelGGL(vis_pooled_head_kernel, dim3(B), dim3(256), lds, st, x, T, H, gamma, beta, eps, Wp, P, E, n, cos_out, emb_out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
