// Inpainting (diffusers StableDiffusionInpaintPipeline) byte movers: the once-per-call mask front end, the per-evaluation model input of
// a 9-channel UNet and the per-step latent blend of a 4-channel one.  The UNet, the VAE encoder and the schedulers are the txt2img launches.
#include "kernels.h"

static inline int grid_for(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// One thread per image pixel.  image: uint8 NHWC [B][S][S][3] (x / 255, then 2 x - 1, in fp32) or, image_f32, fp32 NCHW [B][3][S][S]
// already in [-1,1]; mask: uint8 [B][S][S] (/ 255) or, mask_f32, fp32 [B][S][S] in [0,1], binarized m < 0.5 -> 0, else 1.
// image_out / masked_out fp32 NCHW [B][3][H][W] (masked = image * (m < 0.5)); mask_lat fp32 [B][1][H/f][W/f] takes pixel (f i, f j)
// (nearest).  Any output may be null.
__global__ void inpaint_front_kernel(const void* __restrict__ image, int image_f32, const void* __restrict__ mask, int mask_f32, int B, int H,
                                     int W, int f, float* __restrict__ image_out, float* __restrict__ masked_out, float* __restrict__ mask_lat) {
  const long long HW = (long long)H * W, total = (long long)B * HW;
  const int Lh = H / f, Lw = W / f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW);
    const long long p = i - (long long)b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const float m = mask_f32 ? ((const float*)mask)[i] : (float)((const unsigned char*)mask)[i] / 255.0f;
    const float mb = m < 0.5f ? 0.f : 1.f;
    const float keep = mb < 0.5f ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long o = ((long long)b * 3 + c) * HW + p;
      float v;
      if (image_f32) v = ((const float*)image)[o];
      else { v = (float)((const unsigned char*)image)[i * 3 + c] / 255.0f; v = 2.0f * v - 1.0f; }
      if (image_out) image_out[o] = v;
      if (masked_out) masked_out[o] = v * keep;
    }
    if (mask_lat && y % f == 0 && x % f == 0) mask_lat[((long long)b * Lh + y / f) * Lw + x / f] = mb;
  }
}
int launch_inpaint_front(const void* image, int image_f32, const void* mask, int mask_f32, int B, int H, int W, int f, float* image_out,
                         float* masked_out, float* mask_lat, hipStream_t st) {
  if (B < 1 || f < 1 || H < f || H % f || W < f || W % f) { agd_set_error("inpaint front end: batch %d size %d x %d (each side a multiple of %d)", B, H, W, f); return -1; }
  hipLaunchKernelGGL(inpaint_front_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, st, image, image_f32, mask, mask_f32, B, H, W, f,
                     image_out, masked_out, mask_lat);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// The 9-channel UNet input, written whole every evaluation like prep_latents_kernel: bf16 NHWC [dup B][HW][Cpad] with channels
// [0, Cl) the latents (fp32 NCHW [B][Cl][HW]), [Cl, Cl + Cm) the mask ([B][Cm][HW]), [Cl + Cm, Cl + Cm + Cc) the masked-image latents
// ([B][Cc][HW]), zero above.  Row r reads image r % B: both CFG halves see the same mask and masked latents.
__global__ void prep_inpaint_kernel(const float* __restrict__ lat, const float* __restrict__ mask, const float* __restrict__ cond,
                                    bf16_t* __restrict__ out, int B, int Cl, int Cm, int Cc, int HW, int Cpad, int dup) {
  const long long total = (long long)dup * B * HW * Cpad;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cpad);
    const long long px = i / Cpad;
    const int p = (int)(px % HW);
    const int b = (int)((px / HW) % B);
    float v = 0.f;
    if (c < Cl) v = lat[((long long)b * Cl + c) * HW + p];
    else if (c < Cl + Cm) v = mask[((long long)b * Cm + (c - Cl)) * HW + p];
    else if (c < Cl + Cm + Cc) v = cond[((long long)b * Cc + (c - Cl - Cm)) * HW + p];
    out[i] = f2bf(v);
  }
}
int launch_prep_inpaint(const float* lat, const float* mask, const float* cond, bf16_t* out, int B, int Cl, int Cm, int Cc, int HW, int Cpad,
                        int dup, hipStream_t st) {
  if (Cl + Cm + Cc > Cpad) { agd_set_error("prep_inpaint: %d + %d + %d channels exceed the %d-channel input", Cl, Cm, Cc, Cpad); return -1; }
  hipLaunchKernelGGL(prep_inpaint_kernel, dim3(grid_for((long long)dup * B * HW * Cpad)), dim3(256), 0, st, lat, mask, cond, out, B, Cl, Cm, Cc,
                     HW, Cpad, dup);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// The 4-channel blend after a scheduler step, in place on fp32 NCHW latents [B][C][HW]:
//   x = (1 - m) (sa x0img + sb n) + m x,  m = mask[b][p]
// In this form m = 0, sa = 1, sb = 0 gives x0img exactly and m = 1 gives x exactly.
__global__ void inpaint_blend_kernel(float* __restrict__ lat, const float* __restrict__ x0img, const float* __restrict__ noise,
                                     const float* __restrict__ mask, int B, int C, int HW, float sa, float sb) {
  const long long total = (long long)B * C * HW;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    const int b = (int)(i / ((long long)HW * C));
    const float m = mask[(long long)b * HW + p];
    lat[i] = (1.f - m) * (sa * x0img[i] + sb * noise[i]) + m * lat[i];
  }
}
int launch_inpaint_blend(float* lat, const float* x0img, const float* noise, const float* mask, int B, int C, int HW, float sa, float sb,
                         hipStream_t st) {
  hipLaunchKernelGGL(inpaint_blend_kernel, dim3(grid_for((long long)B * C * HW)), dim3(256), 0, st, lat, x0img, noise, mask, B, C, HW, sa, sb);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
