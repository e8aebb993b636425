// InstructPix2Pix (diffusers StableDiffusionInstructPix2PixPipeline) byte movers: the once-per-call image front end, the per-evaluation
// model input of the three guidance branches of an 8-channel UNet, and the fold of the three branch outputs into the [uncond | cond] pair
// the schedulers' two-way step kernels take.  The UNet, the VAE encoder and the step kernels are the txt2img launches.
#include "kernels.h"

static inline int grid_for(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// One thread per output element.  image: uint8 NHWC [B][H][W][3] (x / 255, then 2 x - 1, in fp32) or, image_f32, fp32 NCHW [B][3][H][W]
// already in [-1,1] (copied).  out fp32 NCHW [B][3][H][W].
__global__ void ip2p_front_kernel(const void* __restrict__ image, int image_f32, long long HW, long long total, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    float v;
    if (image_f32) v = ((const float*)image)[i];
    else {
      const long long p = i % HW, bc = i / HW, b = bc / 3, ch = bc - b * 3;
      v = (float)((const unsigned char*)image)[(b * HW + p) * 3 + ch] / 255.0f; v = 2.0f * v - 1.0f;
    }
    out[i] = v;
  }
}
int launch_ip2p_front(const void* image, int image_f32, int B, int H, int W, float* out, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1) { agd_set_error("ip2p front end: batch %d size %d x %d", B, H, W); return -1; }
  const long long HW = (long long)H * W, total = (long long)B * 3 * HW;
  hipLaunchKernelGGL(ip2p_front_kernel, dim3(grid_for(total)), dim3(256), 0, st, image, image_f32, HW, total, out);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// The 8-channel UNet input of the three branches, written whole every evaluation like prep_inpaint_kernel: bf16 NHWC [3 B][HW][Cpad].
// Channels [0, Cl) are the latents (fp32 NCHW [B][Cl][HW]) in every row; channels [Cl, Cl + Cc) are the image latents ([B][Cc][HW]) in
// rows [B, 3 B) (the image and text branches) and zero in rows [0, B) (the uncond branch); zero above.  Row r reads image r % B.
__global__ void prep_ip2p_kernel(const float* __restrict__ lat, const float* __restrict__ img, bf16_t* __restrict__ out, int B, int Cl, int Cc,
                                 int HW, int Cpad) {
  const long long total = (long long)3 * B * HW * Cpad;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cpad);
    const long long px = i / Cpad;
    const int p = (int)(px % HW);
    const int r = (int)(px / HW);
    const int b = r % B;
    float v = 0.f;
    if (c < Cl) v = lat[((long long)b * Cl + c) * HW + p];
    else if (c < Cl + Cc && r >= B) v = img[((long long)b * Cc + (c - Cl)) * HW + p];
    out[i] = f2bf(v);
  }
}
int launch_prep_ip2p(const float* lat, const float* img, bf16_t* out, int B, int Cl, int Cc, int HW, int Cpad, hipStream_t st) {
  if (Cl + Cc > Cpad) { agd_set_error("prep_ip2p: %d + %d channels exceed the %d-channel input", Cl, Cc, Cpad); return -1; }
  hipLaunchKernelGGL(prep_ip2p_kernel, dim3(grid_for((long long)3 * B * HW * Cpad)), dim3(256), 0, st, lat, img, out, B, Cl, Cc, HW, Cpad);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// The three-way guidance folded into a two-way one, in place.  eps fp32 [3][n]: e_uncond | e_image | e_text (n = B HW ldc).  Rewrites
//   e_image <- lo = e_uncond + s_i (e_image - e_uncond),   e_text <- hi = lo + (e_text - e_image)
// so a two-way step on (lo, hi) with the text scale s_t gives lo + s_t (hi - lo) = e_uncond + s_t (e_text - e_image) + s_i (e_image - e_uncond).
// In this form e_image == e_uncond gives lo = e_uncond whatever s_i, and e_text == e_image gives hi = lo exactly.
__global__ void ip2p_fold_kernel(float* __restrict__ eps, long long n, float s_i) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float eu = eps[i], ei = eps[n + i], et = eps[2 * n + i];
    const float lo = eu + s_i * (ei - eu);
    eps[n + i] = lo;
    eps[2 * n + i] = lo + (et - ei);
  }
}
int launch_ip2p_fold(float* eps, long long n, float image_guidance, hipStream_t st) {
  hipLaunchKernelGGL(ip2p_fold_kernel, dim3(grid_for(n)), dim3(256), 0, st, eps, n, image_guidance);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
