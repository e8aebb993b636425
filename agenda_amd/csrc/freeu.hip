// FreeU (Si et al. 2023; diffusers >= 0.22 enable_freeu): the re-weighting of an up block's resnet inputs, both tensors in ONE launch.
//   hidden' = hidden with its first Ch / 2 channels times b                      (the backbone scale)
//   skip'   = ifft(mask . fft(skip)).real, mask = s on the centred 2 x 2 block   (diffusers fourier_filter, threshold = 1)
// The mask scales the frequencies {-1 mod H, 0} x {-1 mod W, 0} (as sets) and nothing else, so the filter is a rank-4 projection:
//   y = x + (s - 1) / (H W) . Sum_k [ C_k cos a_k + S_k sin a_k ],   C_k = Sum x cos a_k,   S_k = Sum x sin a_k,   a_k = ky th y + kx ph x
// with th = 2 pi / H, ph = 2 pi / W.  A term is the same for k and -k, so the kernel takes a = th y, ph x and th y + ph x: seven real sums per
// (image, channel) -- Sum x, and a cos / sin pair for each of the three angles, the third pair from the angle-addition products of the
// first two -- and one apply pass.  A side of 1 has no frequency -1: its pairs are dropped.  No transform, no complex numbers, any H, W >= 1.
#include "kernels.h"

#define FREEU_TAB 512        // H + W entries of (cos, sin) kept in LDS; larger maps evaluate sincospif per pixel

struct FreeuJob { const bf16_t* x; bf16_t* y; float* part; int C, VC, nblk; };

// One workgroup owns one image x (VC vectors of 8 channels): thread (rg, vc) walks the map's pixels rg, rg + RG, .. inside each 64-pixel
// tile (RG = 256 / VC) with 16-byte loads and stores -- lanes along channels, the map's rows over the row groups / waves.
//   filter job (blocks [0, job[0].nblk)): pass 1 sums the seven moments per thread, the row groups are summed in ascending order out of LDS
//     by one thread per (moment, channel); pass 2 re-reads the map (L2) and writes y.
//   scale job (the rest): y = bf16(x * (channel < half ? b : 1)).
// part != nullptr: the workgroup also leaves the GroupNorm partial sums of its output, [B2 HW / 64][C] float2 = (sum, sum of squares) of the
// bf16-ROUNDED values per 64-row tile -- the igemm epilogue's colstat_out layout (HW % 64 == 0).  Every sum runs in a fixed order, no atomics:
// two runs are bit-identical.
__global__ __launch_bounds__(256) void freeu_kernel(FreeuJob j0, FreeuJob j1, int H, int W, float g, float b, int half) {
  __shared__ float red[256 * 56];
  __shared__ float mom[7 * 64];
  __shared__ float tab[2 * FREEU_TAB];
  const bool filter = (int)blockIdx.x < j0.nblk;
  const FreeuJob J = filter ? j0 : j1;
  const int bid = filter ? blockIdx.x : blockIdx.x - j0.nblk;
  const int HW = H * W, C = J.C, VC = J.VC, RG = 256 / VC, W8 = VC * 8, ncb = C / W8;
  const int img = bid / ncb, cb = bid - img * ncb;
  const int tid = threadIdx.x, vc = tid % VC, rg = tid / VC;
  const int ch = cb * W8 + vc * 8;
  const bf16_t* xp = J.x + (long long)img * HW * C + ch;
  bf16_t* yp = J.y + (long long)img * HW * C + ch;
  const bool use_tab = H + W <= FREEU_TAB;
  const int ntile = (HW + 63) / 64;
  float m[7][8];

  auto trig = [&](int p, float& cy, float& sy, float& cx, float& sx) {
    const int py = p / W, px = p - py * W;
    if (use_tab) { cy = tab[2 * py]; sy = tab[2 * py + 1]; cx = tab[2 * (H + px)]; sx = tab[2 * (H + px) + 1]; }
    else { sincospif(2.f * (float)py / (float)H, &sy, &cy); sincospif(2.f * (float)px / (float)W, &sx, &cx); }
  };

  if (filter) {
    if (use_tab) {
      for (int i = tid; i < H + W; i += 256) {
        float s_, c_;
        if (i < H) sincospif(2.f * (float)i / (float)H, &s_, &c_); else sincospif(2.f * (float)(i - H) / (float)W, &s_, &c_);
        tab[2 * i] = c_; tab[2 * i + 1] = s_;
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) m[k][e] = 0.f;
    for (int t = 0; t < ntile; ++t) {
      const int pe = min(HW, t * 64 + 64);
      for (int p = t * 64 + rg; p < pe; p += RG) {
        float cy, sy, cx, sx; trig(p, cy, sy, cx, sx);
        const float cxy = cy * cx - sy * sx, sxy = sy * cx + cy * sx;
        const s16x8 xv = *(const s16x8*)(xp + (long long)p * C);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = bf2f((bf16_t)xv[e]);
          m[0][e] += v;
          m[1][e] = fmaf(v, cy, m[1][e]); m[2][e] = fmaf(v, sy, m[2][e]);
          m[3][e] = fmaf(v, cx, m[3][e]); m[4][e] = fmaf(v, sx, m[4][e]);
          m[5][e] = fmaf(v, cxy, m[5][e]); m[6][e] = fmaf(v, sxy, m[6][e]);
        }
      }
    }
    // red[rg][moment][vc * 8 + e]; then output o = moment * W8 + channel sums its RG row groups in ascending order
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[(rg * 7 + k) * W8 + vc * 8 + e] = m[k][e];
    __syncthreads();
    for (int o = tid; o < 7 * W8; o += 256) {
      float a = 0.f;
      for (int r = 0; r < RG; ++r) a += red[r * 7 * W8 + o];
      const int k = o / W8;
      // the weight (s - 1) / (H W) folded in; a side of 1 has only frequency 0 (its cos table is 1, its pair would count frequency 0 again)
      const bool on = k == 0 || (k <= 2 ? H > 1 : k <= 4 ? W > 1 : (H > 1 && W > 1));
      mom[o] = on ? g * a : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) m[k][e] = mom[k * W8 + vc * 8 + e];
  }

  for (int t = 0; t < ntile; ++t) {
    const int pe = min(HW, t * 64 + 64);
    float sum[8], sq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sum[e] = 0.f; sq[e] = 0.f; }
    for (int p = t * 64 + rg; p < pe; p += RG) {
      const s16x8 xv = *(const s16x8*)(xp + (long long)p * C);
      float o[8];
      if (filter) {
        float cy, sy, cx, sx; trig(p, cy, sy, cx, sx);
        const float cxy = cy * cx - sy * sx, sxy = sy * cx + cy * sx;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float d = m[0][e];
          d = fmaf(m[1][e], cy, d); d = fmaf(m[2][e], sy, d); d = fmaf(m[3][e], cx, d); d = fmaf(m[4][e], sx, d);
          d = fmaf(m[5][e], cxy, d); d = fmaf(m[6][e], sxy, d);
          o[e] = bf2f((bf16_t)xv[e]) + d;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = bf2f((bf16_t)xv[e]) * (ch + e < half ? b : 1.f);
      }
      u32x4 pk;
      pk[0] = pack_bf2(o[0], o[1]); pk[1] = pack_bf2(o[2], o[3]); pk[2] = pack_bf2(o[4], o[5]); pk[3] = pack_bf2(o[6], o[7]);
      *(u32x4*)(yp + (long long)p * C) = pk;
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float v = __uint_as_float(e & 1 ? pk[e >> 1] & 0xFFFF0000u : pk[e >> 1] << 16); sum[e] += v; sq[e] += v * v; }
    }
    if (J.part) {                                        // (uniform over the workgroup)
      __syncthreads();                                   // the previous tile's (or the moments') readers are done with red
#pragma unroll
      for (int e = 0; e < 8; ++e) { red[2 * (rg * W8 + vc * 8 + e)] = sum[e]; red[2 * (rg * W8 + vc * 8 + e) + 1] = sq[e]; }
      __syncthreads();
      if (tid < W8) {
        float a = 0.f, q = 0.f;
        for (int r = 0; r < RG; ++r) { a += red[2 * (r * W8 + tid)]; q += red[2 * (r * W8 + tid) + 1]; }
        float* dst = J.part + (((long long)img * (HW / 64) + t) * C + cb * W8 + tid) * 2;
        dst[0] = a; dst[1] = q;
      }
    }
  }
}

// One launch for one resnet's pair.  skip_out == nullptr: no filter (s == 1); hidden_out == nullptr: no scale (b == 1); both null is refused
// (the caller launches nothing).  *_part: room for [B2 HW / 64][C] float2 each, or nullptr (then HW need not be a multiple of 64).
int launch_freeu(const bf16_t* hidden, bf16_t* hidden_out, float* hidden_part, int Ch, const bf16_t* skip, bf16_t* skip_out, float* skip_part, int Cs,
                 int B2, int H, int W, float b, float s, hipStream_t st) {
  const bool do_h = hidden_out != nullptr, do_s = skip_out != nullptr;
  if (!do_h && !do_s) { agd_set_error("freeu: nothing to do (b = 1 and s = 1 launch nothing)"); return -1; }
  if (B2 < 1 || H < 1 || W < 1 || (long long)H * W >= (1ll << 24) || (long long)B2 * H * W >= (1ll << 30)) { agd_set_error("freeu: %d maps of %d x %d", B2, H, W); return -1; }
  if ((do_h && (!hidden || Ch < 8 || Ch % 8)) || (do_s && (!skip || Cs < 8 || Cs % 8))) {
    agd_set_error("freeu: %d backbone / %d skip channels (multiples of 8)", Ch, Cs); return -1; }
  const int HW = H * W;
  if (((do_h && hidden_part) || (do_s && skip_part)) && HW % 64) { agd_set_error("freeu: 64-row statistics tiles on maps of %d pixels", HW); return -1; }
  auto vc_of = [](int C) { const int nvec = C / 8; return nvec % 8 == 0 ? 8 : nvec % 4 == 0 ? 4 : nvec % 2 == 0 ? 2 : 1; };
  FreeuJob j0{}, j1{};
  if (do_s) { j0.x = skip; j0.y = skip_out; j0.part = skip_part; j0.C = Cs; j0.VC = vc_of(Cs); j0.nblk = B2 * (Cs / (j0.VC * 8)); }
  if (do_h) { j1.x = hidden; j1.y = hidden_out; j1.part = hidden_part; j1.C = Ch; j1.VC = vc_of(Ch); j1.nblk = B2 * (Ch / (j1.VC * 8)); }
  const float g = (s - 1.f) / (float)HW;
  hipLaunchKernelGGL(freeu_kernel, dim3((unsigned)(j0.nblk + j1.nblk)), dim3(256), 0, st, j0, j1, H, W, g, b, Ch / 2);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
