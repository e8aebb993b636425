// MultiDiffusion panorama (diffusers StableDiffusionPanoramaPipeline [upstream-knowledge]) byte movers: the window gather that cuts views out
// of the canvas, the overlap mean that fuses stepped views (or per-view heat maps) back into it, and the row tiling that replicates the
// projected context per view.  The UNet, the CFG + DDIM step and the per-view DAAM map are the txt2img launches.
//
// Views: nbh x nbw windows of win x win at (i stride, j stride), view v = i nbw + j (row-major, diffusers get_views).  A view buffer holds
// images of [C][win][win] fp32; image of (panorama p, view v) = p * pano_stride + v * view_stride, so the same kernels serve the op layout
// (view-major within a panorama: pano_stride = views, view_stride = 1) and the denoise loop's (panorama-major within a view: 1, B).
#include "kernels.h"

static inline int grid_for(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g)); }

int pano_view_grid(int Lh, int Lw, int win, int stride, int* nbh, int* nbw) {
  if (win < 1 || stride < 1 || Lh < win || Lw < win) { agd_set_error("panorama: latent size %d x %d, window %d, stride %d (each side at least the window)", Lh, Lw, win, stride); return -1; }
  *nbh = (Lh - win) / stride + 1; *nbw = (Lw - win) / stride + 1;
  return 0;
}

template <int VEC> struct VecT { typedef float type; };
template <> struct VecT<4> { typedef f32x4 type; };

// One thread per VEC output elements of views [v0, v0 + n) of every panorama: plain loads from the canvas rows, plain stores.
template <int VEC>
__global__ void window_gather_kernel(const float* __restrict__ canvas, float* __restrict__ views, int B, int C, int Lh, int Lw, int win,
                                     int stride, int nbw, int v0, int n, long long pano_stride, long long view_stride) {
  typedef typename VecT<VEC>::type V;
  const int wv = win / VEC;
  const long long total = (long long)B * n * C * win * wv;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int xx = (int)(t % wv) * VEC;
    long long r = t / wv;
    const int yy = (int)(r % win); r /= win;
    const int c = (int)(r % C); r /= C;
    const int vv = (int)(r % n);
    const int p = (int)(r / n);
    const int v = v0 + vv, i = v / nbw, j = v - i * nbw;
    const long long src = (((long long)p * C + c) * Lh + (i * stride + yy)) * Lw + (j * stride + xx);
    const long long dst = (((long long)p * pano_stride + (long long)vv * view_stride) * C + c) * win * win + (long long)yy * win + xx;
    *(V*)(views + dst) = *(const V*)(canvas + src);
  }
}

// One thread per VEC canvas elements: the views that cover it are rows i0..i1 x columns j0..j1 of the view grid; they are added in
// ascending view order in fp32 (diffusers' `value[view] += stepped` order) and divided by their number -- no atomics, no value / count
// buffers.  VEC = 4 needs stride, win and Lw multiples of 4: the four elements then share their covering views.  An element no view
// covers (sizes off the stride grid) gets 0, diffusers' `where(count > 0, value / count, value)`.
template <int VEC>
__global__ void window_mean_kernel(const float* __restrict__ views, float* __restrict__ canvas, int B, int C, int Lh, int Lw, int win,
                                   int stride, int nbh, int nbw, long long pano_stride, long long view_stride) {
  typedef typename VecT<VEC>::type V;
  const int lwv = Lw / VEC;
  const long long total = (long long)B * C * Lh * lwv;
  const long long img = (long long)C * win * win;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(t % lwv) * VEC;
    long long r = t / lwv;
    const int y = (int)(r % Lh); r /= Lh;
    const int c = (int)(r % C);
    const int p = (int)(r / C);
    const int i0 = y < win ? 0 : (y - win) / stride + 1, j0 = x < win ? 0 : (x - win) / stride + 1;
    int i1 = y / stride, j1 = x / stride;
    i1 = i1 < nbh - 1 ? i1 : nbh - 1; j1 = j1 < nbw - 1 ? j1 : nbw - 1;
    V sum = {};
    int cnt = 0;
    for (int i = i0; i <= i1; ++i)
      for (int j = j0; j <= j1; ++j) {
        const long long v = (long long)i * nbw + j;
        sum += *(const V*)(views + ((long long)p * pano_stride + v * view_stride) * img + (long long)c * win * win +
                           (long long)(y - i * stride) * win + (x - j * stride));
        ++cnt;
      }
    if (cnt > 0) {
      const float d = (float)cnt;
      if constexpr (VEC == 4) { sum[0] = __fdiv_rn(sum[0], d); sum[1] = __fdiv_rn(sum[1], d); sum[2] = __fdiv_rn(sum[2], d); sum[3] = __fdiv_rn(sum[3], d); }
      else sum = __fdiv_rn(sum, d);
    }
    *(V*)(canvas + t * VEC) = sum;
  }
}

static bool vec4_ok(const void* a, const void* b, int Lw, int win, int stride) {
  return Lw % 4 == 0 && win % 4 == 0 && stride % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

int launch_window_gather(const float* canvas, float* views, int B, int C, int Lh, int Lw, int win, int stride, int v0, int n,
                         long long pano_stride, long long view_stride, hipStream_t st) {
  int nbh, nbw;
  if (pano_view_grid(Lh, Lw, win, stride, &nbh, &nbw)) return -1;
  if (B < 1 || C < 1 || v0 < 0 || n < 1 || v0 + n > nbh * nbw) { agd_set_error("window_gather: batch %d, channels %d, views [%d, %d) of %d", B, C, v0, v0 + n, nbh * nbw); return -1; }
  const long long total = (long long)B * n * C * win * win;
  if (vec4_ok(canvas, views, Lw, win, stride))
    hipLaunchKernelGGL(window_gather_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, st, canvas, views, B, C, Lh, Lw, win, stride, nbw, v0, n, pano_stride, view_stride);
  else
    hipLaunchKernelGGL(window_gather_kernel<1>, dim3(grid_for(total)), dim3(256), 0, st, canvas, views, B, C, Lh, Lw, win, stride, nbw, v0, n, pano_stride, view_stride);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

int launch_window_mean(const float* views, float* canvas, int B, int C, int Lh, int Lw, int win, int stride, long long pano_stride,
                       long long view_stride, hipStream_t st) {
  int nbh, nbw;
  if (pano_view_grid(Lh, Lw, win, stride, &nbh, &nbw)) return -1;
  if (B < 1 || C < 1) { agd_set_error("window_mean: batch %d, channels %d", B, C); return -1; }
  const long long total = (long long)B * C * Lh * Lw;
  if (vec4_ok(canvas, views, Lw, win, stride))
    hipLaunchKernelGGL(window_mean_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, st, views, canvas, B, C, Lh, Lw, win, stride, nbh, nbw, pano_stride, view_stride);
  else
    hipLaunchKernelGGL(window_mean_kernel<1>, dim3(grid_for(total)), dim3(256), 0, st, views, canvas, B, C, Lh, Lw, win, stride, nbh, nbw, pano_stride, view_stride);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}

// dst [halves][B * reps][row] = src [halves][B][row] with row r of a half reading row r % B: the CFG context of B prompts replicated for
// `reps` views per prompt (UNet batch order within a half: view-major, panorama-minor).  Rows are copied in 16-byte (or 4-byte) units.
template <typename U>
__global__ void tile_rows_kernel(const U* __restrict__ src, U* __restrict__ dst, int halves, int B, int reps, long long row_units) {
  const long long total = (long long)halves * B * reps * row_units;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long u = t % row_units, r = t / row_units;
    const int h = (int)(r / ((long long)B * reps)), b = (int)(r % B);
    dst[t] = src[((long long)h * B + b) * row_units + u];
  }
}
int launch_tile_rows(const void* src, void* dst, int halves, int B, int reps, size_t row_bytes, hipStream_t st) {
  if (halves < 1 || B < 1 || reps < 1 || row_bytes % 4) { agd_set_error("tile_rows: %d x %d rows x %d of %zu bytes", halves, B, reps, row_bytes); return -1; }
  const bool v16 = row_bytes % 16 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  const long long units = (long long)(row_bytes / (v16 ? 16 : 4));
  const long long total = (long long)halves * B * reps * units;
  if (v16) hipLaunchKernelGGL(tile_rows_kernel<u32x4>, dim3(grid_for(total)), dim3(256), 0, st, (const u32x4*)src, (u32x4*)dst, halves, B, reps, units);
  else hipLaunchKernelGGL(tile_rows_kernel<unsigned int>, dim3(grid_for(total)), dim3(256), 0, st, (const unsigned int*)src, (unsigned int*)dst, halves, B, reps, units);
  HIP_CHECK_RET(hipGetLastError()); return 0;
}
