// Elastic deformation (Simard et al. 2003; A.ElasticTransform) for the GPU input pipeline, as two entry points:
//   sepblur_reflect_f32 : separable 1-D correlation of fp32 planes with caller-supplied taps, along H then along W (scipy's axis
//                         order), scipy's mode='reflect' (half-sample symmetric, d c b a | a b c d | d c b a, period 2n) at both ends.
//                         The kernel knows nothing about Gaussians; utils/elastic.py hands it scipy's truncated Gaussian.
//   warp_field_u8       : warp_u8 with a per-pixel displacement added to the destination coordinate before the affine map,
//                         out(p) = src(M (p + alpha d(p))), one interpolation for both (sampling code: warp_sample.hpp).
//
// Blur kernels.  Both passes stage the *extended* signal (reflection resolved while staging) of one output tile into LDS, so the
// tap loop is a straight sliding window with no index arithmetic, and both read and write global memory along W:
//   H pass: a workgroup owns a strip of 64 columns x 64 output rows; a wave reads / writes one 256-byte row segment per access.
//           A thread owns one column and 16 consecutive rows and slides a 16-register window down the column: one LDS read and
//           16 FMAs per tap.
//   W pass: a workgroup owns 8 rows x 256 columns; a thread owns one column of the 8 rows: one LDS read (consecutive lanes,
//           consecutive banks) and one FMA per tap and output.
// The taps are read with a wave-uniform index (scalar loads).  The halo a tile needs grows with R, the LDS does not: the taps are
// walked in chunks (H: 192, W: 256) and the tile is re-staged per chunk, so any R up to MI355_BLUR_MAX_RADIUS and any H, W >= 1
// fit in 64 KiB (H) / 16 KiB (W) of LDS; at R <= 95 (H) and R <= 127 (W) a tile is staged exactly once.  Every output is one fp32
// FMA chain over k = 0 .. 2R in ascending order; no atomics: two runs give the same bits.
#include "common.hpp"
#include "warp_sample.hpp"

#define BLUR_MAX_RADIUS 1024

// index of position e of the half-sample symmetric extension of an n-element axis (any e)
__device__ __forceinline__ int reflect_sym(int e, int n) {
  const int p = 2 * n;
  int m = e % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

constexpr int HB_COLS = 64, HB_ROWS = 64, HB_PER = 16, HB_CHUNK = 192, HB_LDS_ROWS = HB_ROWS + HB_CHUNK;   // 256 rows x 256 B = 64 KiB

// grid: planes * tilesY * tilesX workgroups of 256 threads (4 waves: wave w owns rows 16w .. 16w+15 of the tile)
__global__ __launch_bounds__(256) void sepblur_h_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ taps,
                                                        int R, int H, int W, int tilesX, int tilesY) {
  __shared__ float lds[HB_LDS_ROWS * HB_COLS];
  int b = blockIdx.x;
  const int tx_ = b % tilesX; b /= tilesX;
  const int ty_ = b % tilesY;
  const size_t plane = (size_t)(b / tilesY) * H * W;
  const int x0 = tx_ * HB_COLS, y0 = ty_ * HB_ROWS;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = x0 + lane;
  const int ntaps = 2 * R + 1;
  float acc[HB_PER];
#pragma unroll
  for (int i = 0; i < HB_PER; ++i) acc[i] = 0.f;
  for (int k0 = 0; k0 < ntaps; k0 += HB_CHUNK) {
    const int kc = min(HB_CHUNK, ntaps - k0);
    const int rows = HB_ROWS + kc - 1;                   // LDS row j holds extended row y0 - R + k0 + j
    if (k0) __syncthreads();                             // the previous chunk's window reads are done
    for (int j = wv; j < rows; j += 4) {
      const int yy = reflect_sym(y0 - R + k0 + j, H);
      lds[j * HB_COLS + lane] = x < W ? src[plane + (size_t)yy * W + x] : 0.f;
    }
    __syncthreads();
    const float* col = lds + (wv * HB_PER) * HB_COLS + lane;       // col[(i + kk) * 64]: row i of this thread under tap k0 + kk
    const int full = kc & ~(HB_PER - 1);
    float w[HB_PER];
    if (full) {
#pragma unroll
      for (int i = 0; i < HB_PER; ++i) w[i] = col[i * HB_COLS];
    }
    for (int kk = 0; kk < full; kk += HB_PER) {
      // at step j, w[(i + j) & 15] holds col[(i + kk + j) * 64]; the slot of element 0 then takes element 16 (highest row read:
      // 48 + 15 + kc - 1 + 1 <= 255, inside the array; the last one read is never used)
#pragma unroll
      for (int j = 0; j < HB_PER; ++j) {
        const float t = taps[k0 + kk + j];
#pragma unroll
        for (int i = 0; i < HB_PER; ++i) acc[i] = __builtin_fmaf(t, w[(i + j) & (HB_PER - 1)], acc[i]);
        w[j] = col[(kk + j + HB_PER) * HB_COLS];
      }
    }
    for (int kk = full; kk < kc; ++kk) {                 // at most 15 taps of the last chunk
      const float t = taps[k0 + kk];
#pragma unroll
      for (int i = 0; i < HB_PER; ++i) acc[i] = __builtin_fmaf(t, col[(i + kk) * HB_COLS], acc[i]);
    }
  }
  if (x < W) {
#pragma unroll
    for (int i = 0; i < HB_PER; ++i) {
      const int y = y0 + wv * HB_PER + i;
      if (y < H) dst[plane + (size_t)y * W + x] = acc[i];
    }
  }
}

constexpr int WB_COLS = 256, WB_ROWS = 8, WB_CHUNK = 256, WB_LDS_COLS = WB_COLS + WB_CHUNK;                // 8 rows x 2 KiB = 16 KiB

// grid: planes * tilesY * tilesX workgroups of 256 threads (thread = column of the tile)
__global__ __launch_bounds__(256) void sepblur_w_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ taps,
                                                        int R, int H, int W, int tilesX, int tilesY) {
  __shared__ float lds[WB_ROWS * WB_LDS_COLS];
  int b = blockIdx.x;
  const int tx_ = b % tilesX; b /= tilesX;
  const int ty_ = b % tilesY;
  const size_t plane = (size_t)(b / tilesY) * H * W;
  const int x0 = tx_ * WB_COLS, y0 = ty_ * WB_ROWS;
  const int tid = threadIdx.x;
  const int ntaps = 2 * R + 1;
  float acc[WB_ROWS];
#pragma unroll
  for (int r = 0; r < WB_ROWS; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < ntaps; k0 += WB_CHUNK) {
    const int kc = min(WB_CHUNK, ntaps - k0);
    const int cols = WB_COLS + kc - 1;                   // LDS column j holds extended column x0 - R + k0 + j (cols <= 511)
    if (k0) __syncthreads();
    for (int j = tid; j < cols; j += 256) {
      const int xx = reflect_sym(x0 - R + k0 + j, W);
#pragma unroll
      for (int r = 0; r < WB_ROWS; ++r) lds[r * WB_LDS_COLS + j] = y0 + r < H ? src[plane + (size_t)(y0 + r) * W + xx] : 0.f;
    }
    __syncthreads();
    const float* row = lds + tid;
#pragma unroll 4
    for (int kk = 0; kk < kc; ++kk) {
      const float t = taps[k0 + kk];
#pragma unroll
      for (int r = 0; r < WB_ROWS; ++r) acc[r] = __builtin_fmaf(t, row[r * WB_LDS_COLS + kk], acc[r]);
    }
  }
  const int x = x0 + tid;
  if (x < W) {
#pragma unroll
    for (int r = 0; r < WB_ROWS; ++r)
      if (y0 + r < H) dst[plane + (size_t)(y0 + r) * W + x] = acc[r];
  }
}

extern "C" int mi355_sepblur_reflect_f32(const float* src, int planes, int H, int W, const float* taps, int radius, float* tmp, float* dst,
                                         mi355_stream_t s) {
  MI355_CHECK_ARG(src, "sepblur_reflect_f32: null pointer (src)");
  MI355_CHECK_ARG(taps, "sepblur_reflect_f32: null pointer (taps)");
  MI355_CHECK_ARG(tmp, "sepblur_reflect_f32: null pointer (tmp)");
  MI355_CHECK_ARG(dst, "sepblur_reflect_f32: null pointer (dst)");
  MI355_CHECK_ARG(planes > 0 && H > 0 && W > 0, "sepblur_reflect_f32: planes, H, W must be positive (%d, %d, %d)", planes, H, W);
  MI355_CHECK_ARG(radius >= 0 && radius <= BLUR_MAX_RADIUS, "sepblur_reflect_f32: radius %d outside 0 .. %d", radius, BLUR_MAX_RADIUS);
  MI355_CHECK_ARG(src != tmp && src != dst && tmp != dst, "sepblur_reflect_f32: src, tmp and dst must not alias");
  MI355_CHECK_ARG(H <= (1 << 29) && W <= (1 << 29), "sepblur_reflect_f32: H, W above 2^29 (%d, %d)", H, W);
  const int hx = ceil_div(W, HB_COLS), hy = ceil_div(H, HB_ROWS), wx = ceil_div(W, WB_COLS), wy = ceil_div(H, WB_ROWS);
  const long long hblocks = (long long)planes * hy * hx, wblocks = (long long)planes * wy * wx;
  MI355_CHECK_ARG(hblocks <= 0x7fffffffLL && wblocks <= 0x7fffffffLL, "sepblur_reflect_f32: %d planes of %d x %d need more than 2^31 - 1 tiles",
                  planes, H, W);
  hipLaunchKernelGGL(sepblur_h_kernel, dim3((unsigned)hblocks), dim3(256), 0, (hipStream_t)s, src, tmp, taps, radius, H, W, hx, hy);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(sepblur_w_kernel, dim3((unsigned)wblocks), dim3(256), 0, (hipStream_t)s, (const float*)tmp, dst, taps, radius, H, W, wx, wy);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// field: [N][2][H][W] fp32 (dx, dy) at destination resolution; alpha: [N]; m as in warp_u8
__global__ void warp_field_u8_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, const float* __restrict__ m,
                                     const float* __restrict__ field, const float* __restrict__ alpha, uint8_t* __restrict__ dst, int H, int W,
                                     int C, int nearest, int reflect, long long total) {
#pragma clang fp contract(off)      // as warp_u8_kernel: the coordinates are a plain IEEE evaluation, in the order of the header's formula
  const size_t hw = (size_t)H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    long long r = i / W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    const float* mm = m + (size_t)n * 6;
    const float* f = field + (size_t)n * 2 * hw + (size_t)y * W + x;
    const float a = alpha[n];
    const float px = x + a * f[0], py = y + a * f[hw];
    const float sx = mm[0] * px + mm[1] * py + mm[2], sy = mm[3] * px + mm[4] * py + mm[5];
    warp_sample_u8(src + (size_t)n * Hs * Ws * C, Hs, Ws, C, sx, sy, dst + ((size_t)(n * H + y) * W + x) * C, nearest, reflect);
  }
}

extern "C" int mi355_warp_field_u8(const uint8_t* src, int N, int Hs, int Ws, int C, const float* m, const float* field, const float* alpha,
                                   uint8_t* dst, int H, int W, int nearest, int reflect, mi355_stream_t s) {
  MI355_CHECK_ARG(src, "warp_field_u8: null pointer (src)");
  MI355_CHECK_ARG(m, "warp_field_u8: null pointer (m)");
  MI355_CHECK_ARG(field, "warp_field_u8: null pointer (field)");
  MI355_CHECK_ARG(alpha, "warp_field_u8: null pointer (alpha)");
  MI355_CHECK_ARG(dst, "warp_field_u8: null pointer (dst)");
  MI355_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "warp_field_u8: N, Hs, Ws, H, W must be positive (%d, %d, %d, %d, %d)", N, Hs, Ws,
                  H, W);
  MI355_CHECK_ARG(C > 0 && C <= 4, "warp_field_u8: C = %d outside 1 .. 4", C);
  MI355_CHECK_ARG((const void*)src != (const void*)dst, "warp_field_u8: src and dst must not alias");
  const long long total = (long long)N * H * W;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(warp_field_u8_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)s, src, Hs, Ws, m, field, alpha, dst, H, W, C, nearest,
                     reflect, total);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
