// Surface-distance metrics of binary segmentation masks: the raw, exact quantities behind Hausdorff distance, its percentile
// (HD95), average symmetric surface distance and surface Dice (utils/tester.py turns them into the final values).
//
// For unit pixel spacing every squared distance is an integer, so everything but the two sums of square roots is integer
// arithmetic and is reproduced bit for bit; the sums are fp64, added in an order that depends on the shape alone.  Four launches on
// the caller's stream, all scratch in the caller's workspace ws = [g2 / d2 towards T: B H W int32][g2 / d2 towards P: B H W int32]
// [border bytes: B H W, bit 0 = border of P, bit 1 = border of T]:
//
//   surface_border_kernel    binarises both maps (the expression of seg_counts_kernel, loss_optim.hip) and marks the pixels of a mask
//                            that have a 4-neighbour outside it (outside the image = background)
//   surface_column_kernel    g2(y, x) = squared vertical distance to the nearest border pixel of the OTHER mask in column x
//                            (SURFACE_NONE^2 when the column has none): 64 rows of a column are one 64-bit word per thread, the
//                            nearest set bit above / below is a count of leading / trailing zeros, neighbouring segments meet in LDS
//   surface_row_kernel       d2(y, x) = min_x' (x - x')^2 + g2(y, x') at the border pixels of the source mask, -1 elsewhere, written
//                            over g2: the row of g2 sits in LDS, every lane reads the same address (a broadcast, no bank conflict),
//                            waves without a source pixel skip the loop — the O(H W W) part
//   surface_stats_kernel     one workgroup per sample: counts, maxima, within-tolerance counts and the fp64 sums in one sweep, then
//                            the two order statistics by a three-digit radix select (LDS histograms filled with INTEGER atomics,
//                            which commute) and one "smallest value above" sweep
#include "common.hpp"

#define SURFACE_MAX_SIDE 1024
#define SURFACE_NONE 16384                        /* "no border pixel in this column": NONE^2 + 1279^2 still fits an int32 ... */
#define SURFACE_NONE2 (SURFACE_NONE * SURFACE_NONE) /* ... and every real d2 <= 2 * 1023^2 = 2 093 058 < 2^21 is far below it */
#define SURFACE_SEGS 16                           /* segments of a column (one wave each): ceil(H / 16) <= 64 rows = one word */

__device__ __forceinline__ bool surface_on(float v, int is_logit, float thr) {
  if (is_logit) v = 1.f / (1.f + __expf(-v));
  return v > thr;
}

// inside the mask, and at least one of the four neighbours is not
__device__ __forceinline__ unsigned surface_is_border(const float* __restrict__ m, int y, int x, int H, int W, int is_logit, float thr) {
  const float* c = m + (size_t)y * W + x;
  if (!surface_on(c[0], is_logit, thr)) return 0u;
  const bool l = x > 0 && surface_on(c[-1], is_logit, thr);
  const bool r = x + 1 < W && surface_on(c[1], is_logit, thr);
  const bool u = y > 0 && surface_on(c[-W], is_logit, thr);
  const bool d = y + 1 < H && surface_on(c[W], is_logit, thr);
  return (l && r && u && d) ? 0u : 1u;
}

// grid (ceil(W / 256), H, B)
__global__ __launch_bounds__(256) void surface_border_kernel(const float* __restrict__ pred, const float* __restrict__ target, int H, int W,
                                                             int is_logit, float thr, uint8_t* __restrict__ border) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const size_t img = (size_t)blockIdx.z * H * W;
  const unsigned bp = surface_is_border(pred + img, y, x, H, W, is_logit, thr);
  const unsigned bt = surface_is_border(target + img, y, x, H, W, 0, thr);
  border[img + (size_t)y * W + x] = (uint8_t)(bp | (bt << 1));
}

// grid (ceil(W / 64), B), 1024 threads: lane = column, wave = segment of S = ceil(H / 16) rows.
__global__ __launch_bounds__(1024) void surface_column_kernel(const uint8_t* __restrict__ border, int H, int W, int* __restrict__ g_t,
                                                              int* __restrict__ g_p) {
  __shared__ short first_y[2][SURFACE_SEGS][64], last_y[2][SURFACE_SEGS][64];      // -1: the segment has no border pixel
  const int col = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + col;
  const int S = (H + SURFACE_SEGS - 1) / SURFACE_SEGS;
  const int y0 = seg * S;
  const size_t img = (size_t)blockIdx.y * H * W;
  unsigned long long m[2] = {0ull, 0ull};      // m[0]: border of T (what P's pixels measure to), m[1]: border of P
  if (x < W) {
#pragma unroll 8
    for (int j = 0; j < S; ++j) {
      const int y = y0 + j;
      const unsigned ld = border[img + (size_t)(y < H ? y : H - 1) * W + x];      // (a clamped address, not a load under a condition)
      const unsigned v = y < H ? ld : 0u;
      m[0] |= (unsigned long long)((v >> 1) & 1u) << j;
      m[1] |= (unsigned long long)(v & 1u) << j;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    first_y[k][seg][col] = m[k] ? (short)(y0 + __builtin_ctzll(m[k])) : (short)-1;
    last_y[k][seg][col] = m[k] ? (short)(y0 + 63 - __builtin_clzll(m[k])) : (short)-1;
  }
  __syncthreads();
  if (x >= W) return;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    int above = -1, below = -1;                // nearest border row of the segments above / below this one
    for (int q = seg - 1; q >= 0 && above < 0; --q) above = last_y[k][q][col];
    for (int q = seg + 1; q < SURFACE_SEGS && below < 0; ++q) below = first_y[k][q][col];
    int* __restrict__ g = (k == 0 ? g_t : g_p) + img + x;
    const unsigned long long w = m[k];
    for (int j = 0; j < S; ++j) {
      const int y = y0 + j;
      if (y >= H) break;
      const unsigned long long up = w & ((2ull << j) - 1ull);      // rows y0 .. y (2 << 63 wraps to 0: every bit)
      const unsigned long long dn = w >> j;                        // rows y .. y0 + 63
      const int du = up ? j - (63 - __builtin_clzll(up)) : (above >= 0 ? y - above : SURFACE_NONE);
      const int dd = dn ? __builtin_ctzll(dn) : (below >= 0 ? below - y : SURFACE_NONE);
      const int d = du < dd ? du : dd;
      g[(size_t)y * W] = d * d;
    }
  }
}

// grid (H, B, 2), 256 threads: block (y, b, k) turns row y of g2 towards T (k = 0, sources = border of P) or towards P (k = 1) into d2.
__global__ __launch_bounds__(256) void surface_row_kernel(const uint8_t* __restrict__ border, int H, int W, int* __restrict__ g_t,
                                                          int* __restrict__ g_p) {
  __shared__ __attribute__((aligned(16))) int row[SURFACE_MAX_SIDE];
  const int k = blockIdx.z;
  const size_t off = ((size_t)blockIdx.y * H + blockIdx.x) * W;
  int* __restrict__ g = (k == 0 ? g_t : g_p) + off;
  const uint8_t* __restrict__ bd = border + off;
  const int W4 = (W + 3) & ~3;
  for (int x = threadIdx.x; x < W4; x += 256) row[x] = x < W ? g[x] : SURFACE_NONE2;
  __syncthreads();
  for (int x0 = 0; x0 < W; x0 += 256) {
    const int x = x0 + threadIdx.x;
    const bool src = x < W && ((bd[x < W ? x : 0] >> k) & 1u);
    int best = -1;
    if (__any(src)) {                          // wave-uniform: 64 consecutive pixels without a source pixel cost nothing
      best = 0x7fffffff;
      for (int xp = 0; xp < W4; xp += 4) {
        const int4 v = *reinterpret_cast<const int4*>(row + xp);
        const int d0 = x - xp, d1 = d0 - 1, d2 = d0 - 2, d3 = d0 - 3;      // |d| < 2^11: the 24-bit multiply is exact
        best = min(best, __mul24(d0, d0) + v.x);
        best = min(best, __mul24(d1, d1) + v.y);
        best = min(best, __mul24(d2, d2) + v.z);
        best = min(best, __mul24(d3, d3) + v.w);
      }
      if (!src) best = -1;
    }
    if (x < W) g[x] = best;
  }
}

__device__ __forceinline__ int surface_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int surface_wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int surface_wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (B), 1024 threads.  d_all = [d2 of P's border towards T: B HW][d2 of T's border towards P: B HW], -1 off the source border.
// Rank lo of the non-negative entries by a radix select, eight bits a sweep from the top of a 24-bit key (`below` = entries under
// every key that starts with `prefix`), and with it the number of entries <= that value: the next rank is the same value or the
// smallest one above it.
__global__ __launch_bounds__(1024) void surface_stats_kernel(const int* __restrict__ d_all, long long BHW, int HW, int q, int tol2,
                                                             int* __restrict__ out_i, double* __restrict__ out_d) {
  __shared__ int red_i[16][6];
  __shared__ double red_d[16][2];
  __shared__ int hist[256];
  __shared__ int bcast[2];
  __shared__ long long n_le_s;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* __restrict__ dpt = d_all + (size_t)b * HW;            // d2 of P's border pixels towards T
  const int* __restrict__ dtp = d_all + BHW + (size_t)b * HW;      // d2 of T's border pixels towards P
  int cnt[2] = {0, 0}, mx[2] = {0, 0}, within[2] = {0, 0};
  double sum[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int* __restrict__ d = k == 0 ? dpt : dtp;
    for (int i = threadIdx.x; i < HW; i += 1024) {
      const int v = d[i];
      if (v >= 0) {
        ++cnt[k];
        mx[k] = max(mx[k], v);
        within[k] += v <= tol2;
        sum[k] += sqrt((double)v);
      }
    }
  }
  // thread -> wave -> workgroup, always in the same order
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    cnt[k] = surface_wave_sum_i(cnt[k]);
    mx[k] = surface_wave_max_i(mx[k]);
    within[k] = surface_wave_sum_i(within[k]);
    sum[k] = wave_sum_d(sum[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      red_i[wave][k] = cnt[k];
      red_i[wave][2 + k] = mx[k];
      red_i[wave][4 + k] = within[k];
      red_d[wave][k] = sum[k];
    }
  }
  __syncthreads();
  int tot[6] = {0, 0, 0, 0, 0, 0};
  double tsum[2] = {0.0, 0.0};
  for (int w = 0; w < 16; ++w) {
    tot[0] += red_i[w][0];
    tot[1] += red_i[w][1];
    tot[2] = max(tot[2], red_i[w][2]);
    tot[3] = max(tot[3], red_i[w][3]);
    tot[4] += red_i[w][4];
    tot[5] += red_i[w][5];
    tsum[0] += red_d[w][0];
    tsum[1] += red_d[w][1];
  }
  int* __restrict__ oi = out_i + (size_t)b * 8;
  double* __restrict__ od = out_d + (size_t)b * 2;
  if (tot[0] == 0 || tot[1] == 0) {            // (uniform over the workgroup) nothing to measure to: the counts say which case
    if (threadIdx.x < 8) oi[threadIdx.x] = threadIdx.x < 2 ? tot[threadIdx.x] : 0;
    if (threadIdx.x < 2) od[threadIdx.x] = 0.0;
    return;
  }
  // the concatenation of both directions is never formed: every sweep below walks the sample's two pieces
  const long long n = (long long)tot[0] + tot[1];
  const long long pos = (long long)q * (n - 1);
  const long long lo = pos / 100;
  const bool two = (pos % 100) != 0;
  // ---- radix select over the two ranges --------------------------------------------------------------------------------------
  int prefix = 0, in_bin = 0;
  long long below = 0;
  for (int shift = 16; shift >= 0; shift -= 8) {
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int* __restrict__ d = k == 0 ? dpt : dtp;
      for (int i = threadIdx.x; i < HW; i += 1024) {
        const int v = d[i];
        if (v >= 0 && (shift == 16 || (v >> (shift + 8)) == prefix)) atomicAdd(&hist[(v >> shift) & 255], 1);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long acc = below;
      int bin = 0;
      for (; bin < 255; ++bin) {
        if (acc + hist[bin] > lo) break;
        acc += hist[bin];
      }
      bcast[0] = bin;
      bcast[1] = hist[bin];
      n_le_s = acc;
    }
    __syncthreads();
    prefix = (prefix << 8) | bcast[0];
    in_bin = bcast[1];
    below = n_le_s;
    __syncthreads();
  }
  const int lo2 = prefix;
  int hi2 = lo2;
  if (two && lo + 1 >= below + in_bin) {       // (uniform) the next rank is the smallest value above lo2
    int nxt = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int* __restrict__ d = k == 0 ? dpt : dtp;
      for (int i = threadIdx.x; i < HW; i += 1024) {
        const int v = d[i];
        if (v > lo2) nxt = min(nxt, v);
      }
    }
    nxt = surface_wave_min_i(nxt);
    if (lane == 0) red_i[wave][0] = nxt;
    __syncthreads();
    nxt = red_i[0][0];
    for (int w = 1; w < 16; ++w) nxt = min(nxt, red_i[w][0]);
    hi2 = nxt;
  }
  if (threadIdx.x == 0) {
    oi[0] = tot[0];
    oi[1] = tot[1];
    oi[2] = tot[2];
    oi[3] = tot[3];
    oi[4] = lo2;
    oi[5] = hi2;
    oi[6] = tot[4];
    oi[7] = tot[5];
    od[0] = tsum[0];
    od[1] = tsum[1];
  }
}

static long long surface_ws_need(int B, int H, int W) {
  const long long n = (long long)B * H * W;
  return 2 * n + (n + 3) / 4;
}

#define SURFACE_MAX_B 65535      /* the sample index is a grid coordinate */
#define SURFACE_CHECK_SHAPE(who)                                                                                                  \
  MI355_CHECK_ARG(B > 0 && B <= SURFACE_MAX_B && H >= 1 && H <= SURFACE_MAX_SIDE && W >= 1 && W <= SURFACE_MAX_SIDE &&            \
                      surface_ws_need(B > 0 ? B : 1, H, W) <= 0x7fffffffLL,                                                       \
                  who ": 1 <= H, W <= %d, 0 < B <= %d and a workspace below 2^31 elements expected (B=%d, H=%d, W=%d)",           \
                  SURFACE_MAX_SIDE, SURFACE_MAX_B, B, H, W)

extern "C" int mi355_surface_ws_ints(int B, int H, int W) {
  SURFACE_CHECK_SHAPE("surface_ws_ints");
  return (int)surface_ws_need(B, H, W);
}

extern "C" int mi355_surface_distances(const float* pred, const float* target, int B, int H, int W, int is_logit, float thr, int q,
                                       int tol2, int32_t* ws, long long ws_ints, int32_t* out_i, double* out_d, mi355_stream_t s) {
  MI355_CHECK_ARG(pred && target && ws && out_i && out_d, "surface_distances: null pointer");
  SURFACE_CHECK_SHAPE("surface_distances");
  MI355_CHECK_ARG(q >= 0 && q <= 100, "surface_distances: percentile q=%d outside 0..100", q);
  MI355_CHECK_ARG(tol2 >= 0, "surface_distances: tol2=%d must not be negative", tol2);
  const long long need = surface_ws_need(B, H, W);
  MI355_CHECK_ARG(ws_ints >= need, "surface_distances: workspace of %lld int32 elements is too short, %lld needed (B=%d, H=%d, W=%d)",
                  ws_ints, need, B, H, W);
  MI355_CHECK_ARG(((uintptr_t)ws % 16) == 0, "surface_distances: ws must be 16-byte aligned");
  const long long n = (long long)B * H * W;
  int* g_t = ws;
  int* g_p = ws + n;
  uint8_t* border = reinterpret_cast<uint8_t*>(ws + 2 * n);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(surface_border_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, st, pred, target, H, W, is_logit ? 1 : 0, thr,
                     border);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(surface_column_kernel, dim3((W + 63) / 64, B), dim3(1024), 0, st, border, H, W, g_t, g_p);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(surface_row_kernel, dim3(H, B, 2), dim3(256), 0, st, border, H, W, g_t, g_p);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(surface_stats_kernel, dim3(B), dim3(1024), 0, st, ws, n, H * W, q, tol2, out_i, out_d);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
