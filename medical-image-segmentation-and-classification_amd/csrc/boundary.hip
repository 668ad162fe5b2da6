// Boundary loss (Kervadec et al., MIDL 2019) on the device: the signed squared Euclidean distance map of a binary target and the
// loss / gradient that consume it.
//
// Map.  T = target > thr (the expression of surface_on with is_logit = 0, surface.hip).  Per sample:
//   outside pixel:  sd2 = +min (dy^2 + dx^2) over the foreground pixels of the sample   (>= 1)
//   inside pixel:   sd2 = -min (dy^2 + dx^2) over the background pixels of the sample   (<= -1)
//   a sample without foreground or without background has no boundary: sd2 = 0 everywhere.
// Pixels outside the image are NOT background — unlike the border rule of surface.hip, where the frame cuts a mask open: a
// foreground that fills the image has no distance to measure, it does not get one to the frame.  Unit spacing makes every value an
// integer (|sd2| <= 2 * 1023^2 < 2^21), so the map is reproduced bit for bit.  Two launches, the two-pass scheme of surface.hip:
//
//   sdist_column_kernel   64 rows of a column are one 64-bit word per thread; per pixel the squared vertical distance to the nearest
//                         foreground pixel of its column goes to `sd2` (used as scratch), to the nearest background pixel to `ws`
//                         (SDIST_NONE^2 where the column has none)
//   sdist_row_kernel      one workgroup per row: both g2 rows sit in LDS, every pixel scans the row of the OPPOSITE class,
//                         d2(y, x) = min_x' (x - x')^2 + g2(y, x') — every lane reads the same address (a broadcast); a wave whose
//                         64 pixels are all of one class scans one row only.  A class that the sample lacks shows as
//                         best >= SDIST_NONE^2 and is written as 0: the degenerate-sample rule needs no reduction of its own.
//
// Loss.  phi = sqrt(sd2) (sd2 > 0), -(sqrt(-sd2) - 1) (sd2 < 0), 0 (sd2 = 0) — Kervadec's distance(neg) * neg - (distance(pos) - 1)
// * pos; loss = base + weight / n * sum sigmoid(z) phi, dz (+)= gscale weight / n * phi p (1 - p).  Deterministic as seg_loss.hip:
// one partial per workgroup, folded by one workgroup in a fixed order in double, no floating-point atomics.  Nothing is allocated,
// nothing synchronises, every scalar the launches need lives in device memory or in their arguments.
#include "common.hpp"

#define SDIST_MAX_SIDE 1024
#define SDIST_MAX_B 65535                       /* the sample index is a grid coordinate */
#define SDIST_NONE 16384                        /* "no such pixel in this column": NONE^2 + 1023^2 still fits an int32 ... */
#define SDIST_NONE2 (SDIST_NONE * SDIST_NONE)   /* ... and every real d2 <= 2 * 1023^2 is far below it */
#define SDIST_SEGS 16                           /* segments of a column (one wave each): ceil(H / 16) <= 64 rows = one word */

// grid (ceil(W / 64), B), 1024 threads: lane = column, wave = segment of S = ceil(H / 16) rows.
__global__ __launch_bounds__(1024) void sdist_column_kernel(const float* __restrict__ target, int H, int W, float thr,
                                                            int* __restrict__ g_fg, int* __restrict__ g_bg) {
  __shared__ short first_y[2][SDIST_SEGS][64], last_y[2][SDIST_SEGS][64];      // -1: the segment has no pixel of the class
  const int col = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + col;
  const int S = (H + SDIST_SEGS - 1) / SDIST_SEGS;
  const int y0 = seg * S;
  const size_t img = (size_t)blockIdx.y * H * W;
  unsigned long long m[2] = {0ull, 0ull};      // m[0]: foreground rows of the segment, m[1]: background rows (rows >= H are neither)
  if (x < W) {
#pragma unroll 8
    for (int j = 0; j < S; ++j) {
      const int y = y0 + j;
      const float v = target[img + (size_t)(y < H ? y : H - 1) * W + x];      // (a clamped address, not a load under a condition)
      const unsigned long long in = y < H ? 1ull : 0ull;
      const unsigned long long on = v > thr ? 1ull : 0ull;
      m[0] |= (in & on) << j;
      m[1] |= (in & (on ^ 1ull)) << j;
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
    int above = -1, below = -1;                // nearest row of the class in the segments above / below this one
    for (int q = seg - 1; q >= 0 && above < 0; --q) above = last_y[k][q][col];
    for (int q = seg + 1; q < SDIST_SEGS && below < 0; ++q) below = first_y[k][q][col];
    int* __restrict__ g = (k == 0 ? g_fg : g_bg) + img + x;
    const unsigned long long w = m[k];
    for (int j = 0; j < S; ++j) {
      const int y = y0 + j;
      if (y >= H) break;
      const unsigned long long up = w & ((2ull << j) - 1ull);      // rows y0 .. y (2 << 63 wraps to 0: every bit)
      const unsigned long long dn = w >> j;                        // rows y .. y0 + 63
      const int du = up ? j - (63 - __builtin_clzll(up)) : (above >= 0 ? y - above : SDIST_NONE);
      const int dd = dn ? __builtin_ctzll(dn) : (below >= 0 ? below - y : SDIST_NONE);
      const int d = du < dd ? du : dd;
      g[(size_t)y * W] = d * d;
    }
  }
}

__device__ __forceinline__ int sdist_scan(const int* __restrict__ row, int x, int W4) {
  int best = 0x7fffffff;
  for (int xp = 0; xp < W4; xp += 4) {
    const int4 v = *reinterpret_cast<const int4*>(row + xp);
    const int d0 = x - xp, d1 = d0 - 1, d2 = d0 - 2, d3 = d0 - 3;      // |d| < 2^11: the 24-bit multiply is exact
    best = min(best, __mul24(d0, d0) + v.x);
    best = min(best, __mul24(d1, d1) + v.y);
    best = min(best, __mul24(d2, d2) + v.z);
    best = min(best, __mul24(d3, d3) + v.w);
  }
  return best;
}

// grid (H, B), 256 threads: block (y, b) turns row y of both g2 maps into the signed d2, written over the foreground map.
__global__ __launch_bounds__(256) void sdist_row_kernel(int H, int W, int* __restrict__ sd2, const int* __restrict__ g_bg) {
  __shared__ __attribute__((aligned(16))) int row_fg[SDIST_MAX_SIDE];
  __shared__ __attribute__((aligned(16))) int row_bg[SDIST_MAX_SIDE];
  const size_t off = ((size_t)blockIdx.y * H + blockIdx.x) * W;
  int* __restrict__ out = sd2 + off;
  const int* __restrict__ gb = g_bg + off;
  const int W4 = (W + 3) & ~3;
  for (int x = threadIdx.x; x < W4; x += 256) {
    row_fg[x] = x < W ? out[x] : SDIST_NONE2;
    row_bg[x] = x < W ? gb[x] : SDIST_NONE2;
  }
  __syncthreads();                             // the whole row is in LDS before any of it is overwritten
  for (int x0 = 0; x0 < W; x0 += 256) {
    const int x = x0 + threadIdx.x;
    const bool live = x < W;
    const bool inside = live && row_fg[live ? x : 0] == 0;      // a foreground pixel is its own nearest foreground pixel
    int best = SDIST_NONE2;
    // wave-uniform branches: 64 consecutive pixels of one class cost one scan
    if (__any(live && !inside)) {
      const int b = sdist_scan(row_fg, x, W4);
      if (!inside) best = b;
    }
    if (__any(inside)) {
      const int b = sdist_scan(row_bg, x, W4);
      if (inside) best = b;
    }
    if (live) out[x] = best >= SDIST_NONE2 ? 0 : (inside ? -best : best);
  }
}

static long long sdist_ws_need(int B, int H, int W) { return (long long)B * H * W; }

#define SDIST_CHECK_SHAPE(who)                                                                                                    \
  MI355_CHECK_ARG(B > 0 && B <= SDIST_MAX_B && H >= 1 && H <= SDIST_MAX_SIDE && W >= 1 && W <= SDIST_MAX_SIDE &&                  \
                      sdist_ws_need(B > 0 ? B : 1, H, W) <= 0x7fffffffLL,                                                         \
                  who ": 1 <= H, W <= %d, 0 < B <= %d and a workspace below 2^31 elements expected (B=%d, H=%d, W=%d)",           \
                  SDIST_MAX_SIDE, SDIST_MAX_B, B, H, W)

extern "C" int mi355_sdist_ws_ints(int B, int H, int W) {
  SDIST_CHECK_SHAPE("sdist_ws_ints");
  return (int)sdist_ws_need(B, H, W);
}

extern "C" int mi355_signed_dist2(const float* target, int B, int H, int W, float thr, int32_t* ws, long long ws_ints, int32_t* sd2,
                                  mi355_stream_t s) {
  MI355_CHECK_ARG(target, "signed_dist2: null pointer (target)");
  MI355_CHECK_ARG(ws, "signed_dist2: null pointer (ws)");
  MI355_CHECK_ARG(sd2, "signed_dist2: null pointer (sd2)");
  SDIST_CHECK_SHAPE("signed_dist2");
  const long long need = sdist_ws_need(B, H, W);
  MI355_CHECK_ARG(ws_ints >= need, "signed_dist2: workspace ws of %lld int32 elements is too short, %lld needed (B=%d, H=%d, W=%d)",
                  ws_ints, need, B, H, W);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(sdist_column_kernel, dim3((W + 63) / 64, B), dim3(1024), 0, st, target, H, W, thr, sd2, ws);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(sdist_row_kernel, dim3(H, B), dim3(256), 0, st, H, W, sd2, ws);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- the loss --------------------------------------------------------------------------------------------------------------------
template <int E> struct alignas(4 * E) BndVecF { float v[E]; };
template <int E> struct alignas(4 * E) BndVecI { int v[E]; };

// |sd2| < 2^24 converts exactly; sqrtf is correctly rounded
__device__ __forceinline__ float bnd_phi(int sd2) {
  return sd2 > 0 ? sqrtf((float)sd2) : (sd2 < 0 ? 1.f - sqrtf((float)(-sd2)) : 0.f);
}

// the forms of seg_sigmoid (seg_loss.hip): e = exp(-|x|) never overflows, p (1 - p) = e s^2 on both sides
__device__ __forceinline__ void bnd_sigmoid(float x, float& p, float& pq) {
  const float e = __expf(-fabsf(x));
  const float s = __builtin_amdgcn_rcpf(1.f + e);
  p = x >= 0.f ? s : e * s;
  pq = (e * s) * s;
}

// grid (gx, B): workgroup (g, b) strides over sample b's vectors; partial[b * gx + g] = its sum of p phi.
template <int E>
__global__ __launch_bounds__(256) void boundary_fwd_kernel(const float* __restrict__ z, const int* __restrict__ sd2, long long per,
                                                           float* __restrict__ partial) {
  typedef BndVecF<E> VF;
  typedef BndVecI<E> VI;
  const int b = blockIdx.y;
  const VF* __restrict__ zv = reinterpret_cast<const VF*>(z + (size_t)b * per);
  const VI* __restrict__ dv = reinterpret_cast<const VI*>(sd2 + (size_t)b * per);
  const long long nv = per / E;
  const long long st = (long long)gridDim.x * 256;
  float acc[E];
#pragma unroll
  for (int k = 0; k < E; ++k) acc[k] = 0.f;
#pragma unroll 4
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += st) {
    const VF a = zv[i];
    const VI d = dv[i];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      float p, pq;
      bnd_sigmoid(a.v[k], p, pq);
      acc[k] += p * bnd_phi(d.v[k]);
    }
  }
  // thread -> wave -> workgroup, in double, always in the same order
  __shared__ double red[4];
  double v = 0;
#pragma unroll
  for (int k = 0; k < E; ++k) v += (double)acc[k];
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

// One workgroup: thread t folds rows t, t + 256, ..., then lanes, then the four waves in wave order.
__global__ __launch_bounds__(256) void boundary_finalize_kernel(const float* __restrict__ partial, int rows, double scale,
                                                                const float* __restrict__ base, float* __restrict__ loss) {
  double v = 0;
  for (int i = threadIdx.x; i < rows; i += 256) v += (double)partial[i];
  v = wave_sum_d(v);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((base ? (double)base[0] : 0.0) + scale * ((red[0] + red[1]) + (red[2] + red[3])));
}

// grid (gx, B), the forward's sweep: dz (+)= gscale[0] * c * phi p (1 - p), c = weight / (B per).
template <int E, bool ACC>
__global__ __launch_bounds__(256) void boundary_bwd_kernel(const float* __restrict__ z, const int* __restrict__ sd2, long long per,
                                                           float c, const float* __restrict__ gscale, float* __restrict__ dz) {
#pragma clang fp contract(off)      /* accumulate adds the ROUNDED term: two launches give what one launch plus a sum gives */
  typedef BndVecF<E> VF;
  typedef BndVecI<E> VI;
  const int b = blockIdx.y;
  const VF* __restrict__ zv = reinterpret_cast<const VF*>(z + (size_t)b * per);
  const VI* __restrict__ dv = reinterpret_cast<const VI*>(sd2 + (size_t)b * per);
  VF* __restrict__ ov = reinterpret_cast<VF*>(dz + (size_t)b * per);
  const float k0 = (gscale ? gscale[0] : 1.f) * c;
  const long long nv = per / E;
  const long long st = (long long)gridDim.x * 256;
#pragma unroll 4
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += st) {
    const VF a = zv[i];
    const VI d = dv[i];
    VF o;
    if constexpr (ACC) o = ov[i];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      float p, pq;
      bnd_sigmoid(a.v[k], p, pq);
      const float term = (k0 * bnd_phi(d.v[k])) * pq;
      o.v[k] = ACC ? o.v[k] + term : term;
    }
    ov[i] = o;
  }
}

// Workgroups per sample: the rule of seg_loss_gx (seg_loss.hip) — at most ~1024 workgroups in all and 256 per sample; a function
// of (B, per) alone, so rows(), forward and backward agree on it.
static int boundary_gx(int B, long long per) {
  long long gx = per / (4 * 256 * 4);
  const long long cap = 1024 / B;
  if (gx > cap) gx = cap;
  if (gx > 256) gx = 256;
  return (int)(gx < 1 ? 1 : gx);
}

static bool bnd_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

#define BND_CHECK_SHAPE(who)                                                                                                      \
  MI355_CHECK_ARG(B > 0 && B <= SDIST_MAX_B && per > 0, who ": 0 < B <= %d and per > 0 expected (B=%d, per=%lld)", SDIST_MAX_B,  \
                  B, per)

extern "C" int mi355_boundary_loss_rows(int B, long long per) {
  BND_CHECK_SHAPE("boundary_loss_rows");
  return B * boundary_gx(B, per);
}

extern "C" int mi355_boundary_loss_fwd(const float* z, const int32_t* sd2, int B, long long per, float weight, const float* base,
                                       float* partial, float* loss, mi355_stream_t s) {
  MI355_CHECK_ARG(z, "boundary_loss_fwd: null pointer (z)");
  MI355_CHECK_ARG(sd2, "boundary_loss_fwd: null pointer (sd2)");
  MI355_CHECK_ARG(partial, "boundary_loss_fwd: null pointer (partial)");
  MI355_CHECK_ARG(loss, "boundary_loss_fwd: null pointer (loss)");
  BND_CHECK_SHAPE("boundary_loss_fwd");
  MI355_CHECK_ARG(weight >= 0.f, "boundary_loss_fwd: weight must not be negative (%g)", (double)weight);
  const int gx = boundary_gx(B, per);
  if (per % 4 == 0 && bnd_aligned16(z) && bnd_aligned16(sd2))
    hipLaunchKernelGGL((boundary_fwd_kernel<4>), dim3(gx, B), dim3(256), 0, (hipStream_t)s, z, sd2, per, partial);
  else
    hipLaunchKernelGGL((boundary_fwd_kernel<1>), dim3(gx, B), dim3(256), 0, (hipStream_t)s, z, sd2, per, partial);
  MI355_LAUNCH_CHECK();
  const double scale = (double)weight / ((double)B * (double)per);
  hipLaunchKernelGGL(boundary_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partial, B * gx, scale, base, loss);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_boundary_loss_bwd(const float* z, const int32_t* sd2, int B, long long per, float weight, const float* gscale,
                                       int accumulate, float* dz, mi355_stream_t s) {
  MI355_CHECK_ARG(z, "boundary_loss_bwd: null pointer (z)");
  MI355_CHECK_ARG(sd2, "boundary_loss_bwd: null pointer (sd2)");
  MI355_CHECK_ARG(dz, "boundary_loss_bwd: null pointer (dz)");
  BND_CHECK_SHAPE("boundary_loss_bwd");
  MI355_CHECK_ARG(weight >= 0.f, "boundary_loss_bwd: weight must not be negative (%g)", (double)weight);
  const int gx = boundary_gx(B, per);
  const float c = (float)((double)weight / ((double)B * (double)per));
  const bool vec = per % 4 == 0 && bnd_aligned16(z) && bnd_aligned16(sd2) && bnd_aligned16(dz);
  const dim3 grid(gx, B), block(256);
  hipStream_t st = (hipStream_t)s;
  if (vec && accumulate)
    hipLaunchKernelGGL((boundary_bwd_kernel<4, true>), grid, block, 0, st, z, sd2, per, c, gscale, dz);
  else if (vec)
    hipLaunchKernelGGL((boundary_bwd_kernel<4, false>), grid, block, 0, st, z, sd2, per, c, gscale, dz);
  else if (accumulate)
    hipLaunchKernelGGL((boundary_bwd_kernel<1, true>), grid, block, 0, st, z, sd2, per, c, gscale, dz);
  else
    hipLaunchKernelGGL((boundary_bwd_kernel<1, false>), grid, block, 0, st, z, sd2, per, c, gscale, dz);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
