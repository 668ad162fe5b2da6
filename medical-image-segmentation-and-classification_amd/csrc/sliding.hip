// Sliding-window inference (utils/sliding.py; nothing in the reference): a batch kept at a higher resolution is cut into overlapping
// T x T tiles on a grid of Py row starts and Px column starts, every tile goes through the segmenter at ONE plan shape, and the
// one-channel logit maps are blended where the tiles overlap.
//   tile_gather_f32 : the listed tiles of a normalised fp32 NCHW batch -> one fp32 [M][C][T][T] batch
//   tile_blend      : the tiles' logit maps -> per pixel the weighted mean over the covering tiles (separable window wy[ty] * wx[tx]),
//                     the spread (max - min) of the covering values, how many tiles cover the pixel, and the thresholded mask
// Every floating-point operation is rounded on its own (no FMA contraction), nothing is atomic and every sum runs in a fixed
// order (iy ascending, within iy ix ascending): the outputs are bit-identical run to run and equal tests/sliding_ref.py's float32
// restatement.  The blend is a gather per OUTPUT pixel: nothing is accumulated in memory.
// Both kernels stream.  The tile starts travel in the kernel arguments (validated on the host) and are only ever indexed by
// wave-uniform values, so they are scalar loads from the argument segment.  A lane owns 4 consecutive x (16-byte loads and
// stores) when T, W and every column start are multiples of 4 and the pointers are 16-byte aligned: a group of 4 then lies wholly
// inside or outside every tile.  Otherwise a lane owns one x.
#include "common.hpp"
#include "decide.hpp"

#define SW_MAX_STARTS 64

struct SwGrid {
  int32_t ys[SW_MAX_STARTS];
  int32_t xs[SW_MAX_STARTS];
  int Py, Px;
};

template <int V> struct SwVec;
template <> struct SwVec<1> {
  typedef float F;
  typedef uint8_t B;
};
template <> struct SwVec<4> {
  typedef f32x4 F;
  typedef __attribute__((ext_vector_type(4))) uint8_t B;
};

// ---- gather ------------------------------------------------------------------------------------------------------------------
// blockIdx.x = the entry i of the tile list (its tile, hence iy and ix, is uniform over the block); blockIdx.y strides over the
// C * T * (T / V) groups of the tile.  An entry outside [0, N Py Px) is skipped.
template <int V>
__global__ void tile_gather_kernel(const float* __restrict__ src, int N, int C, int H, int W, int T, const SwGrid g,
                                   const int32_t* __restrict__ tiles, float* __restrict__ dst) {
#pragma clang fp contract(off)
  typedef typename SwVec<V>::F F;
  const int i = blockIdx.x;
  const int t = tiles[i];
  if (t < 0 || t >= N * g.Py * g.Px) return;
  const int ix = t % g.Px, iy = (t / g.Px) % g.Py, n = t / (g.Px * g.Py);
  const int y0 = g.ys[iy], x0 = g.xs[ix];
  const int TV = T / V;
  const long long groups = (long long)C * T * TV;
  const size_t plane = (size_t)H * W;
  const float* s = src + (size_t)n * C * plane + (size_t)y0 * W + x0;
  float* d = dst + (size_t)i * C * T * T;
  for (long long q = (long long)blockIdx.y * blockDim.x + threadIdx.x; q < groups; q += (long long)gridDim.y * blockDim.x) {
    const int tx = (int)(q % TV) * V;
    const long long r = q / TV;
    const int ty = (int)(r % T), c = (int)(r / T);
    *(F*)(d + ((size_t)c * T + ty) * T + tx) = *(const F*)(s + (size_t)c * plane + (size_t)ty * W + tx);
  }
}

// ys / xs: strictly ascending, first 0, last extent - T, every gap <= T (no pixel uncovered)
static const char* sw_check_starts(const int32_t* st, int P, int extent, int T) {
  if (st[0] != 0) return "the first start must be 0";
  if (st[P - 1] != extent - T) return "the last start must be extent - T";
  for (int i = 1; i < P; ++i) {
    if (st[i] <= st[i - 1]) return "starts must be strictly ascending";
    if (st[i] - st[i - 1] > T) return "a gap between starts exceeds T (uncovered pixels)";
  }
  return nullptr;
}

// the most starts that fall into any half-open range of T pixels: how many tiles cover one pixel along this axis at the most
static int sw_depth(const int32_t* st, int P, int T) {
  int best = 1;
  for (int i = 0, j = 0; i < P; ++i) {
    while (st[i] - st[j] >= T) ++j;
    if (i - j + 1 > best) best = i - j + 1;
  }
  return best;
}

// fills g; returns nonzero with the error set
static int sw_grid(const char* who, int N, int H, int W, int T, const int32_t* ys, int Py, const int32_t* xs, int Px, SwGrid& g) {
  MI355_CHECK_ARG(ys && xs, "%s: null tile starts", who);
  MI355_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: bad sizes (N=%d H=%d W=%d)", who, N, H, W);
  MI355_CHECK_ARG(T >= 1 && T <= H && T <= W, "%s: 1 <= T <= min(H, W) required (T=%d H=%d W=%d)", who, T, H, W);
  MI355_CHECK_ARG(Py >= 1 && Py <= SW_MAX_STARTS && Px >= 1 && Px <= SW_MAX_STARTS, "%s: 1 <= Py, Px <= %d required (Py=%d Px=%d)", who,
                  SW_MAX_STARTS, Py, Px);
  MI355_CHECK_ARG((long long)N * Py * Px <= 0x7fffffffLL, "%s: too many tiles", who);
  const char* why = sw_check_starts(ys, Py, H, T);
  MI355_CHECK_ARG(!why, "%s: ys: %s", who, why);
  why = sw_check_starts(xs, Px, W, T);
  MI355_CHECK_ARG(!why, "%s: xs: %s", who, why);
  const int deep = sw_depth(ys, Py, T) * sw_depth(xs, Px, T);                        // cover is a uint8 plane
  MI355_CHECK_ARG(deep <= 255, "%s: up to %d tiles cover one pixel, at most 255 are supported", who, deep);
  memset(&g, 0, sizeof(g));
  memcpy(g.ys, ys, sizeof(int32_t) * Py);
  memcpy(g.xs, xs, sizeof(int32_t) * Px);
  g.Py = Py;
  g.Px = Px;
  return MI355_OK;
}

static bool sw_vec4(const SwGrid& g, int W, int T) {
  if (T % 4 || W % 4) return false;
  for (int i = 0; i < g.Px; ++i)
    if (g.xs[i] % 4) return false;
  return true;
}

static bool sw_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" int mi355_tile_gather_f32(const float* src, int N, int C, int H, int W, int T, const int32_t* ys, int Py, const int32_t* xs, int Px,
                                     const int32_t* tiles, int M, float* dst, mi355_stream_t s) {
  MI355_CHECK_ARG(src && tiles && dst && src != dst, "tile_gather_f32: null pointer or src == dst");
  MI355_CHECK_ARG(C >= 1 && M >= 1, "tile_gather_f32: bad sizes (C=%d M=%d)", C, M);
  SwGrid g;
  if (int rc = sw_grid("tile_gather_f32", N, H, W, T, ys, Py, xs, Px, g)) return rc;
  const bool vec = sw_vec4(g, W, T) && sw_aligned(src, 16) && sw_aligned(dst, 16);
  const long long groups = (long long)C * T * (T / (vec ? 4 : 1));
  long long by = (groups + 255) / 256;
  if (by > 1024) by = 1024;
  if (vec)
    hipLaunchKernelGGL(tile_gather_kernel<4>, dim3(M, (int)by), dim3(256), 0, (hipStream_t)s, src, N, C, H, W, T, g, tiles, dst);
  else
    hipLaunchKernelGGL(tile_gather_kernel<1>, dim3(M, (int)by), dim3(256), 0, (hipStream_t)s, src, N, C, H, W, T, g, tiles, dst);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- blend -------------------------------------------------------------------------------------------------------------------
// One workgroup: the segment [bx0, bx0 + blockDim.x * V) of row y = blockIdx.y of sample n = blockIdx.z.  The covering iy are
// found from y (uniform), the ix that touch the segment from bx0 (uniform); a lane then only tests its own x against the tile.
template <int V>
__global__ void tile_blend_kernel(const float* __restrict__ z, int H, int W, int T, const SwGrid g, const float* __restrict__ wy,
                                  const float* __restrict__ wx, int prob, float thr, const int32_t* __restrict__ idx,
                                  float* __restrict__ mean, float* __restrict__ spread, uint8_t* __restrict__ cover,
                                  uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
  typedef typename SwVec<V>::F F;
  typedef typename SwVec<V>::B B;
  const int y = blockIdx.y, n = blockIdx.z;
  const int bx0 = blockIdx.x * blockDim.x * V, bx1 = min(bx0 + (int)blockDim.x * V, W);
  const int x = bx0 + threadIdx.x * V;
  const bool live = x < W;                                // V = 4: W % 4 == 0, the whole group is live or not
  const size_t tile = (size_t)T * T;
  float num[V], den[V], lo[V], hi[V];
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    num[j] = 0.f;
    den[j] = 0.f;
    lo[j] = INFINITY;
    hi[j] = -INFINITY;
  }
  for (int iy = 0; iy < g.Py; ++iy) {
    const int ty = y - g.ys[iy];
    if (ty < 0 || ty >= T) continue;
    const float wr = wy[ty];
    for (int ix = 0; ix < g.Px; ++ix) {
      const int x0 = g.xs[ix];
      if (x0 >= bx1 || x0 + T <= bx0) continue;           // the tile misses the whole segment
      const int tx = x - x0;
      if (!live || tx < 0 || tx >= T) continue;
      const size_t p = ((size_t)n * g.Py + iy) * g.Px + ix;
      const F vv = *(const F*)(z + p * tile + (size_t)ty * T + tx);
      const F ww = *(const F*)(wx + tx);
      ++cnt;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float v, wc;
        if constexpr (V == 1) {
          v = vv;
          wc = ww;
        } else {
          v = vv[j];
          wc = ww[j];
        }
        if (prob) v = sigmoid_f32(v);
        const float w = wr * wc;
        num[j] = num[j] + (w * v);
        den[j] = den[j] + w;
        lo[j] = fminf(lo[j], v);
        hi[j] = fmaxf(hi[j], v);
      }
    }
  }
  if (!live) return;
  const size_t q = (size_t)y * W + x, plane = (size_t)H * W;
  F mu, sp;
  B cv, mk;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float m = num[j] / den[j];
    const float d = hi[j] - lo[j];
    const uint8_t b = (prob ? m : sigmoid_f32(m)) > thr ? 255 : 0;
    if constexpr (V == 1) {
      mu = m;
      sp = d;
      cv = (uint8_t)cnt;
      mk = b;
    } else {
      mu[j] = m;
      sp[j] = d;
      cv[j] = (uint8_t)cnt;
      mk[j] = b;
    }
  }
  *(F*)(mean + (size_t)n * plane + q) = mu;
  if (spread) *(F*)(spread + (size_t)n * plane + q) = sp;
  if (cover && n == 0) *(B*)(cover + q) = cv;
  if (mask) *(B*)(mask + (size_t)(idx ? idx[n] : n) * plane + q) = mk;
}

extern "C" int mi355_tile_blend(const float* z, int N, int H, int W, int T, const int32_t* ys, int Py, const int32_t* xs, int Px,
                                const float* wy, const float* wx, int prob, float thr, const int32_t* idx, float* mean, float* spread,
                                uint8_t* cover, uint8_t* mask, mi355_stream_t s) {
  MI355_CHECK_ARG(z && wy && wx && mean, "tile_blend: null pointer");
  SwGrid g;
  if (int rc = sw_grid("tile_blend", N, H, W, T, ys, Py, xs, Px, g)) return rc;
  const bool vec = sw_vec4(g, W, T) && sw_aligned(z, 16) && sw_aligned(wx, 16) && sw_aligned(mean, 16) && (!spread || sw_aligned(spread, 16)) &&
                   (!cover || sw_aligned(cover, 4)) && (!mask || sw_aligned(mask, 4));
  const int per = vec ? 4 : 1;
  const int lanes = (W + per - 1) / per;
  int threads = (lanes + 63) / 64 * 64;
  if (threads > 256) threads = 256;
  const dim3 grid((lanes + threads - 1) / threads, H, N);
  if (vec)
    hipLaunchKernelGGL(tile_blend_kernel<4>, grid, dim3(threads), 0, (hipStream_t)s, z, H, W, T, g, wy, wx, prob, thr, idx, mean, spread, cover,
                       mask);
  else
    hipLaunchKernelGGL(tile_blend_kernel<1>, grid, dim3(threads), 0, (hipStream_t)s, z, H, W, T, g, wy, wx, prob, thr, idx, mean, spread, cover,
                       mask);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
