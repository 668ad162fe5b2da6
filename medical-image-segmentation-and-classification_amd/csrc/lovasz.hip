// Lovasz hinge (Berman, Triki, Blaschko, CVPR 2018, Algorithm 1) on the device: the convex surrogate of the Jaccard index.
//
// Per segment (one image, or the whole batch): y_i = t_i > thr, margin m_i = y_i ? z_i : -z_i (exact in fp32), the margins ranked
// ascending by the stable segmented sort of segsort.hip — the MARGINS are sorted, not the errors 1 - m: the fp32 margin is what an
// fp64 yardstick sorts too, so both see the same ties.  With P the positives of the segment and c_k the positives among ranks
// 0 .. k:  I_k = P - c_k,  U_k = P + (k + 1) - c_k, and the increment of the Jaccard loss at rank k in closed form from the integers
//   positive:            w_k = 1 / U_k
//   negative, U_k > 1:   w_k = I_k / ((U_k - 1) U_k)
//   negative, U_k = 1:   w_k = 1                      (no positives, first rank)
// never as a difference J_k - J_{k-1} of two numbers near 0.5.  L = sum_k max(e_(k), 0) w_k with e = 1 - m, dL/dz_i = (y_i ? -1 : +1)
// w_rank(i) where e_i > 0, else 0.  loss[0] = base + weight / S * sum_s L_s, coef_i = weight / S * dL_s/dz_i.
//
//   lovasz_margin_kernel     m = y ? z : -z                                                  one streaming pass
//   (segsort)                perm = the ranks
//   lovasz_count_kernel      positives per tile of SEGSORT_TILE consecutive RANKS            gathers t through perm
//   (segsort_rowscan_kernel) positives before each tile, P per segment
//   lovasz_weight_kernel     c_k by ballots within the tile, w_k, e, the product and the fold in double; coef scattered to the
//                            pixel (rounded to fp32 once); one partial per tile
//   lovasz_finalize_kernel   one workgroup folds the partials in a fixed order in double, loss rounded to fp32 once
//
// Activity is tested as !(e <= 0): a NaN logit stays active and makes the loss NaN.  No floating-point atomics, nothing allocated,
// nothing synchronises, nothing read back.  The backward is one streaming pass over coef.
#include "segsort.hpp"

#define LOVASZ_KPT (SEGSORT_TILE / 256)

__global__ __launch_bounds__(256) void lovasz_margin_kernel(const float* __restrict__ z, const float* __restrict__ t, long long n,
                                                            float thr, float* __restrict__ m) {
  const long long st = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += st) {
    const float a = z[i];
    m[i] = t[i] > thr ? a : -a;
  }
}

// grid (ntiles, S): tilepos[s][tile] = positives among the ranks of the tile
__global__ __launch_bounds__(256) void lovasz_count_kernel(const float* __restrict__ t, const int* __restrict__ perm, int len,
                                                           int ntiles, float thr, int* __restrict__ tilepos) {
  __shared__ int red[4];
  const int s = blockIdx.y, tile = blockIdx.x;
  const long long seg = (long long)s * len;
  const int t0 = tile * SEGSORT_TILE;
  int c = 0;
#pragma unroll
  for (int j = 0; j < LOVASZ_KPT; ++j) {
    const int k = t0 + j * 256 + threadIdx.x;
    if (k < len) c += t[seg + perm[seg + k]] > thr ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tilepos[(size_t)s * ntiles + tile] = (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ void lovasz_put_double(int* __restrict__ p, double v) {      // ws is int32: no 8-byte alignment assumed
  p[0] = __double2loint(v);
  p[1] = __double2hiint(v);
}
__device__ __forceinline__ double lovasz_get_double(const int* __restrict__ p) { return __hiloint2double(p[1], p[0]); }

// grid (ntiles, S), 256 threads: rank k = t0 + j * 256 + tid, so step j covers 256 consecutive ranks.
__global__ __launch_bounds__(256) void lovasz_weight_kernel(const float* __restrict__ t, const float* __restrict__ m,
                                                            const int* __restrict__ perm, const int* __restrict__ tilebase,
                                                            const int* __restrict__ ptot, int len, int ntiles, float thr, double cs,
                                                            float* __restrict__ coef, int* __restrict__ partial) {
  __shared__ int wt[LOVASZ_KPT][4];             // positives of (step, wave)
  __shared__ double red[4];
  const int s = blockIdx.y, tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long seg = (long long)s * len;
  const int t0 = tile * SEGSORT_TILE;
  const unsigned long long le = (2ull << lane) - 1ull;      // lanes 0 .. lane (2 << 63 wraps to 0: every bit)
  int idx[LOVASZ_KPT], incl[LOVASZ_KPT];
  float mk[LOVASZ_KPT];
  bool y[LOVASZ_KPT];
#pragma unroll
  for (int j = 0; j < LOVASZ_KPT; ++j) {
    const int k = t0 + j * 256 + tid;
    const bool valid = k < len;
    idx[j] = valid ? perm[seg + k] : 0;
    y[j] = valid && t[seg + idx[j]] > thr;
    mk[j] = valid ? m[seg + idx[j]] : 0.f;
    const unsigned long long b = __ballot(y[j]);
    incl[j] = __popcll(b & le);
    if (lane == 0) wt[j][w] = __popcll(b);
  }
  __syncthreads();
  const int P = ptot[s];
  int before = tilebase[(size_t)s * ntiles + tile];      // positives at the ranks before (step j, wave w)
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < LOVASZ_KPT; ++j) {
    int mine = before;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = wt[j][q];
      mine += q < w ? c : 0;
      before += c;
    }
    const int k = t0 + j * 256 + tid;
    if (k < len) {
      const int c = mine + incl[j];
      const int I = P - c;
      const long long U = (long long)P + (k + 1) - c;
      const double wk = y[j] ? 1.0 / (double)U : (U > 1 ? (double)I / (double)((U - 1) * U) : 1.0);
      const double e = 1.0 - (double)mk[j];
      const bool active = !(e <= 0.0);
      acc += active ? e * wk : 0.0;
      coef[seg + idx[j]] = active ? (float)((y[j] ? -wk : wk) * cs) : 0.f;
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) red[w] = acc;
  __syncthreads();
  if (tid == 0) lovasz_put_double(partial + 2 * ((size_t)s * ntiles + tile), (red[0] + red[1]) + (red[2] + red[3]));
}

// One workgroup: thread t folds partials t, t + 256, ..., then lanes, then the four waves in wave order.
__global__ __launch_bounds__(256) void lovasz_finalize_kernel(const int* __restrict__ partial, int rows, double cs,
                                                              const float* __restrict__ base, float* __restrict__ loss) {
  double v = 0;
  for (int i = threadIdx.x; i < rows; i += 256) v += lovasz_get_double(partial + 2 * (size_t)i);
  v = wave_sum_d(v);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((base ? (double)base[0] : 0.0) + cs * ((red[0] + red[1]) + (red[2] + red[3])));
}

// dz (+)= gscale[0] * coef: 16-byte accesses over the first n / 4 vectors when VEC, the remainder (or everything) element-wise.
template <bool VEC, bool ACC>
__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float* __restrict__ coef, long long n, const float* __restrict__ gscale,
                                                         float* __restrict__ dz) {
#pragma clang fp contract(off)      /* accumulate adds the ROUNDED term: two launches give what one launch plus a sum gives */
  const float g = gscale ? gscale[0] : 1.f;
  const long long st = (long long)gridDim.x * 256;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
  long long done = 0;
  if constexpr (VEC) {
    const long long nv = n / 4;
    for (long long i = i0; i < nv; i += st) {
      const Vec16<float> c = ld16_plain<float>(coef + 4 * i);
      Vec16<float> o;
      if constexpr (ACC) o = ld16_plain<float>(dz + 4 * i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float term = g * c.v[k];
        o.v[k] = ACC ? o.v[k] + term : term;
      }
      st16<float>(dz + 4 * i, o);
    }
    done = nv * 4;
  }
  for (long long i = done + i0; i < n; i += st) {
    const float term = g * coef[i];
    dz[i] = ACC ? dz[i] + term : term;
  }
}

// ws = [m : n | perm : n | tilepos : S ntiles | P : S | partial : 2 S ntiles | the sort's workspace]
static long long lovasz_ws_need(int S, long long len) {
  const long long n = (long long)S * len, nt = segsort_ntiles(len);
  return 2 * n + 3 * (long long)S * nt + S + segsort_ws_need(S, len);
}

#define LOVASZ_CHECK_SHAPE(who)                                                                                                   \
  MI355_CHECK_ARG(segsort_shape_ok(S, len), who ": 1 <= S <= %d, len >= 1 and S * len <= 2^26 expected (S=%d, len=%lld)",         \
                  SEGSORT_MAX_S, S, len)

extern "C" int mi355_lovasz_ws_ints(int S, long long len) {
  LOVASZ_CHECK_SHAPE("lovasz_ws_ints");
  return (int)lovasz_ws_need(S, len);
}

extern "C" int mi355_lovasz_fwd(const float* z, const float* t, int S, long long len, float thr, float weight, const float* base,
                                int32_t* ws, long long ws_ints, float* coef, float* loss, mi355_stream_t s) {
  MI355_CHECK_ARG(z, "lovasz_fwd: null pointer (z)");
  MI355_CHECK_ARG(t, "lovasz_fwd: null pointer (t)");
  MI355_CHECK_ARG(ws, "lovasz_fwd: null pointer (ws)");
  MI355_CHECK_ARG(coef, "lovasz_fwd: null pointer (coef)");
  MI355_CHECK_ARG(loss, "lovasz_fwd: null pointer (loss)");
  LOVASZ_CHECK_SHAPE("lovasz_fwd");
  MI355_CHECK_ARG(weight >= 0.f, "lovasz_fwd: weight must not be negative (%g)", (double)weight);
  const long long need = lovasz_ws_need(S, len);
  MI355_CHECK_ARG(ws_ints >= need, "lovasz_fwd: workspace ws of %lld int32 elements is too short, %lld needed (S=%d, len=%lld)",
                  ws_ints, need, S, len);
  hipStream_t st = (hipStream_t)s;
  const long long n = (long long)S * len;
  const int nt = segsort_ntiles(len);
  float* m = reinterpret_cast<float*>(ws);
  int* perm = ws + n;
  int* tilepos = ws + 2 * n;
  int* ptot = tilepos + (size_t)S * nt;
  int* partial = ptot + S;
  int32_t* sort_ws = partial + 2 * (size_t)S * nt;
  long long gm = (n + 4 * 256 - 1) / (4 * 256);
  if (gm > 2048) gm = 2048;
  hipLaunchKernelGGL(lovasz_margin_kernel, dim3((unsigned)gm), dim3(256), 0, st, z, t, n, thr, m);
  MI355_LAUNCH_CHECK();
  int rc = segsort_launch(m, S, len, sort_ws, perm, st);
  if (rc != MI355_OK) return rc;
  const dim3 grid(nt, S), block(256);
  hipLaunchKernelGGL(lovasz_count_kernel, grid, block, 0, st, t, perm, (int)len, nt, thr, tilepos);
  MI355_LAUNCH_CHECK();
  rc = segsort_rowscan_launch(tilepos, ptot, nt, 1, S, st);
  if (rc != MI355_OK) return rc;
  const double cs = (double)weight / (double)S;
  hipLaunchKernelGGL(lovasz_weight_kernel, grid, block, 0, st, t, m, perm, tilepos, ptot, (int)len, nt, thr, cs, coef, partial);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(256), 0, st, partial, S * nt, cs, base, loss);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

static bool lovasz_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

extern "C" int mi355_lovasz_bwd(const float* coef, long long n, const float* gscale, int accumulate, float* dz, mi355_stream_t s) {
  MI355_CHECK_ARG(coef, "lovasz_bwd: null pointer (coef)");
  MI355_CHECK_ARG(dz, "lovasz_bwd: null pointer (dz)");
  MI355_CHECK_ARG(n >= 1 && n <= SEGSORT_MAX_N, "lovasz_bwd: 1 <= n <= 2^26 expected (n=%lld)", n);
  const bool vec = n >= 4 && lovasz_aligned16(coef) && lovasz_aligned16(dz);
  long long gx = (n + 4 * 256 - 1) / (4 * 256);
  if (gx > 2048) gx = 2048;
  const dim3 grid((unsigned)gx), block(256);
  hipStream_t st = (hipStream_t)s;
  if (vec && accumulate) hipLaunchKernelGGL((lovasz_bwd_kernel<true, true>), grid, block, 0, st, coef, n, gscale, dz);
  else if (vec) hipLaunchKernelGGL((lovasz_bwd_kernel<true, false>), grid, block, 0, st, coef, n, gscale, dz);
  else if (accumulate) hipLaunchKernelGGL((lovasz_bwd_kernel<false, true>), grid, block, 0, st, coef, n, gscale, dz);
  else hipLaunchKernelGGL((lovasz_bwd_kernel<false, false>), grid, block, 0, st, coef, n, gscale, dz);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
