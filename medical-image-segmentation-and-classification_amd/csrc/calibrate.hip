// Post-hoc calibration on the device: the temperature of a classifier (Guo et al. 2017) fitted on held-out logits, and the sweep of
// a segmenter's mask threshold over a list of candidates that picks the one with the best mean Dice.
//
// Temperature.  With beta = 1 / T the mean negative log-likelihood g(beta) = mean_i(log sum_j exp(beta x_ij - m_i) + m_i - beta x_iy) is
// convex, g' = mean_i(E_p[x_i] - x_iy), g'' = mean_i Var_p[x_i], p = softmax(beta x_i).  Every row is evaluated in double relative to its
// largest logit, d_j = x_j - max x (exact in double): e_j = exp(beta d_j) <= 1, S0 = sum e_j, S1 = sum e_j d_j, S2 = sum e_j d_j^2 and
//   NLL_i = log S0 - beta d_y,   g'_i = S1 / S0 - d_y,   g''_i = max(0, S2 / S0 - (S1 / S0)^2)
//   temp_init_kernel    beta = 1, the bracket [2^-6, 2^6], status "running"
//   temp_rows_kernel    one evaluation: a row per thread (C <= 32) or per wave (beyond), one partial (NLL, g', g'') per workgroup
//   temp_update_kernel  one workgroup folds the partials in a fixed order and one thread moves beta
//   temp_eval_kernel    the fold alone: the three figures of one evaluation at a given beta (mi355_temperature_eval)
// The host enqueues TEMP_MAX_EVALS (rows, update) pairs and never reads beta; once the status is set both kernels return at once.
// Evaluation 1 is at beta = 1 (flat: g'' = 0 -> status 3).  Evaluation 2 is at the end of the bracket that g'(1) points to: no sign
// change there is the clamp (status 1 / 2: an underflowed g' = 0 at 2^6 is separable data all the same).  From then on the bracket
// holds a sign change of g' and shrinks by the sign of g' at every evaluation; the next beta is Newton's, or the bracket's geometric
// mean when g'' <= 0 or the step leaves the bracket.  The iteration stops at the evaluated beta once the step |dbeta| <= 2^-40 beta:
// state[3..5] are the figures AT state[0].
//
// Sweep.  A pixel's bin is #{k : v > thr[k]} over the ascending candidates (a NaN: 0), found by bisection of the list in LDS.
//   sweep_hist_kernel     grid (chunks, B): positives and negatives per bin of SWEEP_CHUNK pixels, integer LDS atomics; bins 0 and K —
//                         where a trained segmenter puts nearly every pixel — are counted in registers instead
//   sweep_suffix_kernel   grid (B): adds an image's chunks bin by bin and suffix-sums them: tp[k] = positives in the bins above k
//   sweep_fold_kernel     thread = candidate: the images' Dice and IoU in double, added to the running sums in image order
//   sweep_pick_kernel     one workgroup: the lowest index of the largest mean Dice
//
// No floating-point atomics, nothing allocated, nothing synchronises, nothing read back: the same input gives the same bytes.
#include "common.hpp"

__device__ __forceinline__ void cal_put_double(int* __restrict__ p, double v) {         // ws is int32: no 8-byte alignment assumed
  p[0] = __double2loint(v);
  p[1] = __double2hiint(v);
}
__device__ __forceinline__ double cal_get_double(const int* __restrict__ p) { return __hiloint2double(p[1], p[0]); }

// ---- temperature -------------------------------------------------------------------------------------------------------------------
#define TEMP_MAX_C 4096
#define TEMP_MAX_N (1ll << 26)
#define TEMP_MAX_EVALS 64
#define TEMP_LANE_C 32                          /* up to here a thread owns a row, beyond a wave does */
#define TEMP_WAVE_ROWS 16                       /* rows of a workgroup of the wave-per-row kernel */
#define TEMP_HDR 8                              /* ws = [lo, hi, cand : double | phase, pad | partials : 3 doubles per workgroup] */
#define TEMP_BETA_LO 0.015625
#define TEMP_BETA_HI 64.0
#define TEMP_STEP_TOL 9.094947017729282e-13     /* 2^-40 */

static inline int temp_rows_per_block(int C) { return C <= TEMP_LANE_C ? 256 : TEMP_WAVE_ROWS; }

__global__ void temp_init_kernel(double* __restrict__ state, int* __restrict__ ws) {
  if (threadIdx.x != 0) return;
  state[0] = 1.0;
  state[1] = 1.0;
  for (int i = 2; i < 7; ++i) state[i] = 0.0;
  state[7] = -1.0;
  cal_put_double(ws + 0, TEMP_BETA_LO);
  cal_put_double(ws + 2, TEMP_BETA_HI);
  cal_put_double(ws + 4, 1.0);
  ws[6] = 0;
  ws[7] = 0;
}

// the row's three figures from lanes sub, sub + LPR, ... of it; every lane of the row returns the same values
template <int LPR>
__device__ __forceinline__ void temp_row(const float* __restrict__ row, int C, int y, double beta, int sub, double& nll, double& g1,
                                         double& g2) {
  float mxf = -INFINITY;
  for (int c = sub; c < C; c += LPR) mxf = fmaxf(mxf, row[c]);
#pragma unroll
  for (int o = LPR >> 1; o > 0; o >>= 1) mxf = fmaxf(mxf, __shfl_xor(mxf, o, 64));
  const double mx = (double)mxf;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int c = sub; c < C; c += LPR) {
    const double d = (double)row[c] - mx;
    const double e = exp(beta * d);
    s0 += e;
    s1 += e * d;
    s2 += e * d * d;
  }
#pragma unroll
  for (int o = LPR >> 1; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64);
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  // a label outside 0 .. C - 1 lives on the device and cannot be refused by the launcher: it reads nothing and poisons the fit
  const double dy = (y >= 0 && y < C) ? (double)row[y] - mx : __longlong_as_double(0x7ff8000000000000ll);
  const double mean = s1 / s0;
  nll = log(s0) - beta * dy;
  g1 = mean - dy;
  g2 = fmax(0.0, s2 / s0 - mean * mean);
}

// grid (ceil(N / rows per workgroup)), 256 threads; `status` NULL (a single evaluation) or the fit's: set = return.  LPR = 1: thread = row, folded over lanes then waves.  LPR = 64: wave w owns rows
// 4 w .. 4 w + 3 of the workgroup's 16, added in row order.  part[block] = (sum NLL, sum g', sum g'').
template <int LPR>
__global__ __launch_bounds__(256) void temp_rows_kernel(const float* __restrict__ x, const int* __restrict__ labels, int N, int C,
                                                        const double* __restrict__ beta_dev, const double* __restrict__ status,
                                                        int* __restrict__ part) {
  __shared__ double red[3][4];
  if (status && status[0] >= 0.0) return;
  const double beta = beta_dev[0];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double nll = 0.0, g1 = 0.0, g2 = 0.0;
  if constexpr (LPR == 1) {
    const long long i = (long long)blockIdx.x * 256 + tid;
    if (i < N) temp_row<1>(x + i * C, C, labels[i], beta, 0, nll, g1, g2);
    nll = wave_sum_d(nll);
    g1 = wave_sum_d(g1);
    g2 = wave_sum_d(g2);
  } else {
    for (int r = 0; r < TEMP_WAVE_ROWS / 4; ++r) {
      const long long i = (long long)blockIdx.x * TEMP_WAVE_ROWS + w * (TEMP_WAVE_ROWS / 4) + r;
      if (i < N) {                              // wave-uniform
        double a, b, c;
        temp_row<64>(x + i * C, C, labels[i], beta, lane, a, b, c);
        nll += a;
        g1 += b;
        g2 += c;
      }
    }
  }
  if (lane == 0) {
    red[0][w] = nll;
    red[1][w] = g1;
    red[2][w] = g2;
  }
  __syncthreads();
  if (tid < 3) cal_put_double(part + 6 * (size_t)blockIdx.x + 2 * tid, (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]));
}

// the means over the N rows, valid in thread 0: thread t folds partials t, t + 256, ..., then lanes, then the four waves
__device__ __forceinline__ void temp_fold(const int* __restrict__ part, int nblocks, int N, double (*red)[4], double& nll, double& g1,
                                          double& g2) {
  const int tid = threadIdx.x;
  nll = 0.0;
  g1 = 0.0;
  g2 = 0.0;
  for (int b = tid; b < nblocks; b += 256) {
    const int* p = part + 6 * (size_t)b;
    nll += cal_get_double(p);
    g1 += cal_get_double(p + 2);
    g2 += cal_get_double(p + 4);
  }
  nll = wave_sum_d(nll);
  g1 = wave_sum_d(g1);
  g2 = wave_sum_d(g2);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = nll;
    red[1][tid >> 6] = g1;
    red[2][tid >> 6] = g2;
  }
  __syncthreads();
  nll = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (double)N;
  g1 = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (double)N;
  g2 = ((red[2][0] + red[2][1]) + (red[2][2] + red[2][3])) / (double)N;
}

// one workgroup: out = the mean NLL, g', g'' of one evaluation
__global__ __launch_bounds__(256) void temp_eval_kernel(const int* __restrict__ part, int nblocks, int N, double* __restrict__ out) {
  __shared__ double red[3][4];
  double nll, g1, g2;
  temp_fold(part, nblocks, N, red, nll, g1, g2);
  if (threadIdx.x != 0) return;
  out[0] = nll;
  out[1] = g1;
  out[2] = g2;
}

// one workgroup folds the evaluation; thread 0 moves beta
__global__ __launch_bounds__(256) void temp_update_kernel(const int* __restrict__ part, int nblocks, int N, double* __restrict__ state,
                                                          int* __restrict__ hdr) {
  __shared__ double red[3][4];
  if (state[7] >= 0.0) return;
  double nll, g1, g2;
  temp_fold(part, nblocks, N, red, nll, g1, g2);
  if (threadIdx.x != 0) return;
  const double beta = state[0];
  const int evals = (int)state[6] + 1;
  double lo = cal_get_double(hdr + 0), hi = cal_get_double(hdr + 2), cand = cal_get_double(hdr + 4);
  int phase = hdr[6];
  state[3] = nll;
  state[4] = g1;
  state[5] = g2;
  state[6] = (double)evals;
  if (evals == 1) state[2] = nll;
  int status = -1;
  double next = beta;
  if (!(g1 == g1) || !(g2 == g2)) {             // NaN logits or a label out of range: nothing to iterate on
    status = 4;
  } else if (phase == 0) {                      // at beta = 1
    if (!(g2 > 0.0)) {
      status = 3;
    } else if (g1 == 0.0) {
      status = 0;
    } else {
      cand = beta - g1 / g2;
      if (g1 < 0.0) {
        lo = beta;
        next = hi;
      } else {
        hi = beta;
        next = lo;
      }
      phase = 1;
    }
  } else if (phase == 1) {                      // at the end of the bracket
    if (beta > 1.0 && g1 <= 0.0) {
      status = 2;
    } else if (beta < 1.0 && g1 >= 0.0) {
      status = 1;
    } else {
      next = (cand > lo && cand < hi) ? cand : sqrt(lo * hi);
      phase = 2;
    }
  } else if (g1 == 0.0) {
    status = 0;
  } else {
    if (g1 > 0.0) hi = beta;
    else lo = beta;
    next = beta - g1 / g2;                      // a step below the tolerance ends the iteration, even one that rounds onto the bracket's end
    if (!(g2 > 0.0) || (fabs(next - beta) > TEMP_STEP_TOL * beta && !(next > lo && next < hi))) next = sqrt(lo * hi);
    if (fabs(next - beta) <= TEMP_STEP_TOL * beta) {
      status = 0;
      next = beta;
    }
  }
  if (status < 0 && evals >= TEMP_MAX_EVALS) status = 4;
  if (status < 0) {
    state[0] = next;
    state[1] = 1.0 / next;
    cal_put_double(hdr + 0, lo);
    cal_put_double(hdr + 2, hi);
    cal_put_double(hdr + 4, cand);
    hdr[6] = phase;
  } else {
    state[7] = (double)status;
  }
}

#define TEMP_CHECK_SHAPE(who)                                                                                                     \
  MI355_CHECK_ARG(N >= 1 && C >= 2 && C <= TEMP_MAX_C && (long long)N * C <= TEMP_MAX_N,                                          \
                  who ": N >= 1, 2 <= C <= %d and N * C <= 2^26 expected (N=%d, C=%d)", TEMP_MAX_C, N, C)

extern "C" int mi355_temperature_fit_ws_ints(int N, int C) {
  TEMP_CHECK_SHAPE("temperature_fit_ws_ints");
  return TEMP_HDR + 6 * ceil_div(N, temp_rows_per_block(C));
}

extern "C" int mi355_temperature_fit(const float* x, int N, int C, const int32_t* labels, int32_t* ws, long long ws_ints, double* state,
                                     mi355_stream_t s) {
  MI355_CHECK_ARG(x, "temperature_fit: null pointer (x)");
  MI355_CHECK_ARG(labels, "temperature_fit: null pointer (labels)");
  MI355_CHECK_ARG(ws, "temperature_fit: null pointer (ws)");
  MI355_CHECK_ARG(state, "temperature_fit: null pointer (state)");
  TEMP_CHECK_SHAPE("temperature_fit");
  const int nb = ceil_div(N, temp_rows_per_block(C));
  const long long need = TEMP_HDR + 6ll * nb;
  MI355_CHECK_ARG(ws_ints >= need, "temperature_fit: workspace ws of %lld int32 elements is too short, %lld needed (N=%d, C=%d)",
                  ws_ints, need, N, C);
  hipStream_t st = (hipStream_t)s;
  int* part = ws + TEMP_HDR;
  hipLaunchKernelGGL(temp_init_kernel, dim3(1), dim3(64), 0, st, state, ws);
  MI355_LAUNCH_CHECK();
  for (int it = 0; it < TEMP_MAX_EVALS; ++it) {
    if (C <= TEMP_LANE_C)
      hipLaunchKernelGGL((temp_rows_kernel<1>), dim3(nb), dim3(256), 0, st, x, labels, N, C, state, state + 7, part);
    else
      hipLaunchKernelGGL((temp_rows_kernel<64>), dim3(nb), dim3(256), 0, st, x, labels, N, C, state, state + 7, part);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(temp_update_kernel, dim3(1), dim3(256), 0, st, part, nb, N, state, ws);
    MI355_LAUNCH_CHECK();
  }
  return MI355_OK;
}

extern "C" int mi355_temperature_eval(const float* x, int N, int C, const int32_t* labels, const double* beta_dev, int32_t* ws,
                                      long long ws_ints, double* out, mi355_stream_t s) {
  MI355_CHECK_ARG(x, "temperature_eval: null pointer (x)");
  MI355_CHECK_ARG(labels, "temperature_eval: null pointer (labels)");
  MI355_CHECK_ARG(beta_dev, "temperature_eval: null pointer (beta_dev)");
  MI355_CHECK_ARG(ws, "temperature_eval: null pointer (ws)");
  MI355_CHECK_ARG(out, "temperature_eval: null pointer (out)");
  TEMP_CHECK_SHAPE("temperature_eval");
  const int nb = ceil_div(N, temp_rows_per_block(C));
  const long long need = TEMP_HDR + 6ll * nb;
  MI355_CHECK_ARG(ws_ints >= need, "temperature_eval: workspace ws of %lld int32 elements is too short, %lld needed (N=%d, C=%d)",
                  ws_ints, need, N, C);
  hipStream_t st = (hipStream_t)s;
  int* part = ws + TEMP_HDR;
  const double* running = nullptr;
  if (C <= TEMP_LANE_C)
    hipLaunchKernelGGL((temp_rows_kernel<1>), dim3(nb), dim3(256), 0, st, x, labels, N, C, beta_dev, running, part);
  else
    hipLaunchKernelGGL((temp_rows_kernel<64>), dim3(nb), dim3(256), 0, st, x, labels, N, C, beta_dev, running, part);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(temp_eval_kernel, dim3(1), dim3(256), 0, st, part, nb, N, out);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// y = fl32(double(x) * beta): 16-byte accesses over the aligned body, the remainder element-wise
__global__ __launch_bounds__(256) void logits_scale_kernel(const float* __restrict__ x, long long n, long long n4, int vec,
                                                           const double* __restrict__ beta_dev, float* __restrict__ y) {
  const double beta = beta_dev[0];
  const long long stride = (long long)gridDim.x * 256;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (vec) {
    for (long long i = t; i < n4; i += stride) {
      Vec16<float> v = ld16_plain<float>(x + 4 * i);
#pragma unroll
      for (int k = 0; k < 4; ++k) v.v[k] = (float)((double)v.v[k] * beta);
      st16<float>(y + 4 * i, v);
    }
  }
  for (long long i = (vec ? 4 * n4 : 0) + t; i < n; i += stride) y[i] = (float)((double)x[i] * beta);
}

extern "C" int mi355_logits_scale(const float* x, int N, int C, const double* beta_dev, float* y, mi355_stream_t s) {
  MI355_CHECK_ARG(x, "logits_scale: null pointer (x)");
  MI355_CHECK_ARG(beta_dev, "logits_scale: null pointer (beta_dev)");
  MI355_CHECK_ARG(y, "logits_scale: null pointer (y)");
  MI355_CHECK_ARG(N >= 1 && C >= 1 && (long long)N * C <= TEMP_MAX_N, "logits_scale: N >= 1, C >= 1 and N * C <= 2^26 expected (N=%d, C=%d)",
                  N, C);
  const long long n = (long long)N * C, n4 = n / 4;
  const int vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0 ? 1 : 0;
  const long long work = vec && n4 > 0 ? n4 : n;
  long long blocks = (work + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(logits_scale_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)s, x, n, n4, vec, beta_dev, y);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- threshold sweep ---------------------------------------------------------------------------------------------------------------
#define SWEEP_MAX_K 1024
#define SWEEP_MAX_LEN (1ll << 24)
#define SWEEP_MAX_B 65535
#define SWEEP_CHUNK 16384                       /* pixels per workgroup: 64 per thread */

static inline int sweep_chunks(long long len) { return (int)((len + SWEEP_CHUNK - 1) / SWEEP_CHUNK); }

// grid (chunks, B), 256 threads.  part[b][chunk][0][j] = positives in bin j, part[b][chunk][1][j] = negatives, j = 0 .. K.
__global__ __launch_bounds__(256) void sweep_hist_kernel(const float* __restrict__ scores, const float* __restrict__ target, long long len,
                                                         const float* __restrict__ thr, int K, int is_logit, float tthr,
                                                         int* __restrict__ part) {
  __shared__ float sthr[SWEEP_MAX_K];
  __shared__ int hist[2][SWEEP_MAX_K + 1];
  const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
  for (int k = tid; k < K; k += 256) sthr[k] = thr[k];
  for (int j = tid; j <= K; j += 256) {
    hist[0][j] = 0;
    hist[1][j] = 0;
  }
  __syncthreads();
  const float* __restrict__ sc = scores + (size_t)b * len;
  const float* __restrict__ tg = target + (size_t)b * len;
  const long long i0 = (long long)chunk * SWEEP_CHUNK;
  const long long i1 = i0 + SWEEP_CHUNK < len ? i0 + SWEEP_CHUNK : len;
  int lo_pos = 0, lo_neg = 0, hi_pos = 0, hi_neg = 0;       // bins 0 and K
#pragma unroll 4
  for (long long i = i0 + tid; i < i1; i += 256) {
    float v = sc[i];
    if (is_logit) v = 1.f / (1.f + __expf(-v));
    const int y = tg[i] > tthr ? 0 : 1;
    int a = 0, n = K;                           // v > sthr[k] for k < bin and for no k >= bin (never for a NaN): a = bin at the end
    while (n > 0) {
      const int h = n >> 1;
      if (v > sthr[a + h]) {
        a += h + 1;
        n -= h + 1;
      } else {
        n = h;
      }
    }
    if (a == 0) {
      lo_pos += 1 - y;
      lo_neg += y;
    } else if (a == K) {
      hi_pos += 1 - y;
      hi_neg += y;
    } else {
      atomicAdd(&hist[y][a], 1);
    }
  }
  if (lo_pos) atomicAdd(&hist[0][0], lo_pos);
  if (lo_neg) atomicAdd(&hist[1][0], lo_neg);
  if (hi_pos) atomicAdd(&hist[0][K], hi_pos);
  if (hi_neg) atomicAdd(&hist[1][K], hi_neg);
  __syncthreads();
  int* __restrict__ mine = part + ((size_t)b * gridDim.x + chunk) * 2 * (size_t)(K + 1);
  for (int j = tid; j <= K; j += 256) {
    mine[j] = hist[0][j];
    mine[K + 1 + j] = hist[1][j];
  }
}

// inclusive suffix sum over the 256 threads (thread t: the values of threads t .. 255); red = 4 ints of LDS
__device__ __forceinline__ int sweep_block_suffix(int v, int* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_down(v, o, 64);
    if (lane + o < 64) v += u;
  }
  if (lane == 0) red[w] = v;
  __syncthreads();
  int above = 0;
#pragma unroll
  for (int q = 1; q < 4; ++q) above += q > w ? red[q] : 0;
  __syncthreads();
  return v + above;
}

// grid (B), 256 threads: thread t owns bins 4 t .. 4 t + 3, bin 1024 (K = 1024 only) is added to every suffix
__global__ __launch_bounds__(256) void sweep_suffix_kernel(const int* __restrict__ part, int nchunks, int K, int* __restrict__ tp,
                                                           int* __restrict__ fp, int* __restrict__ pos) {
  __shared__ int hist[2][SWEEP_MAX_K + 4];
  __shared__ int red[4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int* __restrict__ mine = part + (size_t)b * nchunks * 2 * (size_t)(K + 1);
  for (int j = tid; j < SWEEP_MAX_K + 4; j += 256) {
    int p = 0, n = 0;
    if (j <= K) {
      for (int c = 0; c < nchunks; ++c) {
        const int* q = mine + (size_t)c * 2 * (size_t)(K + 1);
        p += q[j];
        n += q[K + 1 + j];
      }
    }
    hist[0][j] = p;
    hist[1][j] = n;
  }
  __syncthreads();
#pragma unroll
  for (int y = 0; y < 2; ++y) {
    int own[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      own[q] = hist[y][4 * tid + q];
      sum += own[q];
    }
    // the bins above 4 t + 3, bin 1024 included
    int run = sweep_block_suffix(sum, red) - sum + hist[y][SWEEP_MAX_K];
    if (y == 0 && tid == 0) pos[b] = run + sum;
    int* __restrict__ out = (y == 0 ? tp : fp) + (size_t)b * K;
#pragma unroll
    for (int q = 3; q >= 0; --q) {              // out[k] = the bins above k
      const int k = 4 * tid + q;
      if (k < K) out[k] = run;
      run += own[q];
    }
  }
}

// grid (ceil(K / 256)), 256 threads: thread = candidate, images in order
__global__ __launch_bounds__(256) void sweep_fold_kernel(const int* __restrict__ tp, const int* __restrict__ fp,
                                                         const int* __restrict__ pos, int B, int K, double* __restrict__ acc,
                                                         long long* __restrict__ n_images) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) n_images[0] += B;
  if (k >= K) return;
  double dice = acc[k], iou = acc[K + k];
  for (int b = 0; b < B; ++b) {
    const double t = (double)tp[(size_t)b * K + k], pp = t + (double)fp[(size_t)b * K + k], tt = (double)pos[b];
    dice += (2.0 * t + 1e-7) / ((pp + tt) + 1e-7);
    iou += (t + 1e-7) / (((pp + tt) - t) + 1e-7);
  }
  acc[k] = dice;
  acc[K + k] = iou;
}

// one workgroup: the largest mean Dice and the lowest index that has it (a NaN mean is never the larger)
__global__ __launch_bounds__(256) void sweep_pick_kernel(const double* __restrict__ acc, const long long* __restrict__ n_images, int K,
                                                         int k_ref, double* __restrict__ out_d, int* __restrict__ out_k) {
  __shared__ double rv[4];
  __shared__ int rk[4];
  const int tid = threadIdx.x;
  const double n = (double)n_images[0];
  double best = -1.0;
  int at = SWEEP_MAX_K;
  for (int k = tid; k < K; k += 256) {          // ascending k: a strict compare keeps the lowest
    const double m = acc[k] / n;
    if (m > best) {
      best = m;
      at = k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int ok = __shfl_xor(at, o, 64);
    if (ov > best || (ov == best && ok < at)) {
      best = ov;
      at = ok;
    }
  }
  if ((tid & 63) == 0) {
    rv[tid >> 6] = best;
    rk[tid >> 6] = at;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int q = 1; q < 4; ++q) {
    if (rv[q] > best || (rv[q] == best && rk[q] < at)) {
      best = rv[q];
      at = rk[q];
    }
  }
  if (at >= K) at = 0;                          // no image folded, or every mean a NaN
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  out_k[0] = at;
  out_d[0] = acc[at] / n;
  out_d[1] = acc[K + at] / n;
  out_d[2] = k_ref >= 0 ? acc[k_ref] / n : nan;
  out_d[3] = k_ref >= 0 ? acc[K + k_ref] / n : nan;
}

#define SWEEP_CHECK_SHAPE(who)                                                                                                    \
  MI355_CHECK_ARG(B >= 1 && B <= SWEEP_MAX_B && len >= 1 && len <= SWEEP_MAX_LEN && (long long)B * len <= TEMP_MAX_N && K >= 1 &&   \
                      K <= SWEEP_MAX_K,                                                                                           \
                  who ": 1 <= B <= %d, 1 <= len <= 2^24, B * len <= 2^26 and 1 <= K <= %d expected (B=%d, len=%lld, K=%d)",       \
                  SWEEP_MAX_B, SWEEP_MAX_K, B, len, K)

static long long sweep_ws_need(int B, long long len, int K) { return (long long)B * sweep_chunks(len) * 2 * (K + 1); }

extern "C" int mi355_thr_sweep_chunk(void) { return SWEEP_CHUNK; }

extern "C" int mi355_thr_sweep_ws_ints(int B, long long len, int K) {
  SWEEP_CHECK_SHAPE("thr_sweep_ws_ints");
  return (int)sweep_ws_need(B, len, K);          // B * chunks <= 2^12 + B: below 2^28
}

extern "C" int mi355_thr_sweep(const float* scores, const float* target, int B, long long len, const float* thr, int K, int is_logit,
                               float tthr, int32_t* ws, long long ws_ints, int32_t* tp, int32_t* fp, int32_t* pos, mi355_stream_t s) {
  MI355_CHECK_ARG(scores, "thr_sweep: null pointer (scores)");
  MI355_CHECK_ARG(target, "thr_sweep: null pointer (target)");
  MI355_CHECK_ARG(thr, "thr_sweep: null pointer (thr)");
  MI355_CHECK_ARG(ws, "thr_sweep: null pointer (ws)");
  MI355_CHECK_ARG(tp && fp && pos, "thr_sweep: null pointer (tp, fp or pos)");
  SWEEP_CHECK_SHAPE("thr_sweep");
  const long long need = sweep_ws_need(B, len, K);
  MI355_CHECK_ARG(ws_ints >= need, "thr_sweep: workspace ws of %lld int32 elements is too short, %lld needed (B=%d, len=%lld, K=%d)",
                  ws_ints, need, B, len, K);
  hipStream_t st = (hipStream_t)s;
  const int nc = sweep_chunks(len);
  hipLaunchKernelGGL(sweep_hist_kernel, dim3(nc, B), dim3(256), 0, st, scores, target, len, thr, K, is_logit ? 1 : 0, tthr, ws);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(sweep_suffix_kernel, dim3(B), dim3(256), 0, st, ws, nc, K, tp, fp, pos);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_thr_sweep_fold(const int32_t* tp, const int32_t* fp, const int32_t* pos, int B, int K, double* acc,
                                    int64_t* n_images, mi355_stream_t s) {
  MI355_CHECK_ARG(tp && fp && pos, "thr_sweep_fold: null pointer (tp, fp or pos)");
  MI355_CHECK_ARG(acc, "thr_sweep_fold: null pointer (acc)");
  MI355_CHECK_ARG(n_images, "thr_sweep_fold: null pointer (n_images)");
  MI355_CHECK_ARG(B >= 1 && B <= SWEEP_MAX_B && K >= 1 && K <= SWEEP_MAX_K, "thr_sweep_fold: 1 <= B <= %d and 1 <= K <= %d expected (B=%d, K=%d)",
                  SWEEP_MAX_B, SWEEP_MAX_K, B, K);
  hipLaunchKernelGGL(sweep_fold_kernel, dim3(ceil_div(K, 256)), dim3(256), 0, (hipStream_t)s, tp, fp, pos, B, K, acc,
                     reinterpret_cast<long long*>(n_images));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_thr_sweep_pick(const double* acc, const int64_t* n_images, int K, int k_ref, double* out_d, int32_t* out_k,
                                    mi355_stream_t s) {
  MI355_CHECK_ARG(acc, "thr_sweep_pick: null pointer (acc)");
  MI355_CHECK_ARG(n_images, "thr_sweep_pick: null pointer (n_images)");
  MI355_CHECK_ARG(out_d && out_k, "thr_sweep_pick: null pointer (out_d or out_k)");
  MI355_CHECK_ARG(K >= 1 && K <= SWEEP_MAX_K && k_ref >= -1 && k_ref < K, "thr_sweep_pick: 1 <= K <= %d and -1 <= k_ref < K expected (K=%d, k_ref=%d)",
                  SWEEP_MAX_K, K, k_ref);
  hipLaunchKernelGGL(sweep_pick_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, acc, reinterpret_cast<const long long*>(n_images), K,
                     k_ref, out_d, out_k);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
