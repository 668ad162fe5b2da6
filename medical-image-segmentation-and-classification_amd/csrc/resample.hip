// Resampling statistics on the device: multinomial bootstrap weights, the evaluation figures of the tester on the resampled multiset
// (ranking metrics, confusion matrices, NaN-aware sums of per-sample values), percentile intervals over the replicates, and DeLong's
// structural components for the variance of an AUROC and the covariance of two.
//
// A resample is never materialised: replicate r is a row of int32 weights counts[r][i] = how often sample i was drawn, and every
// statistic is evaluated with those weights.  Row 0 of the weights is all ones, so row 0 of every output is the point estimate.
//
//   boot_counts_*         Philox4x32-10, counter (k >> 2, r, 0, 0), key = the seed's two halves; draw k is word k & 3, mapped to an index by
//                         (word * n) >> 32.  Integer adds into an LDS histogram while a row fits, into global memory above that.
//   resample_prep_kernel  after the segmented sort: per rank the sample index, its label and whether the rank opens / closes a tie
//                         group, in one int32.  None of it depends on the weights.
//   boot_rank_kernel      one workgroup per (replicate, segment) walks the ranks 256 at a time: a sum scan of the (negatives,
//                         positives) weights packed in one int64, a max scan that carries the packed prefix at the group's first rank
//                         (both halves grow with the rank, so the packed word does), the group sums at the last rank of each group.
//                         ap is folded per tile of the sort and the tiles in the order of rank_finalize_kernel (ranking.hip): with unit
//                         weights the result is mi355_rank_metrics' to the bit.
//   delong_fwd / bwd      the same scans without weights; the backward walk carries the prefix at the group's LAST rank to every rank
//                         of the group (a min scan from the right) and writes v2 at the sample's own index.
//   delong_cov_kernel     one workgroup per (class, model a, model b): exact integer sums for the means, then a two-pass covariance.
//   boot_confusion / boot_sums / boot_interval: one workgroup per replicate / (replicate, metric) / statistic.
//
// No floating-point atomics, nothing allocated, nothing synchronises, nothing read back; every fold has a fixed order.
#include "segsort.hpp"

#define RS_MAX_N SEGSORT_MAX_N                  /* R1 * n, S * n */
#define RS_LDS_MAX 8192                         /* ints of LDS histogram: the longest row boot_counts keeps on chip */
#define RS_MAX_C 64                             /* confusion matrix: C * C ints of LDS */
#define RS_MAX_R 8192                           /* replicates boot_interval sorts in LDS */
#define RS_KPT (SEGSORT_TILE / 256)             /* 256-rank steps per tile of the sort: the granularity of the ap partials */
#define RS_IDX 0x03ffffff                       /* item: sample index (< 2^26) | label | first | end */
#define RS_Y (1 << 28)
#define RS_FIRST (1 << 29)
#define RS_END (1 << 30)
#define RS_LO32 0xffffffffll

__device__ __forceinline__ double rs_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ void rs_put_i64(int* __restrict__ p, long long v) {          // ws is int32: no 8-byte alignment assumed
  p[0] = (int)(unsigned)((unsigned long long)v & 0xffffffffull);
  p[1] = (int)(unsigned)((unsigned long long)v >> 32);
}
__device__ __forceinline__ long long rs_get_i64(const int* __restrict__ p) {
  return (long long)(((unsigned long long)(unsigned)p[1] << 32) | (unsigned long long)(unsigned)p[0]);
}
__device__ __forceinline__ float rs_canonical(float x) { return (__builtin_bit_cast(uint32_t, x) << 1) == 0u ? 0.f : x; }

// sums over the 256 threads, the same value in every thread, waves folded in wave order; red = 4 elements of LDS, free on return
__device__ __forceinline__ long long rs_block_sum_i(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const long long r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ double rs_block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ long long rs_wave_incl_sum(long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
__device__ __forceinline__ long long rs_wave_incl_max(long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o, 64);
    if (lane >= o) v = v > u ? v : u;
  }
  return v;
}
__device__ __forceinline__ long long rs_wave_incl_min(long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o, 64);
    if (lane >= o) v = v < u ? v : u;
  }
  return v;
}

// ---- bootstrap weights ---------------------------------------------------------------------------------------------------------------
struct rs_u4 { uint32_t x, y, z, w; };

__device__ __forceinline__ rs_u4 rs_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}
__device__ __forceinline__ int rs_draw(uint32_t word, int n) { return (int)(((unsigned long long)word * (unsigned long long)n) >> 32); }

// grid (R1), 256 threads, n <= RS_LDS_MAX: the row's histogram in LDS
__global__ __launch_bounds__(256) void boot_counts_lds_kernel(uint32_t k0, uint32_t k1, int n, int* __restrict__ counts) {
  __shared__ int hist[RS_LDS_MAX];
  const int r = blockIdx.x, tid = threadIdx.x;
  int* __restrict__ row = counts + (size_t)r * n;
  if (r == 0) {
    for (int i = tid; i < n; i += 256) row[i] = 1;
    return;
  }
  for (int i = tid; i < n; i += 256) hist[i] = 0;
  __syncthreads();
  const int nb = (n + 3) >> 2;
  for (int b = tid; b < nb; b += 256) {
    const rs_u4 o = rs_philox((uint32_t)b, (uint32_t)r, 0u, 0u, k0, k1);
    const int k = 4 * b;
    atomicAdd(&hist[rs_draw(o.x, n)], 1);
    if (k + 1 < n) atomicAdd(&hist[rs_draw(o.y, n)], 1);
    if (k + 2 < n) atomicAdd(&hist[rs_draw(o.z, n)], 1);
    if (k + 3 < n) atomicAdd(&hist[rs_draw(o.w, n)], 1);
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) row[i] = hist[i];
}

// grid (ceil(R1 * n / 256)): row 0 = 1, the others 0
__global__ __launch_bounds__(256) void boot_counts_fill_kernel(long long total, int n, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) counts[i] = i < n ? 1 : 0;
}
// grid (ceil(ceil(n / 4) / 256), R), 256 threads: one Philox block per thread, non-returning integer adds
__global__ __launch_bounds__(256) void boot_counts_global_kernel(uint32_t k0, uint32_t k1, int n, int* __restrict__ counts) {
  const int r = blockIdx.y + 1;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= ((n + 3) >> 2)) return;
  int* __restrict__ row = counts + (size_t)r * n;
  const rs_u4 o = rs_philox((uint32_t)b, (uint32_t)r, 0u, 0u, k0, k1);
  const int k = 4 * b;
  atomicAdd(&row[rs_draw(o.x, n)], 1);
  if (k + 1 < n) atomicAdd(&row[rs_draw(o.y, n)], 1);
  if (k + 2 < n) atomicAdd(&row[rs_draw(o.z, n)], 1);
  if (k + 3 < n) atomicAdd(&row[rs_draw(o.w, n)], 1);
}

#define RS_CHECK_ROWS(who, R1, n)                                                                                                 \
  MI355_CHECK_ARG((R1) >= 2 && (n) >= 1 && (long long)(R1) * (n) <= RS_MAX_N,                                                     \
                  who ": R >= 1 replicates (R1 = R + 1 rows), n >= 1 and R1 * n <= 2^26 expected (R1=%lld, n=%lld)",              \
                  (long long)(R1), (long long)(n))

extern "C" int mi355_boot_counts_lds_max(void) { return RS_LDS_MAX; }

extern "C" int mi355_boot_counts(uint64_t seed, int R, long long n, int32_t* counts, mi355_stream_t s) {
  MI355_CHECK_ARG(counts, "boot_counts: null pointer (counts)");
  MI355_CHECK_ARG(R >= 1, "boot_counts: R >= 1 replicates expected (R=%d)", R);
  RS_CHECK_ROWS("boot_counts", (long long)R + 1, n);
  hipStream_t st = (hipStream_t)s;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  const int R1 = R + 1, N = (int)n;
  if (N <= RS_LDS_MAX) {
    hipLaunchKernelGGL(boot_counts_lds_kernel, dim3(R1), dim3(256), 0, st, k0, k1, N, counts);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
  }
  const long long total = (long long)R1 * n;
  hipLaunchKernelGGL(boot_counts_fill_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, total, N, counts);
  MI355_LAUNCH_CHECK();
  // R <= 2^26 / n < 2^13 here: a grid coordinate
  hipLaunchKernelGGL(boot_counts_global_kernel, dim3(ceil_div((N + 3) >> 2, 256), R), dim3(256), 0, st, k0, k1, N, counts);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- ranks: what the weights do not change -------------------------------------------------------------------------------------------
// grid (ceil(len / 256), S), 256 threads.  LABELS: the positives of segment s are labels == s % C.
template <bool LABELS>
__global__ __launch_bounds__(256) void resample_prep_kernel(const float* __restrict__ scores, const float* __restrict__ target,
                                                            const int* __restrict__ labels, const int* __restrict__ perm, int len, int C,
                                                            float thr, int* __restrict__ item) {
  const int s = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= len) return;
  const long long seg = (long long)s * len;
  const int i = perm[seg + k];
  const float v = rs_canonical(scores[seg + i]);
  const bool y = LABELS ? labels[i] == s % C : target[seg + i] > thr;
  const bool first = k == 0 || rs_canonical(scores[seg + perm[seg + k - 1]]) != v;
  const bool end = k == len - 1 || rs_canonical(scores[seg + perm[seg + k + 1]]) != v;
  item[seg + k] = i | (y ? RS_Y : 0) | (first ? RS_FIRST : 0) | (end ? RS_END : 0);
}

// One 256-rank step of the two scans.  v = this rank's packed weight (negatives << 32 | positives), first = it opens a group.
// On return incl = the packed weights up to and including the rank, gs = those before the first rank of its group; running / gcarry
// are advanced to the end of the step.  sm = [2][8] int64 of LDS, par alternates between the steps (one barrier per step).
__device__ __forceinline__ void rs_scan_step(long long v, bool first, long long (*sm)[8], int par, long long& running, long long& gcarry,
                                             long long& incl, long long& gs) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long incl_l = rs_wave_incl_sum(v);
  const long long m_l = rs_wave_incl_max(first ? incl_l - v : -1ll);
  if (lane == 63) {
    sm[par][w] = incl_l;
    sm[par][4 + w] = m_l;
  }
  __syncthreads();
  long long base = running, tot = running, g = gcarry, gnext = gcarry;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long sq = sm[par][q], mq = sm[par][4 + q];
    if (mq >= 0) {
      gnext = mq + tot;                         // tot = the packed weights before wave q
      g = q < w ? gnext : g;
    }
    base += q < w ? sq : 0;
    tot += sq;
  }
  incl = incl_l + base;
  gs = m_l >= 0 ? m_l + base : g;
  running = tot;
  gcarry = gnext;
}

// grid (R1, S), 256 threads.  pnu[r][s] = P, N, U2; ap[r][s].
__global__ __launch_bounds__(256) void boot_rank_kernel(const int* __restrict__ item, const int* __restrict__ counts, int len, int S,
                                                        long long* __restrict__ pnu, double* __restrict__ ap_out) {
  __shared__ long long sm[2][8];
  __shared__ long long redi[4];
  __shared__ double redd[4];
  const int r = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int* __restrict__ it = item + (size_t)s * len;
  const int* __restrict__ wt = counts + (size_t)r * len;
  long long pw = 0, tw = 0;
  for (int k = tid; k < len; k += 256) {
    const int e = it[k], wi = wt[e & RS_IDX];
    tw += wi;
    pw += (e & RS_Y) ? wi : 0;
  }
  const long long P = rs_block_sum_i(pw, redi), N = rs_block_sum_i(tw, redi) - P;
  long long running = 0, gcarry = 0, u2 = 0;
  double ap = 0.0, fold = 0.0;
  const int nsteps = (len + 255) / 256;
  for (int c = 0; c < nsteps; ++c) {
    const int k = c * 256 + tid;
    const bool valid = k < len;
    const int e = valid ? it[k] : 0;
    const long long wi = valid ? wt[e & RS_IDX] : 0;
    long long incl, gs;
    rs_scan_step((e & RS_Y) ? wi : wi << 32, (e & RS_FIRST) != 0, sm, c & 1, running, gcarry, incl, gs);
    if (e & RS_END) {
      const long long Bg = incl & RS_LO32, Ag = incl >> 32, Bp = gs & RS_LO32, Ap = gs >> 32;
      const long long pg = Bg - Bp, tp = P - Bp, fp = N - Ap;
      u2 += pg * (Ag + Ap);
      // (the fused multiply-add hipcc contracts rank_tile_kernel's `ap += a * b` to, written out: row 0 is held to its bits)
      if (pg > 0) ap = __builtin_fma((double)pg / (double)P, (double)tp / (double)(tp + fp), ap);
    }
    if (c % RS_KPT == RS_KPT - 1 || c == nsteps - 1) {            // a tile of the sort ends: its partial goes to thread tile % 256
      ap = wave_sum_d(ap);
      if (lane == 0) redd[w] = ap;
      __syncthreads();
      if (tid == ((c / RS_KPT) & 255)) fold += (redd[0] + redd[1]) + (redd[2] + redd[3]);
      __syncthreads();
      ap = 0.0;
    }
  }
  u2 = rs_block_sum_i(u2, redi);
  fold = rs_block_sum_d(fold, redd);
  if (tid == 0) {
    long long* o = pnu + 3 * ((size_t)r * S + s);
    o[0] = P;
    o[1] = N;
    o[2] = u2;
    ap_out[(size_t)r * S + s] = P > 0 ? fold : rs_nan();
  }
}

// ws = [perm : S len | item : S len | the sort's workspace]
static long long boot_rank_ws_need(int S, long long len) { return 2 * (long long)S * len + segsort_ws_need(S, len); }

#define RS_CHECK_SEG(who)                                                                                                         \
  MI355_CHECK_ARG(segsort_shape_ok(S, len), who ": 1 <= S <= %d, len >= 1 and S * len <= 2^26 expected (S=%d, len=%lld)",         \
                  SEGSORT_MAX_S, S, len)

extern "C" int mi355_boot_rank_ws_ints(int S, long long len) {
  RS_CHECK_SEG("boot_rank_ws_ints");
  return (int)boot_rank_ws_need(S, len);
}

extern "C" int mi355_boot_rank(const float* scores, const float* target, const int32_t* labels, int S, long long len, float thr,
                               const int32_t* counts, int R1, int32_t* ws, long long ws_ints, int64_t* counts64, double* ap,
                               mi355_stream_t s) {
  MI355_CHECK_ARG(scores, "boot_rank: null pointer (scores)");
  MI355_CHECK_ARG((target != nullptr) != (labels != nullptr), "boot_rank: exactly one of target and labels is expected (%s)",
                  target ? "both given" : "neither given");
  MI355_CHECK_ARG(counts, "boot_rank: null pointer (counts)");
  MI355_CHECK_ARG(ws, "boot_rank: null pointer (ws)");
  MI355_CHECK_ARG(counts64, "boot_rank: null pointer (counts64)");
  MI355_CHECK_ARG(ap, "boot_rank: null pointer (ap)");
  RS_CHECK_SEG("boot_rank");
  RS_CHECK_ROWS("boot_rank", R1, len);
  const long long need = boot_rank_ws_need(S, len);
  MI355_CHECK_ARG(ws_ints >= need, "boot_rank: workspace ws of %lld int32 elements is too short, %lld needed (S=%d, len=%lld)", ws_ints,
                  need, S, len);
  hipStream_t st = (hipStream_t)s;
  const long long n = (long long)S * len;
  const int L = (int)len;
  int* perm = ws;
  int* item = ws + n;
  int rc = segsort_launch(scores, S, len, ws + 2 * n, perm, st);
  if (rc != MI355_OK) return rc;
  const dim3 pgrid(ceil_div(len, 256), S), block(256);
  if (labels)
    hipLaunchKernelGGL((resample_prep_kernel<true>), pgrid, block, 0, st, scores, target, labels, perm, L, S, thr, item);
  else
    hipLaunchKernelGGL((resample_prep_kernel<false>), pgrid, block, 0, st, scores, target, labels, perm, L, S, thr, item);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(boot_rank_kernel, dim3(R1, S), block, 0, st, item, counts, L, S, reinterpret_cast<long long*>(counts64), ap);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- confusion matrices ---------------------------------------------------------------------------------------------------------------
// grid (R1), 256 threads: the replicate's C x C weights in LDS (each <= R1 * n <= 2^26), integer adds
__global__ __launch_bounds__(256) void boot_confusion_kernel(const int* __restrict__ pred, const int* __restrict__ labels, int n, int C,
                                                             const int* __restrict__ counts, long long* __restrict__ cm,
                                                             long long* __restrict__ bad) {
  __shared__ int hist[RS_MAX_C * RS_MAX_C];
  __shared__ long long redi[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int* __restrict__ wt = counts + (size_t)r * n;
  for (int i = tid; i < C * C; i += 256) hist[i] = 0;
  __syncthreads();
  long long nbad = 0;
  for (int i = tid; i < n; i += 256) {
    const int p = pred[i], y = labels[i], wi = wt[i];
    if (p >= 0 && p < C && y >= 0 && y < C) {
      if (wi) atomicAdd(&hist[y * C + p], wi);
    } else {
      nbad += wi;
    }
  }
  __syncthreads();
  for (int i = tid; i < C * C; i += 256) cm[(size_t)r * C * C + i] = hist[i];
  nbad = rs_block_sum_i(nbad, redi);
  if (tid == 0) bad[r] = nbad;
}

extern "C" int mi355_boot_confusion(const int32_t* pred, const int32_t* labels, long long n, int C, const int32_t* counts, int R1,
                                    int64_t* cm, int64_t* bad, mi355_stream_t s) {
  MI355_CHECK_ARG(pred, "boot_confusion: null pointer (pred)");
  MI355_CHECK_ARG(labels, "boot_confusion: null pointer (labels)");
  MI355_CHECK_ARG(counts, "boot_confusion: null pointer (counts)");
  MI355_CHECK_ARG(cm, "boot_confusion: null pointer (cm)");
  MI355_CHECK_ARG(bad, "boot_confusion: null pointer (bad)");
  MI355_CHECK_ARG(C >= 1 && C <= RS_MAX_C, "boot_confusion: 1 <= C <= %d expected (C=%d)", RS_MAX_C, C);
  RS_CHECK_ROWS("boot_confusion", R1, n);
  hipLaunchKernelGGL(boot_confusion_kernel, dim3(R1), dim3(256), 0, (hipStream_t)s, pred, labels, (int)n, C, counts,
                     reinterpret_cast<long long*>(cm), reinterpret_cast<long long*>(bad));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- NaN-aware weighted sums ------------------------------------------------------------------------------------------------------------
// grid (R1, M), 256 threads: thread t folds samples t, t + 256, ..., then lanes, then the four waves in wave order
__global__ __launch_bounds__(256) void boot_sums_kernel(const double* __restrict__ values, const int* __restrict__ counts, int n, int M,
                                                        double* __restrict__ sum, long long* __restrict__ weight) {
  __shared__ long long redi[4];
  __shared__ double redd[4];
  const int r = blockIdx.x, m = blockIdx.y;
  const double* __restrict__ v = values + (size_t)m * n;
  const int* __restrict__ wt = counts + (size_t)r * n;
  double a = 0.0;
  long long wsum = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double x = v[i];
    const int wi = wt[i];
    if (x == x) {
      a += (double)wi * x;
      wsum += wi;
    }
  }
  a = rs_block_sum_d(a, redd);
  wsum = rs_block_sum_i(wsum, redi);
  if (threadIdx.x == 0) {
    sum[(size_t)r * M + m] = a;
    weight[(size_t)r * M + m] = wsum;
  }
}

extern "C" int mi355_boot_sums(const double* values, int M, long long n, const int32_t* counts, int R1, double* sum, int64_t* weight,
                               mi355_stream_t s) {
  MI355_CHECK_ARG(values, "boot_sums: null pointer (values)");
  MI355_CHECK_ARG(counts, "boot_sums: null pointer (counts)");
  MI355_CHECK_ARG(sum, "boot_sums: null pointer (sum)");
  MI355_CHECK_ARG(weight, "boot_sums: null pointer (weight)");
  MI355_CHECK_ARG(M >= 1 && M <= SEGSORT_MAX_S, "boot_sums: 1 <= M <= %d expected (M=%d)", SEGSORT_MAX_S, M);
  RS_CHECK_ROWS("boot_sums", R1, n);
  MI355_CHECK_ARG((long long)M * n <= RS_MAX_N, "boot_sums: M * n <= 2^26 expected (M=%d, n=%lld)", M, n);
  hipLaunchKernelGGL(boot_sums_kernel, dim3(R1, M), dim3(256), 0, (hipStream_t)s, values, counts, (int)n, M, sum,
                     reinterpret_cast<long long*>(weight));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- percentile intervals ---------------------------------------------------------------------------------------------------------------
// numpy's method="linear": virtual index q (m - 1), a + (b - a) g below g = 0.5 and b - (b - a) (1 - g) from there
__device__ __forceinline__ double rs_quantile(const double* __restrict__ x, int m, double q) {
  const double pos = (double)(m - 1) * q, fl = floor(pos), g = pos - fl;
  int i0 = (int)fl;
  i0 = i0 < 0 ? 0 : (i0 > m - 1 ? m - 1 : i0);
  const int i1 = i0 + 1 > m - 1 ? m - 1 : i0 + 1;
  const double a = x[i0], b = x[i1], d = b - a;
  return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// grid (K), 256 threads: the R replicates of statistic k in LDS, NaN -> +inf (sorted behind the valid ones), a bitonic network over
// the next power of two, then the folds over the sorted valid values: thread t takes t, t + 256, ..., then lanes, then waves.
__global__ __launch_bounds__(256) void boot_interval_kernel(const double* __restrict__ reps, int R, int K, double lo_q, double hi_q,
                                                            double* __restrict__ out) {
  __shared__ double x[RS_MAX_R];
  __shared__ long long redi[4];
  __shared__ double redd[4];
  const int k = blockIdx.x, tid = threadIdx.x;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  int Np = 1;
  while (Np < R) Np <<= 1;
  long long nnan = 0;
  for (int i = tid; i < Np; i += 256) {
    double v = inf;
    if (i < R) {
      v = reps[(size_t)(i + 1) * K + k];
      if (v != v) {
        v = inf;
        ++nnan;
      }
    }
    x[i] = v;
  }
  const int valid = R - (int)rs_block_sum_i(nnan, redi);      // (its barriers order the stores to x as well)
  for (int size = 2; size <= Np; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (Np >> 1); t += 256) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool up = (i & size) == 0;
        const double a = x[i], b = x[j];
        if ((a > b) == up) {
          x[i] = b;
          x[j] = a;
        }
      }
      __syncthreads();
    }
  }
  double a = 0.0;
  for (int i = tid; i < valid; i += 256) a += x[i];
  const double mean = rs_block_sum_d(a, redd) / (double)valid;
  a = 0.0;
  for (int i = tid; i < valid; i += 256) {
    const double d = x[i] - mean;
    a += d * d;
  }
  const double ss = rs_block_sum_d(a, redd);
  if (tid == 0) {
    double* o = out + 6 * (size_t)k;
    o[0] = reps[k];
    o[1] = valid >= 1 ? mean : rs_nan();
    o[2] = valid >= 2 ? sqrt(ss / (double)(valid - 1)) : rs_nan();
    o[3] = valid >= 1 ? rs_quantile(x, valid, lo_q) : rs_nan();
    o[4] = valid >= 1 ? rs_quantile(x, valid, hi_q) : rs_nan();
    o[5] = (double)valid;
  }
}

extern "C" int mi355_boot_interval(const double* reps, int R1, int K, double lo_q, double hi_q, double* out, mi355_stream_t s) {
  MI355_CHECK_ARG(reps, "boot_interval: null pointer (reps)");
  MI355_CHECK_ARG(out, "boot_interval: null pointer (out)");
  MI355_CHECK_ARG(R1 >= 2 && R1 - 1 <= RS_MAX_R, "boot_interval: 1 <= R <= %d replicates (R1 = R + 1 rows) expected (R1=%d)", RS_MAX_R, R1);
  MI355_CHECK_ARG(K >= 1 && K <= (1 << 20), "boot_interval: 1 <= K <= 2^20 expected (K=%d)", K);
  MI355_CHECK_ARG(lo_q >= 0.0 && lo_q <= hi_q && hi_q <= 1.0, "boot_interval: 0 <= lo_q <= hi_q <= 1 expected (lo_q=%g, hi_q=%g)", lo_q,
                  hi_q);
  hipLaunchKernelGGL(boot_interval_kernel, dim3(K), dim3(256), 0, (hipStream_t)s, reps, R1 - 1, K, lo_q, hi_q, out);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- DeLong ------------------------------------------------------------------------------------------------------------------------------
// grid (S), 256 threads: pre[s][k] = (the packed counts up to and including rank k, those before the first rank of its group);
// tot[s] = P
__global__ __launch_bounds__(256) void delong_fwd_kernel(const int* __restrict__ item, int len, int* __restrict__ pre,
                                                         int* __restrict__ tot) {
  __shared__ long long sm[2][8];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int* __restrict__ it = item + (size_t)s * len;
  int* __restrict__ p = pre + 4 * (size_t)s * len;
  long long running = 0, gcarry = 0;
  const int nsteps = (len + 255) / 256;
  for (int c = 0; c < nsteps; ++c) {
    const int k = c * 256 + tid;
    const bool valid = k < len;
    const int e = valid ? it[k] : 0;
    long long incl, gs;
    rs_scan_step(valid ? ((e & RS_Y) ? 1ll : 1ll << 32) : 0ll, (e & RS_FIRST) != 0, sm, c & 1, running, gcarry, incl, gs);
    if (valid) {
      rs_put_i64(p + 4 * (size_t)k, incl);
      rs_put_i64(p + 4 * (size_t)k + 2, gs);
    }
  }
  if (tid == 0) tot[s] = (int)(running & RS_LO32);
}

// grid (S), 256 threads, from the last rank to the first; thread t takes rank base + 255 - t, so a scan in thread order runs from the
// right: the smallest packed prefix among the group ends at or behind a rank is that of its own group's end.
__global__ __launch_bounds__(256) void delong_bwd_kernel(const int* __restrict__ item, const int* __restrict__ pre,
                                                         const int* __restrict__ tot, int len, long long* __restrict__ v2,
                                                         long long* __restrict__ pnu) {
  __shared__ long long sm[2][4];
  __shared__ long long redi[4];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int* __restrict__ it = item + (size_t)s * len;
  const int* __restrict__ p = pre + 4 * (size_t)s * len;
  const long long P = tot[s];
  const long long big = 0x7fffffffffffffffll;
  long long carry = big, u2 = 0;
  const int nsteps = (len + 255) / 256;
  for (int c = nsteps - 1; c >= 0; --c) {
    const int k = c * 256 + 255 - tid;
    const bool valid = k < len;
    const int e = valid ? it[k] : 0;
    const long long incl = valid ? rs_get_i64(p + 4 * (size_t)k) : 0;
    const long long m_l = rs_wave_incl_min((e & RS_END) ? incl : big);
    if (lane == 63) sm[c & 1][w] = m_l;
    __syncthreads();
    long long before = carry, all = carry;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long mq = sm[c & 1][q];
      before = (q < w && mq < before) ? mq : before;
      all = mq < all ? mq : all;
    }
    const long long ge = m_l < before ? m_l : before;
    carry = all;
    if (valid) {
      const long long gs = rs_get_i64(p + 4 * (size_t)k + 2);
      const long long Bg = ge & RS_LO32, Ag = ge >> 32, Bp = gs & RS_LO32, Ap = gs >> 32;
      const bool y = (e & RS_Y) != 0;
      const long long v = y ? Ag + Ap : 2 * (P - Bg) + (Bg - Bp);
      v2[(size_t)s * len + (e & RS_IDX)] = v;
      u2 += y ? v : 0;
    }
  }
  u2 = rs_block_sum_i(u2, redi);
  if (tid == 0) {
    pnu[3 * (size_t)s + 0] = P;
    pnu[3 * (size_t)s + 1] = len - P;
    pnu[3 * (size_t)s + 2] = u2;
  }
}

// grid (M * M, C), 256 threads: models a, b of class c.  The means come from exact integer sums; the centred products are folded by
// thread t over samples t, t + 256, ..., then lanes, then waves.
__global__ __launch_bounds__(256) void delong_cov_kernel(const long long* __restrict__ v2, const int* __restrict__ labels, int n, int M,
                                                         int C, double* __restrict__ var, double* __restrict__ cov) {
  __shared__ long long redi[4];
  __shared__ double redd[4];
  const int a = blockIdx.x / M, b = blockIdx.x % M, c = blockIdx.y, tid = threadIdx.x;
  const long long* __restrict__ va = v2 + ((size_t)a * C + c) * n;
  const long long* __restrict__ vb = v2 + ((size_t)b * C + c) * n;
  long long cp = 0, sa1 = 0, sb1 = 0, sa0 = 0, sb0 = 0;
  for (int i = tid; i < n; i += 256) {
    const bool y = labels[i] == c;
    const long long x = va[i], z = vb[i];
    cp += y ? 1 : 0;
    sa1 += y ? x : 0;
    sb1 += y ? z : 0;
    sa0 += y ? 0 : x;
    sb0 += y ? 0 : z;
  }
  const long long P = rs_block_sum_i(cp, redi), N = n - P;
  sa1 = rs_block_sum_i(sa1, redi);
  sb1 = rs_block_sum_i(sb1, redi);
  sa0 = rs_block_sum_i(sa0, redi);
  sb0 = rs_block_sum_i(sb0, redi);
  const double d1 = 2.0 * (double)N, d0 = 2.0 * (double)P;        // V10 = v2 / (2 N) on the positives, V01 = v2 / (2 P) on the negatives
  const double ma1 = (double)sa1 / d1 / (double)P, mb1 = (double)sb1 / d1 / (double)P;
  const double ma0 = (double)sa0 / d0 / (double)N, mb0 = (double)sb0 / d0 / (double)N;
  double s1 = 0.0, s0 = 0.0;
  for (int i = tid; i < n; i += 256) {
    const bool y = labels[i] == c;
    const double x = (double)va[i], z = (double)vb[i];
    if (y) s1 += (x / d1 - ma1) * (z / d1 - mb1);
    else s0 += (x / d0 - ma0) * (z / d0 - mb0);
  }
  s1 = rs_block_sum_d(s1, redd);
  s0 = rs_block_sum_d(s0, redd);
  if (tid == 0) {
    const double r = (P >= 2 && N >= 2) ? s1 / (double)(P - 1) / (double)P + s0 / (double)(N - 1) / (double)N : rs_nan();
    cov[((size_t)c * M + a) * M + b] = r;
    if (a == b) var[(size_t)a * C + c] = r;
  }
}

// ws = [perm : S n | item : S n | pre : 4 S n | tot : S | the sort's workspace], S = M C
static long long delong_ws_need(int S, long long len) { return 6 * (long long)S * len + S + segsort_ws_need(S, len); }

#define RS_CHECK_DELONG(who)                                                                                                      \
  MI355_CHECK_ARG(M >= 1 && C >= 1 && (long long)M * C <= SEGSORT_MAX_S && segsort_shape_ok(M * C, n),                            \
                  who ": M, C >= 1, M * C <= %d, n >= 1 and M * C * n <= 2^26 expected (M=%d, C=%d, n=%lld)", SEGSORT_MAX_S, M, C, n)

extern "C" int mi355_delong_ws_ints(int M, int C, long long n) {
  RS_CHECK_DELONG("delong_ws_ints");
  const long long need = delong_ws_need(M * C, n);
  MI355_CHECK_ARG(need <= 0x7fffffffll, "delong_ws_ints: the workspace exceeds 2^31 int32 elements (M=%d, C=%d, n=%lld)", M, C, n);
  return (int)need;
}

extern "C" int mi355_delong(const float* scores, const int32_t* labels, int M, int C, long long n, int32_t* ws, long long ws_ints,
                            int64_t* v2, int64_t* pnu, double* var, double* cov, mi355_stream_t s) {
  MI355_CHECK_ARG(scores, "delong: null pointer (scores)");
  MI355_CHECK_ARG(labels, "delong: null pointer (labels)");
  MI355_CHECK_ARG(ws, "delong: null pointer (ws)");
  MI355_CHECK_ARG(v2, "delong: null pointer (v2)");
  MI355_CHECK_ARG(pnu, "delong: null pointer (pnu)");
  MI355_CHECK_ARG(var, "delong: null pointer (var)");
  MI355_CHECK_ARG(cov, "delong: null pointer (cov)");
  RS_CHECK_DELONG("delong");
  const int S = M * C, L = (int)n;
  const long long need = delong_ws_need(S, n);
  MI355_CHECK_ARG(ws_ints >= need, "delong: workspace ws of %lld int32 elements is too short, %lld needed (M=%d, C=%d, n=%lld)", ws_ints,
                  need, M, C, n);
  hipStream_t st = (hipStream_t)s;
  const long long sn = (long long)S * n;
  int* perm = ws;
  int* item = ws + sn;
  int* pre = ws + 2 * sn;
  int* tot = ws + 6 * sn;
  int rc = segsort_launch(scores, S, n, tot + S, perm, st);
  if (rc != MI355_OK) return rc;
  const dim3 block(256);
  hipLaunchKernelGGL((resample_prep_kernel<true>), dim3(ceil_div(n, 256), S), block, 0, st, scores, (const float*)nullptr, labels, perm, L,
                     C, 0.f, item);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(delong_fwd_kernel, dim3(S), block, 0, st, item, L, pre, tot);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(delong_bwd_kernel, dim3(S), block, 0, st, item, pre, tot, L, reinterpret_cast<long long*>(v2),
                     reinterpret_cast<long long*>(pnu));
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(delong_cov_kernel, dim3(M * M, C), block, 0, st, reinterpret_cast<const long long*>(v2), labels, L, M, C, var, cov);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
