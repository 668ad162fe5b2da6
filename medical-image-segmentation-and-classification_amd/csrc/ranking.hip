// Threshold-free evaluation on the device: ROC-AUC, average precision and the ROC / precision-recall operating points of fp32 scores
// ranked by the segmented sort of segsort.hip, and the calibration of a classifier (ECE, Brier, NLL) with its softmax in double.
//
// mi355_rank_metrics.  Per segment the scores are ranked ascending; a tie group g is a run of equal scores (-0.0 == +0.0).  With A_g,
// B_g the negatives / positives up to and including group g (A_0 = B_0 = 0), p_g = B_g - B_{g-1}, tp_g = P - B_{g-1}, fp_g = N - A_{g-1}:
//   U2 = sum_g p_g (A_g + A_{g-1})             twice the Mann-Whitney statistic, ties counted half: an exact integer
//   ap = sum_g (p_g / P) tp_g / (tp_g + fp_g)  the step-wise average precision
//   operating point T - 1 - g = (score_g, tp_g, fp_g): descending thresholds
// Everything is evaluated at the LAST rank of a group, which knows B_g and A_g from its own cumulative count; what it needs from the
// group's FIRST rank — the rank itself and the positives before it — is a running maximum over the first ranks seen so far, because
// both grow with the rank.  A group may span any number of tiles, so that maximum is carried across tiles by a max-scan.
//
//   rank_gather_kernel    per tile of SEGSORT_TILE ranks: the sorted scores, the labels as one bit per rank, the tile's positives,
//                         its first ranks of groups, the last of them and the positives of the tile before it
//   (segsort_rowscan)     positives / groups before each tile, P and T per segment
//   rank_carry_kernel     one workgroup per segment: (last first-rank, positives before it) over the tiles before each tile
//   rank_tile_kernel      ballots within the tile, the group sums in int64 / double, the operating points; one partial per tile
//   rank_finalize_kernel  one workgroup per segment folds the partials in a fixed order
//
// mi355_cls_calibration.  One thread per sample: softmax in double after subtracting the row maximum, confidence, first argmax, Guo
// et al.'s bin (k / M, (k + 1) / M], -log p_y, the multi-class Brier term, the probabilities rounded to fp32 once and transposed.  A
// workgroup folds its 256 samples per bin in sample order, one workgroup folds the workgroups in order.
//
// No floating-point atomics, nothing allocated, nothing synchronises, nothing read back.  A NaN score differs from every score, its
// own included: it is a group of its own wherever the sort put it, and every index stays in bounds.
#include "segsort.hpp"

#define RANK_KPT (SEGSORT_TILE / 256)
#define RANK_WORDS (SEGSORT_TILE / 32)          /* int32 words of label bits per tile */

__device__ __forceinline__ void rank_put_double(int* __restrict__ p, double v) {        // ws is int32: no 8-byte alignment assumed
  p[0] = __double2loint(v);
  p[1] = __double2hiint(v);
}
__device__ __forceinline__ double rank_get_double(const int* __restrict__ p) { return __hiloint2double(p[1], p[0]); }
__device__ __forceinline__ void rank_put_i64(int* __restrict__ p, long long v) {
  p[0] = (int)(unsigned)((unsigned long long)v & 0xffffffffull);
  p[1] = (int)(unsigned)((unsigned long long)v >> 32);
}
__device__ __forceinline__ long long rank_get_i64(const int* __restrict__ p) {
  return (long long)(((unsigned long long)(unsigned)p[1] << 32) | (unsigned long long)(unsigned)p[0]);
}

// -0.0 -> +0.0, as the sort does before it takes the bit pattern: one bit pattern per tie group
__device__ __forceinline__ float rank_canonical(float x) {
  return (__builtin_bit_cast(uint32_t, x) << 1) == 0u ? 0.f : x;
}

// sum / maximum over the 256 threads, the same value in every thread; red = 4 ints of LDS, free again on return
__device__ __forceinline__ int rank_block_sum(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ int rank_block_max(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int r = max(max(red[0], red[1]), max(red[2], red[3]));
  __syncthreads();
  return r;
}

// grid (ntiles, S), 256 threads: rank k = t0 + j * 256 + tid, so (step j, wave w) covers 64 consecutive ranks and owns one 64-bit
// word of label bits.  tilecnt[s][0][tile] = positives, tilecnt[s][1][tile] = first ranks of groups; tilelast[s][tile] = (the last
// first-rank of the tile or -1, the tile's positives before it).
template <bool LABELS>
__global__ __launch_bounds__(256) void rank_gather_kernel(const float* __restrict__ scores, const float* __restrict__ target,
                                                          const int* __restrict__ labels, const int* __restrict__ perm, int len,
                                                          int ntiles, float thr, float* __restrict__ sorted, int* __restrict__ ybits,
                                                          int* __restrict__ tilecnt, int* __restrict__ tilelast) {
  __shared__ float sc[SEGSORT_TILE + 1];        // sc[1 + r] = the score at rank t0 + r, sc[0] = the one before the tile
  __shared__ int red[4];
  const int s = blockIdx.y, tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long seg = (long long)s * len;
  const int t0 = tile * SEGSORT_TILE;
  bool y[RANK_KPT];
  int npos = 0;
#pragma unroll
  for (int j = 0; j < RANK_KPT; ++j) {
    const int r = j * 256 + tid, k = t0 + r;
    const bool valid = k < len;
    float v = 0.f;
    y[j] = false;
    if (valid) {
      const int i = perm[seg + k];
      v = rank_canonical(scores[seg + i]);
      y[j] = LABELS ? labels[i] == s : target[seg + i] > thr;
      sorted[seg + k] = v;
    }
    sc[1 + r] = v;
    const unsigned long long b = __ballot(y[j]);
    if (lane == 0) {
      int* word = ybits + ((size_t)s * ntiles + tile) * RANK_WORDS + 2 * (j * 4 + w);
      word[0] = (int)(unsigned)(b & 0xffffffffull);
      word[1] = (int)(unsigned)(b >> 32);
    }
    npos += y[j] ? 1 : 0;
  }
  if (tid == 0) {
    float v = 0.f;
    if (t0 > 0) {
      v = rank_canonical(scores[seg + perm[seg + t0 - 1]]);
    }
    sc[0] = v;
  }
  __syncthreads();
  int nfirst = 0, last = -1;
#pragma unroll
  for (int j = 0; j < RANK_KPT; ++j) {
    const int r = j * 256 + tid, k = t0 + r;
    const bool first = k < len && (k == 0 || sc[r] != sc[1 + r]);
    nfirst += first ? 1 : 0;
    last = first ? k : last;                    // k grows with j
  }
  npos = rank_block_sum(npos, red);
  nfirst = rank_block_sum(nfirst, red);
  last = rank_block_max(last, red);
  int pre = 0;
#pragma unroll
  for (int j = 0; j < RANK_KPT; ++j) pre += (y[j] && t0 + j * 256 + tid < last) ? 1 : 0;
  pre = rank_block_sum(pre, red);
  if (tid == 0) {
    tilecnt[((size_t)s * 2 + 0) * ntiles + tile] = npos;
    tilecnt[((size_t)s * 2 + 1) * ntiles + tile] = nfirst;
    tilelast[2 * ((size_t)s * ntiles + tile) + 0] = last;
    tilelast[2 * ((size_t)s * ntiles + tile) + 1] = pre;
  }
}

// (first rank << 32) | positives before it: both grow with the rank, so the later first-rank is the larger word and 0 — rank 0 with
// nothing before it, which every segment has — is the identity of the maximum.
__device__ __forceinline__ long long rank_wave_incl_max(long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o, 64);
    if (lane >= o) v = v > u ? v : u;
  }
  return v;
}

// grid (S), 256 threads, after the row scan (tilecnt[s][0] = positives before each tile): carry[s][tile] = the maximum over the tiles
// before `tile`, 256 tiles per step.
__global__ __launch_bounds__(256) void rank_carry_kernel(const int* __restrict__ tilecnt, const int* __restrict__ tilelast, int ntiles,
                                                         int* __restrict__ carry) {
  __shared__ long long wmax[4];
  const int s = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  const int* __restrict__ posbefore = tilecnt + (size_t)s * 2 * ntiles;
  long long running = 0;
  for (int base = 0; base < ntiles; base += 256) {
    const int i = base + tid;
    long long v = 0;
    if (i < ntiles) {
      const int last = tilelast[2 * ((size_t)s * ntiles + i)];
      if (last >= 0) v = ((long long)last << 32) | (long long)(posbefore[i] + tilelast[2 * ((size_t)s * ntiles + i) + 1]);
    }
    const long long incl = rank_wave_incl_max(v);
    if ((tid & 63) == 63) wmax[w] = incl;
    __syncthreads();
    long long before = running, all = running;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long m = wmax[q];
      before = (q < w && m > before) ? m : before;
      all = m > all ? m : all;
    }
    long long excl = __shfl_up(incl, 1, 64);
    excl = (tid & 63) == 0 ? 0 : excl;
    excl = excl > before ? excl : before;
    if (i < ntiles) rank_put_i64(carry + 2 * ((size_t)s * ntiles + i), excl);
    running = all;
    __syncthreads();
  }
}

// grid (ntiles, S), 256 threads.  partial[s][tile] = (U2 : int64, ap : double), 4 ints.
template <bool CURVE>
__global__ __launch_bounds__(256) void rank_tile_kernel(const float* __restrict__ sorted, const int* __restrict__ ybits,
                                                        const int* __restrict__ tilecnt, const int* __restrict__ tot,
                                                        const int* __restrict__ carry, int len, int ntiles, int* __restrict__ partial,
                                                        float* __restrict__ thresholds, int* __restrict__ ctp, int* __restrict__ cfp) {
  __shared__ unsigned long long yb[RANK_KPT][4];      // label bits of (step, wave)
  __shared__ int wfirst[RANK_KPT][4];                 // first ranks of groups in (step, wave)
  __shared__ long long wlast[RANK_KPT][4];            // its last one as (rank << 32) | positives before it, or -1
  __shared__ long long redi[4];
  __shared__ double redd[4];
  const int s = blockIdx.y, tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long seg = (long long)s * len;
  const int t0 = tile * SEGSORT_TILE;
  const unsigned long long le = (2ull << lane) - 1ull;      // lanes 0 .. lane (2 << 63 wraps to 0: every bit)
  if (tid < RANK_KPT * 4) {
    const int* word = ybits + ((size_t)s * ntiles + tile) * RANK_WORDS + 2 * tid;
    yb[tid >> 2][tid & 3] = ((unsigned long long)(unsigned)word[1] << 32) | (unsigned long long)(unsigned)word[0];
  }
  float v[RANK_KPT];
  unsigned long long fb[RANK_KPT];
  bool end[RANK_KPT];
#pragma unroll
  for (int j = 0; j < RANK_KPT; ++j) {
    const int k = t0 + j * 256 + tid;
    const bool valid = k < len;
    v[j] = valid ? sorted[seg + k] : 0.f;
    const bool first = valid && (k == 0 || sorted[seg + k - 1] != v[j]);
    end[j] = valid && (k == len - 1 || sorted[seg + k + 1] != v[j]);
    fb[j] = __ballot(first);
    if (lane == 0) wfirst[j][w] = __popcll(fb[j]);
  }
  __syncthreads();
  const int P = tot[2 * s], T = tot[2 * s + 1], N = len - P;
  int posb = tilecnt[((size_t)s * 2 + 0) * ntiles + tile];        // positives / first ranks at the ranks before (step j, wave w)
  int firstb = tilecnt[((size_t)s * 2 + 1) * ntiles + tile];
  // the wave's last first-rank needs the positives before it: the positives before the wave are known only now
  int mypos[RANK_KPT], myfirst[RANK_KPT];
#pragma unroll
  for (int j = 0; j < RANK_KPT; ++j) {
    int mp = posb, mf = firstb;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = __popcll(yb[j][q]), f = wfirst[j][q];
      mp += q < w ? c : 0;
      mf += q < w ? f : 0;
      posb += c;
      firstb += f;
    }
    mypos[j] = mp;
    myfirst[j] = mf;
    if (lane == 0) {
      long long e = -1;
      if (fb[j] != 0ull) {
        const int L = 63 - __clzll((long long)fb[j]);
        const unsigned long long lt = (1ull << L) - 1ull;
        e = ((long long)(t0 + j * 256 + w * 64 + L) << 32) | (long long)(mp + __popcll(yb[j][w] & lt));
      }
      wlast[j][w] = e;
    }
  }
  __syncthreads();
  long long running = rank_get_i64(carry + 2 * ((size_t)s * ntiles + tile));
  long long u2 = 0;
  double ap = 0.0;
#pragma unroll
  for (int j = 0; j < RANK_KPT; ++j) {
    long long mine = running;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long e = wlast[j][q];
      mine = (q < w && e >= 0) ? e : mine;
      running = e >= 0 ? e : running;
    }
    if (end[j]) {
      const int k = t0 + j * 256 + tid;
      const unsigned long long ybw = yb[j][w];
      const unsigned long long m = fb[j] & le;
      int gs, gb;                               // the group's first rank and the positives before it
      if (m != 0ull) {
        const int L = 63 - __clzll((long long)m);
        gs = t0 + j * 256 + w * 64 + L;
        gb = mypos[j] + __popcll(ybw & ((1ull << L) - 1ull));
      } else {
        gs = (int)(mine >> 32);
        gb = (int)(mine & 0xffffffffll);
      }
      const int Bg = mypos[j] + __popcll(ybw & le), Ag = (k + 1) - Bg;
      const int Bp = gb, Ap = gs - gb;
      const int pg = Bg - Bp, tp = P - Bp, fp = N - Ap;
      u2 += (long long)pg * (long long)(Ag + Ap);
      if (pg > 0) ap += ((double)pg / (double)P) * ((double)tp / (double)(tp + fp));
      if constexpr (CURVE) {
        const int g = myfirst[j] + __popcll(m) - 1;      // groups are counted by their first ranks: 0 <= g < T <= len
        const long long o = seg + (T - 1 - g);
        thresholds[o] = v[j];
        ctp[o] = tp;
        cfp[o] = fp;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u2 += __shfl_xor(u2, o, 64);
  ap = wave_sum_d(ap);
  if (lane == 0) {
    redi[w] = u2;
    redd[w] = ap;
  }
  __syncthreads();
  if (tid == 0) {
    int* p = partial + 4 * ((size_t)s * ntiles + tile);
    rank_put_i64(p, (redi[0] + redi[1]) + (redi[2] + redi[3]));
    rank_put_double(p + 2, (redd[0] + redd[1]) + (redd[2] + redd[3]));
  }
}

// grid (S), 256 threads: thread t folds partials t, t + 256, ..., then lanes, then the four waves in wave order.
__global__ __launch_bounds__(256) void rank_finalize_kernel(const int* __restrict__ partial, const int* __restrict__ tot, int len,
                                                            int ntiles, long long* __restrict__ counts, double* __restrict__ ap,
                                                            int* __restrict__ npoints) {
  __shared__ long long redi[4];
  __shared__ double redd[4];
  const int s = blockIdx.x;
  long long u2 = 0;
  double a = 0.0;
  for (int i = threadIdx.x; i < ntiles; i += 256) {
    const int* p = partial + 4 * ((size_t)s * ntiles + i);
    u2 += rank_get_i64(p);
    a += rank_get_double(p + 2);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u2 += __shfl_xor(u2, o, 64);
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) {
    redi[threadIdx.x >> 6] = u2;
    redd[threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int P = tot[2 * s], T = tot[2 * s + 1];
    counts[4 * (size_t)s + 0] = P;
    counts[4 * (size_t)s + 1] = len - P;
    counts[4 * (size_t)s + 2] = (redi[0] + redi[1]) + (redi[2] + redi[3]);
    counts[4 * (size_t)s + 3] = T;
    ap[s] = P > 0 ? (redd[0] + redd[1]) + (redd[2] + redd[3]) : __longlong_as_double(0x7ff8000000000000ll);
    if (npoints) npoints[s] = T;
  }
}

// ws = [perm : n | sorted : n | ybits : S nt TILE/32 | tilecnt : 2 S nt | tot : 2 S | tilelast : 2 S nt | carry : 2 S nt |
//       partial : 4 S nt | the sort's workspace]
static long long rank_ws_need(int S, long long len) {
  const long long n = (long long)S * len, snt = (long long)S * segsort_ntiles(len);
  return 2 * n + snt * (RANK_WORDS + 10) + 2 * (long long)S + segsort_ws_need(S, len);
}

#define RANK_CHECK_SHAPE(who)                                                                                                     \
  MI355_CHECK_ARG(segsort_shape_ok(S, len), who ": 1 <= S <= %d, len >= 1 and S * len <= 2^26 expected (S=%d, len=%lld)",         \
                  SEGSORT_MAX_S, S, len)

extern "C" int mi355_rank_ws_ints(int S, long long len) {
  RANK_CHECK_SHAPE("rank_ws_ints");
  return (int)rank_ws_need(S, len);
}

extern "C" int mi355_rank_metrics(const float* scores, const float* target, const int32_t* labels, int S, long long len, float thr,
                                  int32_t* ws, long long ws_ints, int64_t* counts, double* ap, float* thresholds, int32_t* tp,
                                  int32_t* fp, int32_t* npoints, mi355_stream_t s) {
  MI355_CHECK_ARG(scores, "rank_metrics: null pointer (scores)");
  MI355_CHECK_ARG((target != nullptr) != (labels != nullptr), "rank_metrics: exactly one of target and labels is expected (%s)",
                  target ? "both given" : "neither given");
  MI355_CHECK_ARG(ws, "rank_metrics: null pointer (ws)");
  MI355_CHECK_ARG(counts, "rank_metrics: null pointer (counts)");
  MI355_CHECK_ARG(ap, "rank_metrics: null pointer (ap)");
  const bool curve = thresholds || tp || fp || npoints;
  MI355_CHECK_ARG(!curve || (thresholds && tp && fp && npoints),
                  "rank_metrics: the curve outputs thresholds, tp, fp and npoints are given together or all null");
  RANK_CHECK_SHAPE("rank_metrics");
  const long long need = rank_ws_need(S, len);
  MI355_CHECK_ARG(ws_ints >= need, "rank_metrics: workspace ws of %lld int32 elements is too short, %lld needed (S=%d, len=%lld)",
                  ws_ints, need, S, len);
  hipStream_t st = (hipStream_t)s;
  const long long n = (long long)S * len;
  const int nt = segsort_ntiles(len);
  const size_t snt = (size_t)S * nt;
  int* perm = ws;
  float* sorted = reinterpret_cast<float*>(ws + n);
  int* ybits = ws + 2 * n;
  int* tilecnt = ybits + snt * RANK_WORDS;
  int* tot = tilecnt + 2 * snt;
  int* tilelast = tot + 2 * (size_t)S;
  int* carry = tilelast + 2 * snt;
  int* partial = carry + 2 * snt;
  int32_t* sort_ws = partial + 4 * snt;
  int rc = segsort_launch(scores, S, len, sort_ws, perm, st);
  if (rc != MI355_OK) return rc;
  const dim3 grid(nt, S), block(256);
  const int L = (int)len;
  if (labels)
    hipLaunchKernelGGL((rank_gather_kernel<true>), grid, block, 0, st, scores, target, labels, perm, L, nt, thr, sorted, ybits, tilecnt,
                       tilelast);
  else
    hipLaunchKernelGGL((rank_gather_kernel<false>), grid, block, 0, st, scores, target, labels, perm, L, nt, thr, sorted, ybits, tilecnt,
                       tilelast);
  MI355_LAUNCH_CHECK();
  rc = segsort_rowscan_launch(tilecnt, tot, nt, 2, S, st);
  if (rc != MI355_OK) return rc;
  hipLaunchKernelGGL(rank_carry_kernel, dim3(S), block, 0, st, tilecnt, tilelast, nt, carry);
  MI355_LAUNCH_CHECK();
  if (curve)
    hipLaunchKernelGGL((rank_tile_kernel<true>), grid, block, 0, st, sorted, ybits, tilecnt, tot, carry, L, nt, partial, thresholds, tp, fp);
  else
    hipLaunchKernelGGL((rank_tile_kernel<false>), grid, block, 0, st, sorted, ybits, tilecnt, tot, carry, L, nt, partial, thresholds, tp, fp);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_finalize_kernel, dim3(S), block, 0, st, partial, tot, L, nt, reinterpret_cast<long long*>(counts), ap, npoints);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- calibration -------------------------------------------------------------------------------------------------------------------
#define CALIB_MAX_BINS 1024
#define CALIB_MAX_C 4096

// per workgroup: count[bins], correct[bins], conf[bins] (double), nll, brier (double)
static inline long long calib_block_ints(int bins) { return 4 * (long long)bins + 4; }

// grid (ceil(N / 256)), 256 threads: thread = sample
__global__ __launch_bounds__(256) void calib_rows_kernel(const float* __restrict__ x, const int* __restrict__ labels, int N, int C,
                                                         int is_prob, int bins, float* __restrict__ scores_t, int* __restrict__ part) {
  __shared__ double sconf[256];
  __shared__ int sbin[256];                     // the bin, with bit 30 set where the prediction is the label; -1 behind the last sample
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * 256 + tid;
  double nll = 0.0, brier = 0.0;
  sbin[tid] = -1;
  sconf[tid] = 0.0;
  if (i < N) {
    const float* __restrict__ row = x + i * C;
    const int y = labels[i];
    double mx = (double)row[0], sum = 1.0;
    if (!is_prob) {
      for (int c = 1; c < C; ++c) mx = fmax(mx, (double)row[c]);
      sum = 0.0;
      for (int c = 0; c < C; ++c) sum += exp((double)row[c] - mx);
    }
    double conf = -1.0, py = __longlong_as_double(0x7ff8000000000000ll);
    int pred = 0;
    for (int c = 0; c < C; ++c) {
      const double p = is_prob ? (double)row[c] : exp((double)row[c] - mx) / sum;
      if (p > conf) {                           // the first maximum
        conf = p;
        pred = c;
      }
      const double d = p - (c == y ? 1.0 : 0.0);
      brier += d * d;
      if (c == y) py = is_prob ? p : (double)row[c] - mx;
      scores_t[(long long)c * N + i] = (float)p;
    }
    nll = is_prob ? -log(py) : log(sum) - py;   // logits: log sum exp(x - max) - (x_y - max), no quotient under the logarithm
    int b = (int)ceil(conf * (double)bins) - 1;
    b = b < 0 ? 0 : (b > bins - 1 ? bins - 1 : b);
    sbin[tid] = b | (pred == y ? 1 << 30 : 0);
    sconf[tid] = conf;
  }
  nll = wave_sum_d(nll);
  brier = wave_sum_d(brier);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = nll;
    red[1][tid >> 6] = brier;
  }
  __syncthreads();
  int* __restrict__ mine = part + (size_t)blockIdx.x * (4 * (size_t)bins + 4);
  for (int m = tid; m < bins; m += 256) {       // thread = bin: the workgroup's samples in sample order
    int cnt = 0, ok = 0;
    double cs = 0.0;
    for (int q = 0; q < 256; ++q) {
      const int b = sbin[q];
      if (b >= 0 && (b & 0xffff) == m) {
        ++cnt;
        ok += b >> 30;
        cs += sconf[q];
      }
    }
    mine[m] = cnt;
    mine[bins + m] = ok;
    rank_put_double(mine + 2 * bins + 2 * m, cs);
  }
  if (tid == 0) {
    rank_put_double(mine + 4 * bins, (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
    rank_put_double(mine + 4 * bins + 2, (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
  }
}

// one workgroup: thread = bin folds the workgroups in order; nll / brier: thread t folds workgroups t, t + 256, ..., then lanes, then
// the four waves; the ECE is folded over the bins in bin order by one thread
__global__ __launch_bounds__(256) void calib_finalize_kernel(const int* __restrict__ part, int nblocks, int N, int bins,
                                                             long long* __restrict__ bin_count, long long* __restrict__ bin_correct,
                                                             double* __restrict__ bin_conf, double* __restrict__ out) {
  __shared__ double gap[CALIB_MAX_BINS];
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  const size_t stride = 4 * (size_t)bins + 4;
  for (int m = tid; m < bins; m += 256) {
    long long cnt = 0, ok = 0;
    double cs = 0.0;
    for (int b = 0; b < nblocks; ++b) {
      const int* p = part + b * stride;
      cnt += p[m];
      ok += p[bins + m];
      cs += rank_get_double(p + 2 * bins + 2 * m);
    }
    bin_count[m] = cnt;
    bin_correct[m] = ok;
    bin_conf[m] = cs;
    gap[m] = fabs((double)ok - cs);
  }
  double nll = 0.0, brier = 0.0;
  for (int b = tid; b < nblocks; b += 256) {
    const int* p = part + b * stride + 4 * (size_t)bins;
    nll += rank_get_double(p);
    brier += rank_get_double(p + 2);
  }
  nll = wave_sum_d(nll);
  brier = wave_sum_d(brier);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = nll;
    red[1][tid >> 6] = brier;
  }
  __syncthreads();
  if (tid == 0) {
    double e = 0.0;
    for (int m = 0; m < bins; ++m) e += gap[m];
    out[0] = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (double)N;
    out[1] = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (double)N;
    out[2] = e / (double)N;
  }
}

#define CALIB_CHECK_SHAPE(who)                                                                                                    \
  MI355_CHECK_ARG(N >= 1 && C >= 1 && C <= CALIB_MAX_C && (long long)N * C <= SEGSORT_MAX_N,                                      \
                  who ": N >= 1, 1 <= C <= %d and N * C <= 2^26 expected (N=%d, C=%d)", CALIB_MAX_C, N, C);                       \
  MI355_CHECK_ARG(bins >= 1 && bins <= CALIB_MAX_BINS, who ": 1 <= bins <= %d expected (bins=%d)", CALIB_MAX_BINS, bins)

extern "C" int mi355_cls_calibration_ws_ints(int N, int C, int bins) {
  CALIB_CHECK_SHAPE("cls_calibration_ws_ints");
  return (int)(ceil_div(N, 256) * calib_block_ints(bins));
}

extern "C" int mi355_cls_calibration(const float* x, int N, int C, int is_prob, const int32_t* labels, int bins, int32_t* ws,
                                     long long ws_ints, int64_t* bin_count, int64_t* bin_correct, double* bin_conf, double* out,
                                     float* scores_t, mi355_stream_t s) {
  MI355_CHECK_ARG(x, "cls_calibration: null pointer (x)");
  MI355_CHECK_ARG(labels, "cls_calibration: null pointer (labels)");
  MI355_CHECK_ARG(ws, "cls_calibration: null pointer (ws)");
  MI355_CHECK_ARG(bin_count, "cls_calibration: null pointer (bin_count)");
  MI355_CHECK_ARG(bin_correct, "cls_calibration: null pointer (bin_correct)");
  MI355_CHECK_ARG(bin_conf, "cls_calibration: null pointer (bin_conf)");
  MI355_CHECK_ARG(out, "cls_calibration: null pointer (out)");
  MI355_CHECK_ARG(scores_t, "cls_calibration: null pointer (scores_t)");
  CALIB_CHECK_SHAPE("cls_calibration");
  const int nb = ceil_div(N, 256);
  const long long need = nb * calib_block_ints(bins);
  MI355_CHECK_ARG(ws_ints >= need, "cls_calibration: workspace ws of %lld int32 elements is too short, %lld needed (N=%d, bins=%d)",
                  ws_ints, need, N, bins);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(calib_rows_kernel, dim3(nb), dim3(256), 0, st, x, labels, N, C, is_prob ? 1 : 0, bins, scores_t, ws);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(calib_finalize_kernel, dim3(1), dim3(256), 0, st, ws, nb, N, bins, reinterpret_cast<long long*>(bin_count),
                     reinterpret_cast<long long*>(bin_correct), bin_conf, out);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
