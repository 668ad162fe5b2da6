// Weight averaging along the optimiser trajectory (mi355/averaging.py; nothing in the reference): an exponential moving average
// (Mean Teacher, timm's ModelEmaV2) or an equal-weight average (SWA, Izmailov et al. 2018) of the flat fp32 parameter buffer and of
// the BatchNorm running statistics, the exchange of the live and the averaged weights, and the bias correction behind
// averaging.update_bn.
//   avg_update       : avg = avg + a * (p - avg) over one flat range, a from a device-side update counter
//   avg_update_table : the same over rows {avg pointer, p pointer, n} held in device memory (the BatchNorm buffers, one launch)
//   swap_table       : dst <-> src over such rows
//   bn_debias_table  : running /= 1 - (1 - momentum)^nbt over rows {running pointer, nbt pointer, C}
// Every floating-point operation of the update is rounded on its own (no FMA contraction) and nothing is atomic: the output is
// bit-identical run to run and equals tests/averaging_ref.py's float32 restatement.  The coefficient and the skip decision are read
// from device memory, so a step never waits for the host and the launches can be captured.
// Pure streaming, 12 bytes per element (two reads, one write).  A range whose two pointers share their offset within 16 bytes is
// swept with 16-byte accesses between a scalar head (up to the first 16-byte boundary) and a scalar tail; any other range is scalar.
#include "common.hpp"

namespace {

constexpr int WA_THREADS = 256;
constexpr int WA_MAX_BLOCKS = 2048;          // about 8 workgroups per CU; longer ranges are strided
constexpr int WA_TABLE_UPDATE_GX = 4;        // workgroups per row: BatchNorm buffers are at most a few thousand floats
constexpr int WA_TABLE_SWAP_GX = 512;        // one row is the whole flat parameter buffer
constexpr int WA_DEBIAS_GX = 2;

struct Coef {
  float a;
  int what;      // 0: leave avg alone, 1: avg = p, 2: avg = avg + a * (p - avg)
};

// a is formed in double from the update count t (this update included) and rounded to float once
__device__ __forceinline__ Coef avg_coef(int mode, float decay, float warmup, const int32_t* __restrict__ count,
                                         const float* __restrict__ found_inf) {
  Coef c{0.f, 0};
  if (found_inf && found_inf[0] != 0.f) return c;
  const int32_t t = count[0];
  if (t < 1) return c;
  if (mode == 1) {
    c.what = t == 1 ? 1 : 2;
    c.a = (float)(1.0 / (double)t);
  } else {
    double d = (double)decay;
    if (warmup > 0.f) {
      const double w = (1.0 + (double)t) / ((double)warmup + (double)t);
      if (w < d) d = w;
    }
    c.what = 2;
    c.a = (float)(1.0 - d);
  }
  return c;
}

struct UpdateOp {
  float a;
  __device__ __forceinline__ void operator()(float& d, float& s) const {
#pragma clang fp contract(off)
    const float diff = s - d;
    const float step = a * diff;
    const float r = d + step;
    d = diff == 0.f ? d : r;          // p == avg keeps avg's bits (-0 + +0 would be +0)
  }
};
struct CopyOp {
  __device__ __forceinline__ void operator()(float& d, float& s) const { d = s; }
};
struct SwapOp {
  __device__ __forceinline__ void operator()(float& d, float& s) const {
    const float t = d;
    d = s;
    s = t;
  }
};

// op(dst[i], src[i]) for i in [0, n), the calling threads being `tid` of `nthreads`; WRITE_SRC: src is stored back too.
template <bool WRITE_SRC, typename Op>
__device__ __forceinline__ void sweep(float* dst, float* src, long long n, long long tid, long long nthreads, Op op) {
  const uintptr_t db = (uintptr_t)dst, sb = (uintptr_t)src;
  long long head = n;                                              // all scalar unless both pointers meet a 16-byte boundary together
  if (((db ^ sb) & 15) == 0 && (db & 3) == 0) head = (long long)(((16 - (db & 15)) & 15) >> 2);
  if (head > n) head = n;
  const long long nv = (n - head) >> 2;
  const long long tail0 = head + 4 * nv, edge = head + (n - tail0);
  for (long long q = tid; q < nv; q += nthreads) {
    float* dp = dst + head + 4 * q;
    float* sp = src + head + 4 * q;
    Vec16<float> vd = ld16(dp), vs = ld16(sp);
#pragma unroll
    for (int k = 0; k < 4; ++k) op(vd.v[k], vs.v[k]);
    st16(dp, vd);
    if constexpr (WRITE_SRC) st16(sp, vs);
  }
  for (long long e = tid; e < edge; e += nthreads) {
    const long long i = e < head ? e : tail0 + (e - head);
    float d = dst[i], s = src[i];
    op(d, s);
    dst[i] = d;
    if constexpr (WRITE_SRC) src[i] = s;
  }
}

__global__ __launch_bounds__(WA_THREADS) void avg_update_kernel(float* avg, const float* p, long long n, int mode, float decay,
                                                                float warmup, const int32_t* __restrict__ count,
                                                                const float* __restrict__ found_inf) {
  const Coef c = avg_coef(mode, decay, warmup, count, found_inf);
  if (c.what == 0) return;
  const long long tid = (long long)blockIdx.x * WA_THREADS + threadIdx.x, nthreads = (long long)gridDim.x * WA_THREADS;
  if (c.what == 1)
    sweep<false>(avg, const_cast<float*>(p), n, tid, nthreads, CopyOp{});
  else
    sweep<false>(avg, const_cast<float*>(p), n, tid, nthreads, UpdateOp{c.a});
}

// blockIdx.y is the row: its three words are uniform in a workgroup
__global__ __launch_bounds__(WA_THREADS) void avg_update_table_kernel(const int64_t* __restrict__ table, int mode, float decay,
                                                                      float warmup, const int32_t* __restrict__ count,
                                                                      const float* __restrict__ found_inf) {
  const Coef c = avg_coef(mode, decay, warmup, count, found_inf);
  if (c.what == 0) return;
  const int64_t* row = table + 3 * (size_t)blockIdx.y;
  float* avg = reinterpret_cast<float*>((uintptr_t)row[0]);
  float* p = reinterpret_cast<float*>((uintptr_t)row[1]);
  const long long n = row[2];
  if (n <= 0 || !avg || !p) return;
  const long long tid = (long long)blockIdx.x * WA_THREADS + threadIdx.x, nthreads = (long long)gridDim.x * WA_THREADS;
  if (c.what == 1)
    sweep<false>(avg, p, n, tid, nthreads, CopyOp{});
  else
    sweep<false>(avg, p, n, tid, nthreads, UpdateOp{c.a});
}

__global__ __launch_bounds__(WA_THREADS) void swap_table_kernel(const int64_t* __restrict__ table) {
  const int64_t* row = table + 3 * (size_t)blockIdx.y;
  float* a = reinterpret_cast<float*>((uintptr_t)row[0]);
  float* b = reinterpret_cast<float*>((uintptr_t)row[1]);
  const long long n = row[2];
  if (n <= 0 || !a || !b || a == b) return;
  const long long tid = (long long)blockIdx.x * WA_THREADS + threadIdx.x, nthreads = (long long)gridDim.x * WA_THREADS;
  sweep<true>(a, b, n, tid, nthreads, SwapOp{});
}

__global__ __launch_bounds__(WA_THREADS) void bn_debias_table_kernel(const int64_t* __restrict__ table, float momentum) {
  const int64_t* row = table + 3 * (size_t)blockIdx.y;
  float* running = reinterpret_cast<float*>((uintptr_t)row[0]);
  const int64_t* nbt = reinterpret_cast<const int64_t*>((uintptr_t)row[1]);
  const long long C = row[2];
  if (C <= 0 || !running || !nbt) return;
  const int64_t k = nbt[0];
  if (k <= 0) return;                                              // that BatchNorm never ran: nothing to correct
  const double corr = 1.0 - pow(1.0 - (double)momentum, (double)k);
  for (long long c = (long long)blockIdx.x * WA_THREADS + threadIdx.x; c < C; c += (long long)gridDim.x * WA_THREADS)
    running[c] = (float)((double)running[c] / corr);
}

int check_mode(const char* who, int mode, float decay, float warmup) {
  MI355_CHECK_ARG(mode == 0 || mode == 1, "%s: mode %d (0 = EMA, 1 = equal average)", who, mode);
  MI355_CHECK_ARG(mode == 1 || (decay >= 0.f && decay <= 1.f && warmup >= 0.f), "%s: decay %g outside [0, 1] or warmup %g < 0", who,
                  (double)decay, (double)warmup);
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_avg_update_grid_elems(void) { return WA_MAX_BLOCKS * WA_THREADS * 4; }

extern "C" int mi355_avg_update(float* avg, const float* p, long long n, int mode, float decay, float warmup, const int32_t* count,
                                const float* found_inf, mi355_stream_t s) {
  MI355_CHECK_ARG(n >= 0, "avg_update: n = %lld", n);
  if (int rc = check_mode("avg_update", mode, decay, warmup)) return rc;
  if (n == 0) return MI355_OK;
  MI355_CHECK_ARG(avg && p && count, "avg_update: null pointer");
  MI355_CHECK_ARG((((uintptr_t)avg | (uintptr_t)p) & 3) == 0, "avg_update: pointers must be 4-byte aligned");
  const uintptr_t ab = (uintptr_t)avg, pb = (uintptr_t)p, bytes = (uintptr_t)n * sizeof(float);
  MI355_CHECK_ARG(ab == pb || ab + bytes <= pb || pb + bytes <= ab, "avg_update: avg and p overlap without being the same range");
  long long blocks = ((n + 3) / 4 + WA_THREADS - 1) / WA_THREADS;
  if (blocks > WA_MAX_BLOCKS) blocks = WA_MAX_BLOCKS;
  hipLaunchKernelGGL(avg_update_kernel, dim3((unsigned)blocks), dim3(WA_THREADS), 0, (hipStream_t)s, avg, p, n, mode, decay, warmup,
                     count, found_inf);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_avg_update_table(const int64_t* table, int rows, int mode, float decay, float warmup, const int32_t* count,
                                      const float* found_inf, mi355_stream_t s) {
  MI355_CHECK_ARG(rows >= 0 && rows <= 65535, "avg_update_table: rows = %d (0 .. 65535)", rows);
  if (int rc = check_mode("avg_update_table", mode, decay, warmup)) return rc;
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(table && count, "avg_update_table: null pointer");
  hipLaunchKernelGGL(avg_update_table_kernel, dim3(WA_TABLE_UPDATE_GX, (unsigned)rows), dim3(WA_THREADS), 0, (hipStream_t)s, table, mode,
                     decay, warmup, count, found_inf);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_swap_table(const int64_t* table, int rows, mi355_stream_t s) {
  MI355_CHECK_ARG(rows >= 0 && rows <= 65535, "swap_table: rows = %d (0 .. 65535)", rows);
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(table, "swap_table: null pointer");
  hipLaunchKernelGGL(swap_table_kernel, dim3(WA_TABLE_SWAP_GX, (unsigned)rows), dim3(WA_THREADS), 0, (hipStream_t)s, table);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_bn_debias_table(const int64_t* table, int rows, float momentum, mi355_stream_t s) {
  MI355_CHECK_ARG(rows >= 0 && rows <= 65535, "bn_debias_table: rows = %d (0 .. 65535)", rows);
  MI355_CHECK_ARG(momentum > 0.f && momentum <= 1.f, "bn_debias_table: momentum %g outside (0, 1]", (double)momentum);
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(table, "bn_debias_table: null pointer");
  hipLaunchKernelGGL(bn_debias_table_kernel, dim3(WA_DEBIAS_GX, (unsigned)rows), dim3(WA_THREADS), 0, (hipStream_t)s, table, momentum);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
