// Multi-class segmentation: per-pixel softmax cross-entropy + per-class soft Dice on fp32 logits z [N][C][HW] (the NCHW map the
// K-channel heads write) and uint8 labels y [N][HW], and the argmax / confusion-matrix pass of the metrics.  2 <= C <= 16; a pixel
// is valid when its label is in [0, C), every other label (ignore_index among them) selects nothing and is never used as an index.
// With p = softmax_c(z), v the valid mask, w the class weights (NULL: ones):
//
//   CE      = sum_v w[y] (logsumexp(z) - z_y) / sum_v w[y]                         (0 when no pixel is valid)
//   dice_c  = (2 I_c + smooth) / (P_c + T_c + smooth),  I_c = sum_v p_c [y = c],  P_c = sum_v p_c,  T_c = sum_v [y = c]
//   Dice    = 1 - mean_{c in S} dice_c   (sums over the batch, or per image and the N terms averaged)
//   dz_k    = gs (ce_weight w[y] (p_k - [y = k]) / sum w  +  dice_weight p_k (g_k - sum_c g_c p_c)),  g_c = -(a_c [y = c] - b_c) [c in S] / |S|
//
// The launches of seg_loss.hip: the forward leaves one row of (CE numerator, sum w, I_c, P_c, T_c) per workgroup, a fold (one
// workgroup per image, then one for the batch) adds the rows in a fixed order and leaves the loss terms and the backward's
// coefficients in `state`, the backward is one pass that reads them and the device-side gradient scale.  Inputs are widened to double, exp / log are evaluated in
// double, every sum is a double taken in a fixed order, results are rounded to float once on store: no floating-point atomics, the
// same input gives the same bytes.  Nothing is allocated and nothing synchronises.
//
// Load path: a workgroup owns chunks of MC_CHUNK consecutive pixels of one image; with HW % 4 == 0 and aligned bases a lane
// moves four pixels — C 16-byte plane loads and one 32-bit label load, all issued before the first use — otherwise one pixel per
// lane and trip.  Loads are never put under a condition (a lane past the end reads pixel 0 again and drops it: its label is
// forced out of range); only stores are guarded.
#include "common.hpp"

#define MC_CHUNK 1024             /* pixels per workgroup trip: 256 lanes x 4 */
#define MC_ROW MI355_MCSEG_ROW    /* doubles per partial row */
#define MC_MAX_N 65535            /* the image index is the grid's y coordinate */
#define MC_MAX_HW (1LL << 30)

static int mc_gx(int N, long long HW) {
  long long gx = (HW + MC_CHUNK - 1) / MC_CHUNK;
  long long cap = 2048 / N;       // about eight workgroups per CU over the batch; the rest is walked chunk by chunk
  if (cap < 1) cap = 1;
  return (int)(gx < cap ? gx : cap);
}

// E pixels of every class plane and their labels, from unconditional loads
template <int C, int E>
__device__ __forceinline__ void mc_load(const float* __restrict__ zn, const uint8_t* __restrict__ yn, long long HW, long long px,
                                        bool inb, float (&zv)[C][E], int (&lab)[E]) {
  const long long q = inb ? px : 0;
  if constexpr (E == 4) {
    f32x4 v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = *reinterpret_cast<const f32x4*>(zn + (size_t)c * HW + q);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(yn + q);
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) zv[c][k] = v[c][k];
#pragma unroll
    for (int k = 0; k < 4; ++k) lab[k] = inb ? (int)((w >> (8 * k)) & 255u) : 255;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) zv[c][0] = zn[(size_t)c * HW + q];
    const int w = yn[q];
    lab[0] = inb ? w : 255;
  }
}

// e_c = exp(z_c - max z) in double, returns their sum (>= 1)
template <int C, int E>
__device__ __forceinline__ double mc_softmax(const float (&zv)[C][E], int k, double (&e)[C], float& m) {
  m = zv[0][k];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, zv[c][k]);
  double s = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = exp((double)zv[c][k] - (double)m);
    s += e[c];
  }
  return s;
}

// grid (gx, N).  partial[(n * gx + g) * MC_ROW + {0, 1, 2 + c, 2 + C + c, 2 + 2 C + c}] = the workgroup's sums of
// w[y] (lse - z_y), w[y], I_c, P_c, T_c.
template <int C, int E>
__global__ __launch_bounds__(256) void mcseg_fwd_kernel(const float* __restrict__ z, const uint8_t* __restrict__ y, long long HW,
                                                        const float* __restrict__ weight, double* __restrict__ partial) {
  __shared__ double sw[16];
  __shared__ double red[4][2 + 3 * C];
  const int n = blockIdx.y, tid = threadIdx.x;
  if (tid < 16) sw[tid] = (weight && tid < C) ? (double)weight[tid] : 1.0;
  __syncthreads();
  const float* __restrict__ zn = z + (size_t)n * C * HW;
  const uint8_t* __restrict__ yn = y + (size_t)n * HW;
  const long long nch = (HW + MC_CHUNK - 1) / MC_CHUNK;
  double ce = 0, ws = 0, I[C], P[C];
  int T[C];
#pragma unroll
  for (int c = 0; c < C; ++c) I[c] = 0, P[c] = 0, T[c] = 0;
  for (long long ch = blockIdx.x; ch < nch; ch += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < 4 / E; ++j) {
      const long long px = ch * MC_CHUNK + (long long)j * 256 + (long long)tid * E;
      float zv[C][E];
      int lab[E];
      mc_load<C, E>(zn, yn, HW, px, px < HW, zv, lab);
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int l = lab[k];
        if (l < C) {      // (arithmetic only: every load is above)
          double e[C];
          float m;
          const double s = mc_softmax<C, E>(zv, k, e, m);
          const double inv = 1.0 / s, w = sw[l];
          double zy = 0;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const double p = e[c] * inv;
            const bool hit = l == c;
            zy = hit ? (double)zv[c][k] - (double)m : zy;
            P[c] += p;
            I[c] += hit ? p : 0.0;
            T[c] += hit ? 1 : 0;
          }
          ce += w * (log(s) - zy);
          ws += w;
        }
      }
    }
  }
  // thread -> wave -> workgroup, in double, always in the same order
  const int lane = tid & 63, wave = tid >> 6;
  double d;
  d = wave_sum_d(ce);
  if (lane == 0) red[wave][0] = d;
  d = wave_sum_d(ws);
  if (lane == 0) red[wave][1] = d;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    d = wave_sum_d(I[c]);
    if (lane == 0) red[wave][2 + c] = d;
    d = wave_sum_d(P[c]);
    if (lane == 0) red[wave][2 + C + c] = d;
    d = wave_sum_d((double)T[c]);
    if (lane == 0) red[wave][2 + 2 * C + c] = d;
  }
  __syncthreads();
  if (tid < 2 + 3 * C)
    partial[((size_t)n * gridDim.x + blockIdx.x) * MC_ROW + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// sum of v over the workgroup's 256 threads in a fixed order, in every thread
__device__ __forceinline__ double mc_block_sum(double v, double (&red)[4]) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// out[q] (q < R) = the sum over `count` rows of R doubles, `stride` doubles apart, in a fixed order: the 256 threads form
// 256 / R row groups, thread (part, q) adds rows part, part + parts, ... in row order (loads of consecutive q coalesce and the
// groups' loads are in flight together: one thread adding all rows pays a memory latency per row), thread q then adds the groups'
// sums in group order.  The grouping depends on R alone, so the same rows give the same bytes.  Every thread must call it.
__device__ __forceinline__ void mc_fold_rows(const double* base, size_t stride, int count, int R, double (&sh)[256],
                                             double* out) {
  const int tid = threadIdx.x, parts = 256 / R, part = tid / R, q = tid % R;
  double v = 0;
  if (part < parts)
    for (int g = part; g < count; g += parts) v += base[(size_t)g * stride + q];
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  if (tid < R) {
    double t = sh[tid];
    for (int p2 = 1; p2 < parts; ++p2) t += sh[p2 * R + tid];
    out[tid] = t;
  }
  __syncthreads();
}

// grid (N): image n's gx rows are folded into its first row (mcseg_finalize_kernel reads only those).
__global__ __launch_bounds__(256) void mcseg_fold_kernel(double* __restrict__ partial, int C, int gx) {
  __shared__ double sh[256];
  double* base = partial + (size_t)blockIdx.x * gx * MC_ROW;
  mc_fold_rows(base, MC_ROW, gx, 2 + 3 * C, sh, base);      // (every row is read before the barrier in front of the write)
}

// One workgroup, behind mcseg_fold_kernel (gx > 1): (a) the N image rows are folded in a fixed order (CE numerator and sum w; the
// class sums are used in batch mode); (b) thread-strided (n, c): the Dice coefficients of the backward; the Dice terms meet in a
// fixed-order block sum.
// state[0] = 1 / sum w (0 when no pixel is valid), state[1] = sum w, state[2 + 2 (n C + c) + {0, 1}] = (a_c, b_c) [c in S] / (|S| G)
// with the sums of image n (per_sample, G = N) or of the batch (G = 1, the same pair for every image).
__global__ __launch_bounds__(256) void mcseg_finalize_kernel(const double* __restrict__ partial, int N, int C, int gx, float ce_weight,
                                                             float dice_weight, float smooth, int per_sample,
                                                             int include_background, double* __restrict__ state,
                                                             float* __restrict__ loss) {
  __shared__ double tot[MC_ROW];
  __shared__ double sh[256];
  __shared__ double red[4];
  const int tid = threadIdx.x, R = 2 + 3 * C;
  mc_fold_rows(partial, (size_t)gx * MC_ROW, N, R, sh, tot);
  const double sm = smooth;
  const int c0 = include_background ? 0 : 1;
  const double k = 1.0 / ((double)(C - c0) * (per_sample ? (double)N : 1.0));
  double dsum = 0;
  for (long long i = tid; i < (long long)N * C; i += 256) {
    const int n = (int)(i / C), c = (int)(i % C);
    const double* src = per_sample ? partial + (size_t)n * gx * MC_ROW : tot;
    const double Ic = src[2 + c], Pc = src[2 + C + c], Tc = src[2 + 2 * C + c];
    const double den = Pc + Tc + sm, num = 2.0 * Ic + sm;
    const bool in = c >= c0;
    state[2 + 2 * i] = in ? 2.0 / den * k : 0.0;
    state[2 + 2 * i + 1] = in ? num / (den * den) * k : 0.0;
    if (in && (per_sample || n == 0)) dsum += num / den;
  }
  dsum = mc_block_sum(dsum, red);
  if (tid == 0) {
    const double wsum = tot[1];
    const double cev = wsum > 0 ? tot[0] / wsum : 0.0, dice = 1.0 - dsum * k;
    state[0] = wsum > 0 ? 1.0 / wsum : 0.0;
    state[1] = wsum;
    loss[0] = (float)((double)ce_weight * cev + (double)dice_weight * dice);
    loss[1] = (float)cev;
    loss[2] = (float)dice;
  }
}

// grid (gx, N), the forward's sweep.  With A_c, B_c the image's pair from `state`, D = sum_c B_c p_c - A_y p_y:
//   dz_k = gs (cw w[y] (p_k - [y = k]) + dice_weight p_k (B_k - A_k [y = k] - D)),  cw = ce_weight / sum w;  +0 at ignored pixels.
template <int C, int E>
__global__ __launch_bounds__(256) void mcseg_bwd_kernel(const float* __restrict__ z, const uint8_t* __restrict__ y, long long HW,
                                                        const float* __restrict__ weight, float ce_weight, float dice_weight,
                                                        const double* __restrict__ state, const float* __restrict__ gscale,
                                                        float* __restrict__ dz) {
  __shared__ double sw[16], sA[16], sB[16];
  const int n = blockIdx.y, tid = threadIdx.x;
  if (tid < 16) {
    sw[tid] = (weight && tid < C) ? (double)weight[tid] : 1.0;
    sA[tid] = tid < C ? state[2 + 2 * ((size_t)n * C + tid)] : 0.0;
    sB[tid] = tid < C ? state[2 + 2 * ((size_t)n * C + tid) + 1] : 0.0;
  }
  __syncthreads();
  const double gs = gscale ? (double)gscale[0] : 1.0;
  const double cw = (double)ce_weight * state[0], dw = dice_weight;
  const float* __restrict__ zn = z + (size_t)n * C * HW;
  const uint8_t* __restrict__ yn = y + (size_t)n * HW;
  float* __restrict__ dn = dz + (size_t)n * C * HW;
  const long long nch = (HW + MC_CHUNK - 1) / MC_CHUNK;
  for (long long ch = blockIdx.x; ch < nch; ch += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < 4 / E; ++j) {
      const long long px = ch * MC_CHUNK + (long long)j * 256 + (long long)tid * E;
      const bool inb = px < HW;
      float zv[C][E], o[C][E];
      int lab[E];
      mc_load<C, E>(zn, yn, HW, px, inb, zv, lab);
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int l = lab[k];
#pragma unroll
        for (int c = 0; c < C; ++c) o[c][k] = 0.f;
        if (l < C) {
          double e[C];
          float m;
          const double s = mc_softmax<C, E>(zv, k, e, m);
          const double inv = 1.0 / s, cww = cw * sw[l];
          double D = 0, py = 0;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            e[c] *= inv;
            D += sB[c] * e[c];
            py = l == c ? e[c] : py;
          }
          D -= sA[l] * py;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const bool hit = l == c;
            const double g = (hit ? sB[c] - sA[c] : sB[c]) - D;
            o[c][k] = (float)(gs * (cww * (hit ? e[c] - 1.0 : e[c]) + dw * e[c] * g));
          }
        }
      }
      if (inb) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if constexpr (E == 4) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = o[c][k];
            *reinterpret_cast<f32x4*>(dn + (size_t)c * HW + px) = v;
          } else {
            dn[(size_t)c * HW + px] = o[c][0];
          }
        }
      }
    }
  }
}

// grid (gx, N).  pred = the first maximum over c (v > best in ascending c from best = -inf, pred = 0: ties go to the lower class, a
// NaN never wins); conf[n][y][pred] += 1 at valid pixels through an integer LDS histogram and integer global atomics: exact and
// independent of the order.  pred (when given) is written for every pixel.
template <int C, int E>
__global__ __launch_bounds__(256) void mcseg_confusion_kernel(const float* __restrict__ z, const uint8_t* __restrict__ y, long long HW,
                                                              int32_t* __restrict__ conf, uint8_t* __restrict__ pred) {
  __shared__ int hist[C * C];
  const int n = blockIdx.y, tid = threadIdx.x;
  if (tid < C * C) hist[tid] = 0;
  __syncthreads();
  const float* __restrict__ zn = z + (size_t)n * C * HW;
  const uint8_t* __restrict__ yn = y + (size_t)n * HW;
  const long long nch = (HW + MC_CHUNK - 1) / MC_CHUNK;
  for (long long ch = blockIdx.x; ch < nch; ch += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < 4 / E; ++j) {
      const long long px = ch * MC_CHUNK + (long long)j * 256 + (long long)tid * E;
      const bool inb = px < HW;
      float zv[C][E];
      int lab[E];
      mc_load<C, E>(zn, yn, HW, px, inb, zv, lab);
      uint32_t packed = 0;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        float best = -__builtin_inff();
        int p = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const bool gt = zv[c][k] > best;
          best = gt ? zv[c][k] : best;
          p = gt ? c : p;
        }
        if (lab[k] < C) atomicAdd(&hist[lab[k] * C + p], 1);
        packed |= (uint32_t)p << (8 * k);
      }
      if (pred && inb) {
        if constexpr (E == 4) *reinterpret_cast<uint32_t*>(pred + (size_t)n * HW + px) = packed;
        else pred[(size_t)n * HW + px] = (uint8_t)packed;
      }
    }
  }
  __syncthreads();
  if (tid < C * C && hist[tid] != 0) atomicAdd(conf + (size_t)n * C * C + tid, hist[tid]);
}

static bool mc_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

// f(C{}, E{}) with the class count and the pixels per lane as compile-time constants
#define MC_DISPATCH(C_, VEC_, F)                                            \
  switch (C_) {                                                             \
    case 2: if (VEC_) F(2, 4) else F(2, 1) break;                           \
    case 3: if (VEC_) F(3, 4) else F(3, 1) break;                           \
    case 4: if (VEC_) F(4, 4) else F(4, 1) break;                           \
    case 5: if (VEC_) F(5, 4) else F(5, 1) break;                           \
    case 6: if (VEC_) F(6, 4) else F(6, 1) break;                           \
    case 7: if (VEC_) F(7, 4) else F(7, 1) break;                           \
    case 8: if (VEC_) F(8, 4) else F(8, 1) break;                           \
    case 9: if (VEC_) F(9, 4) else F(9, 1) break;                           \
    case 10: if (VEC_) F(10, 4) else F(10, 1) break;                        \
    case 11: if (VEC_) F(11, 4) else F(11, 1) break;                        \
    case 12: if (VEC_) F(12, 4) else F(12, 1) break;                        \
    case 13: if (VEC_) F(13, 4) else F(13, 1) break;                        \
    case 14: if (VEC_) F(14, 4) else F(14, 1) break;                        \
    case 15: if (VEC_) F(15, 4) else F(15, 1) break;                        \
    default: if (VEC_) F(16, 4) else F(16, 1) break;                        \
  }

static int mc_check_shape(const char* who, int N, int C, long long HW, int ignore_index) {
  MI355_CHECK_ARG(N > 0 && N <= MC_MAX_N && HW > 0 && HW <= MC_MAX_HW, "%s: 0 < N <= %d and 0 < HW <= 2^30 expected (N=%d, HW=%lld)",
                  who, MC_MAX_N, N, HW);
  MI355_CHECK_ARG(C >= 2 && C <= 16, "%s: 2 <= C <= 16 expected (C=%d)", who, C);
  MI355_CHECK_ARG(ignore_index == -1 || (ignore_index >= C && ignore_index <= 255),
                  "%s: ignore_index must be -1 or in [C, 255] (ignore_index=%d, C=%d)", who, ignore_index, C);
  return MI355_OK;
}

extern "C" int mi355_mcseg_rows(int N, long long HW) {
  if (!(N > 0 && N <= MC_MAX_N && HW > 0 && HW <= MC_MAX_HW)) {
    mi355_set_error("mcseg_rows: 0 < N <= %d and 0 < HW <= 2^30 expected (N=%d, HW=%lld)", MC_MAX_N, N, HW);
    return -1;
  }
  return N * mc_gx(N, HW);
}

extern "C" int mi355_mcseg_loss_fwd(const float* z, const uint8_t* y, int N, int C, long long HW, const float* weight,
                                    int ignore_index, float ce_weight, float dice_weight, float smooth, int per_sample,
                                    int include_background, double* partial, double* state, float* loss, mi355_stream_t s) {
  MI355_CHECK_ARG(z && y && partial && state && loss, "mcseg_loss_fwd: null pointer");
  if (int rc = mc_check_shape("mcseg_loss_fwd", N, C, HW, ignore_index)) return rc;
  MI355_CHECK_ARG(ce_weight >= 0.f && dice_weight >= 0.f && smooth >= 0.f,
                  "mcseg_loss_fwd: ce_weight, dice_weight and smooth must not be negative (%g, %g, %g)", (double)ce_weight,
                  (double)dice_weight, (double)smooth);
  MI355_CHECK_ARG(mc_aligned(z, 4) && mc_aligned(partial, 8) && mc_aligned(state, 8) && mc_aligned(loss, 4),
                  "mcseg_loss_fwd: z and loss must be 4-byte, partial and state 8-byte aligned");
  const int gx = mc_gx(N, HW);
  const bool vec = HW % 4 == 0 && mc_aligned(z, 16) && mc_aligned(y, 4);
#define MC_FWD(C_, E_) hipLaunchKernelGGL((mcseg_fwd_kernel<C_, E_>), dim3(gx, N), dim3(256), 0, (hipStream_t)s, z, y, HW, weight, partial);
  MC_DISPATCH(C, vec, MC_FWD)
#undef MC_FWD
  MI355_LAUNCH_CHECK();
  if (gx > 1) {
    hipLaunchKernelGGL(mcseg_fold_kernel, dim3(N), dim3(256), 0, (hipStream_t)s, partial, C, gx);
    MI355_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mcseg_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partial, N, C, gx, ce_weight, dice_weight, smooth,
                     per_sample ? 1 : 0, include_background ? 1 : 0, state, loss);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_mcseg_loss_bwd(const float* z, const uint8_t* y, int N, int C, long long HW, const float* weight,
                                    int ignore_index, float ce_weight, float dice_weight, const double* state,
                                    const float* gscale, float* dz, mi355_stream_t s) {
  MI355_CHECK_ARG(z && y && state && dz, "mcseg_loss_bwd: null pointer");
  if (int rc = mc_check_shape("mcseg_loss_bwd", N, C, HW, ignore_index)) return rc;
  MI355_CHECK_ARG(ce_weight >= 0.f && dice_weight >= 0.f, "mcseg_loss_bwd: ce_weight and dice_weight must not be negative (%g, %g)",
                  (double)ce_weight, (double)dice_weight);
  MI355_CHECK_ARG(mc_aligned(z, 4) && mc_aligned(dz, 4) && mc_aligned(state, 8),
                  "mcseg_loss_bwd: z and dz must be 4-byte, state 8-byte aligned");
  const int gx = mc_gx(N, HW);
  const bool vec = HW % 4 == 0 && mc_aligned(z, 16) && mc_aligned(y, 4) && mc_aligned(dz, 16);
#define MC_BWD(C_, E_)                                                                                                          \
  hipLaunchKernelGGL((mcseg_bwd_kernel<C_, E_>), dim3(gx, N), dim3(256), 0, (hipStream_t)s, z, y, HW, weight, ce_weight, dice_weight, \
                     state, gscale, dz);
  MC_DISPATCH(C, vec, MC_BWD)
#undef MC_BWD
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_mcseg_confusion(const float* z, const uint8_t* y, int N, int C, long long HW, int ignore_index, int32_t* conf,
                                     uint8_t* pred, mi355_stream_t s) {
  MI355_CHECK_ARG(z && y && conf, "mcseg_confusion: null pointer");
  if (int rc = mc_check_shape("mcseg_confusion", N, C, HW, ignore_index)) return rc;
  MI355_CHECK_ARG(mc_aligned(z, 4) && mc_aligned(conf, 4), "mcseg_confusion: z and conf must be 4-byte aligned");
  const int gx = mc_gx(N, HW);
  const bool vec = HW % 4 == 0 && mc_aligned(z, 16) && mc_aligned(y, 4) && (!pred || mc_aligned(pred, 4));
  hipError_t e = hipMemsetAsync(conf, 0, (size_t)N * C * C * sizeof(int32_t), (hipStream_t)s);
  if (e != hipSuccess) MI355_FAIL((int)e, "mcseg_confusion: clearing conf failed: %s", hipGetErrorString(e));
#define MC_CONF(C_, E_) hipLaunchKernelGGL((mcseg_confusion_kernel<C_, E_>), dim3(gx, N), dim3(256), 0, (hipStream_t)s, z, y, HW, conf, pred);
  MC_DISPATCH(C, vec, MC_CONF)
#undef MC_CONF
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
