// Knowledge distillation (Hinton et al. 2015; nothing in the reference): the student's loss reads a third tensor, the logits v of a
// frozen teacher, next to its own logits z and the hard target t.
//
// Binary segmentation, [B][per] fp32, n = B per, a = z / T, b = v / T, p_T = sigmoid(a), q = sigmoid(b), p = sigmoid(z):
//
//   KD      = T^2 / n  sum_i KL(Bernoulli(q_i) || Bernoulli(p_T,i))
//   loss[0] = bce_weight mean(BCEWithLogits(z, t)) + dice_weight Dice(z, t) + kd_weight KD,   loss[1] = the two hard terms,  loss[2] = KD
//   dz_i    = gs (bce_weight (p_i - t_i) / n - (a_b t_i - c_b) p_i (1 - p_i) + kd_weight T (p_T,i - q_i) / n)
//
// The KL element is formed without a logarithm of a ratio: softplus(-a) - softplus(-b) + (1 - q)(a - b), which is
// BCEWithLogits(a, q) - BCEWithLogits(b, q).  Both sigmoids come from kd_sig below, so v == z gives an element and a gradient term of
// exactly 0.  The hard terms, their (a_b, c_b) pairs and the passes are those of the Dice loss (seg_loss.hip): a forward sweep that
// leaves one row (bce, p t, p, t, kd) per workgroup and sample, a one-workgroup finalize in double with a fixed fold order, a backward
// sweep that reads `state` and the device-side gradient scale.  No floating-point atomics, no allocation, no synchronisation:
// bit-reproducible, replayable from a launch plan or a captured graph.  kd_weight = 0 instantiates the sweeps without v.
#include "rowred.hpp"

template <int E> struct alignas(4 * E) KdVec { float v[E]; };

// e = exp(-|x|), s = 1 / (1 + e) = sigmoid(|x|), lo = e s = sigmoid(-|x|): sigmoid(x) = pos ? s : lo, 1 - sigmoid(x) = pos ? lo : s
struct KdSig {
  float e, s, lo;
  bool pos;
};

__device__ __forceinline__ KdSig kd_sig(float x) {
#pragma clang fp contract(off)
  KdSig r;
  r.e = __expf(-fabsf(x));
  r.s = __builtin_amdgcn_rcpf(1.f + r.e);
  r.lo = r.e * r.s;
  r.pos = x >= 0.f;
  return r;
}

// sigmoid(a) - sigmoid(b) without cancellation against 1: on the same side of 0 the difference of the two small tails
__device__ __forceinline__ float kd_sig_diff(const KdSig& a, const KdSig& b) {
#pragma clang fp contract(off)
  if (a.pos == b.pos) return a.pos ? b.lo - a.lo : a.lo - b.lo;
  return a.pos ? a.s - b.lo : a.lo - b.s;
}

// (no FMA contraction in the element functions: the hard sums have the same bits with and without the teacher)
template <int E, bool KD>
__device__ __forceinline__ void kd_fwd_terms(const KdVec<E>& x, const KdVec<E>& y, const KdVec<E>& w, float inv_t, float (&acc)[5][E]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const KdSig r = kd_sig(x.v[k]);
    const float p = r.pos ? r.s : r.lo;
    acc[0][k] += fmaxf(x.v[k], 0.f) - x.v[k] * y.v[k] + log1pf(r.e);
    acc[1][k] += p * y.v[k];
    acc[2][k] += p;
    acc[3][k] += y.v[k];
    if constexpr (KD) {
      const float a = x.v[k] * inv_t, b = w.v[k] * inv_t;
      const KdSig ra = kd_sig(a), rb = kd_sig(b);
      const float spa = fmaxf(-a, 0.f) + log1pf(ra.e), spb = fmaxf(-b, 0.f) + log1pf(rb.e);
      acc[4][k] += (spa - spb) + (rb.pos ? rb.lo : rb.s) * (a - b);
    }
  }
}

// grid (gx, B): workgroup (g, b) strides over sample b's vectors; four vectors of every operand in flight per thread, the vectors
// behind the last whole trip go through the one-vector loop.  partial[(b * gx + g) * 8 + {0 .. 4}] = sums of bce, p t, p, t, kd.
template <int E, bool KD>
__global__ __launch_bounds__(256) void kd_seg_fwd_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                         const float* __restrict__ v, long long per, float inv_t,
                                                         float* __restrict__ partial) {
  typedef KdVec<E> V;
  const int b = blockIdx.y;
  const V* __restrict__ zv = reinterpret_cast<const V*>(z + (size_t)b * per);
  const V* __restrict__ tv = reinterpret_cast<const V*>(t + (size_t)b * per);
  const V* __restrict__ vv = reinterpret_cast<const V*>(KD ? v + (size_t)b * per : z);
  const long long nv = per / E;
  const long long st = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  float acc[5][E];
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int k = 0; k < E; ++k) acc[q][k] = 0.f;
  for (; i + 3 * st < nv; i += 4 * st) {
    V x[4], y[4], w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = zv[i + k * st];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = tv[i + k * st];
    if constexpr (KD) {
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = vv[i + k * st];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) kd_fwd_terms<E, KD>(x[k], y[k], KD ? w[k] : x[k], inv_t, acc);
  }
  for (; i < nv; i += st) {
    const V x = zv[i], y = tv[i];
    kd_fwd_terms<E, KD>(x, y, KD ? vv[i] : x, inv_t, acc);
  }
  // thread -> wave -> workgroup, in double, always in the same order
  __shared__ double red[4][5];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    double d = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) d += (double)acc[q][k];
    d = wave_sum_d(d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = d;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int q = threadIdx.x;
    partial[((size_t)b * gridDim.x + blockIdx.x) * 8 + q] =
        q < 5 ? (float)((red[0][q] + red[1][q]) + (red[2][q] + red[3][q])) : 0.f;
  }
}

// One workgroup.  Wave w folds the rows of samples w, w + 4, ... (lanes stride over a sample's gx rows, then the shuffle tree), the
// four waves' totals meet in LDS and are added in wave order.
__global__ __launch_bounds__(256) void kd_seg_finalize_kernel(const float* __restrict__ partial, int B, int gx, long long per,
                                                              float bce_weight, float dice_weight, float smooth, int per_sample,
                                                              float kd_weight, float temperature, float* __restrict__ state,
                                                              float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double bw = bce_weight, dw = dice_weight, sm = smooth;
  double bce = 0, dice = 0, I = 0, P = 0, T = 0, kd = 0;
  for (int b = wave; b < B; b += 4) {
    double q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0;
    for (int g = lane; g < gx; g += 64) {
      const float* row = partial + ((size_t)b * gx + g) * 8;
      const f32x4 r = *reinterpret_cast<const f32x4*>(row);
      const f32x4 r2 = *reinterpret_cast<const f32x4*>(row + 4);
      q0 += (double)r[0];
      q1 += (double)r[1];
      q2 += (double)r[2];
      q3 += (double)r[3];
      q4 += (double)r2[0];
    }
    q0 = wave_sum_d(q0);
    q1 = wave_sum_d(q1);
    q2 = wave_sum_d(q2);
    q3 = wave_sum_d(q3);
    q4 = wave_sum_d(q4);
    bce += q0;
    kd += q4;
    if (per_sample) {
      const double D = q2 + q3 + sm, num = 2.0 * q1 + sm;
      dice += 1.0 - num / D;
      if (lane == 0) {
        state[2 * b] = (float)(dw * 2.0 / (D * (double)B));
        state[2 * b + 1] = (float)(dw * num / (D * D * (double)B));
      }
    } else {
      I += q1;
      P += q2;
      T += q3;
    }
  }
  __shared__ double red[4][6];
  if (lane == 0) {
    red[wave][0] = bce;
    red[wave][1] = dice;
    red[wave][2] = I;
    red[wave][3] = P;
    red[wave][4] = T;
    red[wave][5] = kd;
  }
  __syncthreads();
  double tot[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) tot[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  double dice_loss;
  if (per_sample) {
    dice_loss = tot[1] / (double)B;
  } else {
    const double D = tot[3] + tot[4] + sm, num = 2.0 * tot[2] + sm;
    dice_loss = 1.0 - num / D;
    const float a = (float)(dw * 2.0 / D), c = (float)(dw * num / (D * D));
    for (int b = threadIdx.x; b < B; b += 256) {
      state[2 * b] = a;
      state[2 * b + 1] = c;
    }
  }
  if (threadIdx.x == 0) {
    const double n = (double)B * (double)per, tt = (double)temperature;
    const double hard = bw * tot[0] / n + dw * dice_loss, kdl = tt * tt * tot[5] / n;
    loss[0] = (float)(hard + (double)kd_weight * kdl);
    loss[1] = (float)hard;
    loss[2] = (float)kdl;
  }
}

// bwn = bce_weight / n, kdn = kd_weight T / n.  Every operation is rounded on its own (no FMA contraction here or in kd_sig), so that
// the hard part has the same bits with and without the teacher and a KD part of exactly 0 (v == z) leaves them alone.
template <int E, bool KD>
__device__ __forceinline__ KdVec<E> kd_bwd_terms(const KdVec<E>& x, const KdVec<E>& y, const KdVec<E>& w, float bwn, float a, float c,
                                                 float kdn, float inv_t, float gs) {
#pragma clang fp contract(off)
  KdVec<E> o;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const KdSig r = kd_sig(x.v[k]);
    // p - t on the side where p rounds to 1 is (1 - t) - e s (seg_loss.hip); p (1 - p) = (e s) s on both sides
    const float d = r.pos ? (1.f - y.v[k]) - r.lo : r.lo - y.v[k];
    float g = __fsub_rn(__fmul_rn(bwn, d), __fmul_rn(__fsub_rn(__fmul_rn(a, y.v[k]), c), __fmul_rn(r.lo, r.s)));
    if constexpr (KD) g = __fadd_rn(g, __fmul_rn(kdn, kd_sig_diff(kd_sig(x.v[k] * inv_t), kd_sig(w.v[k] * inv_t))));
    o.v[k] = __fmul_rn(gs, g);
  }
  return o;
}

// grid (gx, B), the forward's sweep
template <int E, bool KD>
__global__ __launch_bounds__(256) void kd_seg_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                         const float* __restrict__ v, long long per, float bwn, float kdn, float inv_t,
                                                         const float* __restrict__ state, const float* __restrict__ gscale,
                                                         float* __restrict__ dz) {
  typedef KdVec<E> V;
  const int b = blockIdx.y;
  const V* __restrict__ zv = reinterpret_cast<const V*>(z + (size_t)b * per);
  const V* __restrict__ tv = reinterpret_cast<const V*>(t + (size_t)b * per);
  const V* __restrict__ vv = reinterpret_cast<const V*>(KD ? v + (size_t)b * per : z);
  V* __restrict__ dv = reinterpret_cast<V*>(dz + (size_t)b * per);
  const float a = state[2 * b], c = state[2 * b + 1];
  const float gs = gscale ? gscale[0] : 1.f;
  const long long nv = per / E;
  const long long st = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * st < nv; i += 4 * st) {
    V x[4], y[4], w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = zv[i + k * st];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = tv[i + k * st];
    if constexpr (KD) {
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = vv[i + k * st];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // (every load of the trip issued before the first store: rowred.hpp, has_pin)
      if constexpr (E == 4) {
        pin16(x[k]);
        pin16(y[k]);
        if constexpr (KD) pin16(w[k]);
      }
      dv[i + k * st] = kd_bwd_terms<E, KD>(x[k], y[k], KD ? w[k] : x[k], bwn, a, c, kdn, inv_t, gs);
    }
  }
  for (; i < nv; i += st) {
    const V x = zv[i], y = tv[i];
    dv[i] = kd_bwd_terms<E, KD>(x, y, KD ? vv[i] : x, bwn, a, c, kdn, inv_t, gs);
  }
}

#define KD_MAX_B 65535         /* the sample index is the grid's y coordinate */
#define KD_TRIP (4 * 256 * 4)  /* floats one workgroup covers in one trip of the four-vector loop */
#define KD_MAX_WGS 1024        /* four workgroups per CU */

// Workgroups per sample, a function of (B, per) alone (forward, finalize and backward agree on it): a whole trip per thread where the
// sample is long enough, within KD_MAX_WGS over the batch and 256 per sample.
static int kd_gx(int B, long long per) {
  const long long want = per / KD_TRIP, cap = KD_MAX_WGS / B < 256 ? KD_MAX_WGS / B : 256;
  const long long gx = want < cap ? want : cap;
  return (int)(gx < 1 ? 1 : gx);
}

static bool kd_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
static bool kd_finite(float x) { return x - x == 0.f; }

#define KD_CHECK_SHAPE(who)                                                                                                         \
  MI355_CHECK_ARG(B > 0 && B <= KD_MAX_B && per > 0, who ": 0 < B <= %d and per > 0 expected (B=%d, per=%lld)", KD_MAX_B, B, per)
#define KD_CHECK_T(who)                                                                                                             \
  MI355_CHECK_ARG(kd_finite(temperature) && temperature > 0.f && kd_finite(kd_weight) && kd_weight >= 0.f,                          \
                  who ": a finite temperature > 0 and a finite kd_weight >= 0 expected (%g, %g)", (double)temperature,               \
                  (double)kd_weight)

extern "C" int mi355_kd_seg_rows(int B, long long per) {
  KD_CHECK_SHAPE("kd_seg_rows");
  return B * kd_gx(B, per);
}

extern "C" int mi355_kd_seg_fwd(const float* z, const float* t, const float* v, int B, long long per, float bce_weight,
                                float dice_weight, float smooth, int per_sample, float kd_weight, float temperature, float* partial,
                                float* state, float* loss, mi355_stream_t s) {
  MI355_CHECK_ARG(z && t && partial && state && loss, "kd_seg_fwd: null pointer");
  KD_CHECK_SHAPE("kd_seg_fwd");
  MI355_CHECK_ARG(bce_weight >= 0.f && dice_weight >= 0.f && smooth >= 0.f,
                  "kd_seg_fwd: bce_weight, dice_weight and smooth must not be negative (%g, %g, %g)", (double)bce_weight,
                  (double)dice_weight, (double)smooth);
  KD_CHECK_T("kd_seg_fwd");
  MI355_CHECK_ARG(v || kd_weight == 0.f, "kd_seg_fwd: null pointer (teacher logits with kd_weight > 0)");
  MI355_CHECK_ARG(kd_aligned16(partial), "kd_seg_fwd: partial must be 16-byte aligned");
  const int gx = kd_gx(B, per);
  const dim3 grid(gx, B);
  const bool kd = kd_weight > 0.f;
  const bool vec = per % 4 == 0 && kd_aligned16(z) && kd_aligned16(t) && (!kd || kd_aligned16(v));
  const float inv_t = 1.f / temperature;
  if (kd) {
    if (vec)
      hipLaunchKernelGGL((kd_seg_fwd_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)s, z, t, v, per, inv_t, partial);
    else
      hipLaunchKernelGGL((kd_seg_fwd_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)s, z, t, v, per, inv_t, partial);
  } else {
    if (vec)
      hipLaunchKernelGGL((kd_seg_fwd_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)s, z, t, v, per, inv_t, partial);
    else
      hipLaunchKernelGGL((kd_seg_fwd_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)s, z, t, v, per, inv_t, partial);
  }
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(kd_seg_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partial, B, gx, per, bce_weight, dice_weight,
                     smooth, per_sample ? 1 : 0, kd_weight, temperature, state, loss);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_kd_seg_bwd(const float* z, const float* t, const float* v, int B, long long per, float bce_weight,
                                float kd_weight, float temperature, const float* state, const float* gscale, float* dz,
                                mi355_stream_t s) {
  MI355_CHECK_ARG(z && t && state && dz, "kd_seg_bwd: null pointer");
  KD_CHECK_SHAPE("kd_seg_bwd");
  MI355_CHECK_ARG(bce_weight >= 0.f, "kd_seg_bwd: bce_weight must not be negative (%g)", (double)bce_weight);
  KD_CHECK_T("kd_seg_bwd");
  MI355_CHECK_ARG(v || kd_weight == 0.f, "kd_seg_bwd: null pointer (teacher logits with kd_weight > 0)");
  const int gx = kd_gx(B, per);
  const dim3 grid(gx, B);
  const bool kd = kd_weight > 0.f;
  const bool vec = per % 4 == 0 && kd_aligned16(z) && kd_aligned16(t) && kd_aligned16(dz) && (!kd || kd_aligned16(v));
  const double n = (double)B * (double)per;
  const float bwn = (float)((double)bce_weight / n), kdn = (float)((double)kd_weight * (double)temperature / n);
  const float inv_t = 1.f / temperature;
  if (kd) {
    if (vec)
      hipLaunchKernelGGL((kd_seg_bwd_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)s, z, t, v, per, bwn, kdn, inv_t, state, gscale, dz);
    else
      hipLaunchKernelGGL((kd_seg_bwd_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)s, z, t, v, per, bwn, kdn, inv_t, state, gscale, dz);
  } else {
    if (vec)
      hipLaunchKernelGGL((kd_seg_bwd_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)s, z, t, v, per, bwn, kdn, inv_t, state, gscale, dz);
    else
      hipLaunchKernelGGL((kd_seg_bwd_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)s, z, t, v, per, bwn, kdn, inv_t, state, gscale, dz);
  }
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- classifiers: hard cross-entropy (mi355_ce_mix's hard-label case) + T^2 KL(softmax(v / T) || softmax(z / T)) ------------------------
// Everything in double (inputs and T widened, exp / log in double), rounded to float once on store; thread b % 256 owns row b, the
// block fold runs in a fixed order.  The KL row is sum_c q_c ((b_c - lse_b) - (a_c - lse_a)): v == z gives exactly 0.  Labels only
// select (c == label), never index.
__global__ __launch_bounds__(256) void ce_distill_kernel(const float* __restrict__ z, const int64_t* __restrict__ y,
                                                         const float* __restrict__ v, const float* __restrict__ weight,
                                                         float* __restrict__ loss, float* __restrict__ dz,
                                                         const float* __restrict__ gscale, int B, int C, float sm, float hard_weight,
                                                         float kd_weight, float temperature) {
  const double gs = (gscale ? (double)gscale[0] : 1.0) / (double)B;
  const double keep = 1.0 - (double)sm, uni = (double)sm / (double)C;
  const double hw = hard_weight, kw = kd_weight, T = temperature;
  const bool kd = kd_weight > 0.f;
  double acc_h = 0.0, acc_k = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* row = z + (size_t)b * C;
    const float* tea = kd ? v + (size_t)b * C : row;
    double mx = -INFINITY, ma = -INFINITY, mb = -INFINITY;
    for (int c = 0; c < C; ++c) {
      mx = fmax(mx, (double)row[c]);
      if (kd) {
        ma = fmax(ma, (double)row[c] / T);
        mb = fmax(mb, (double)tea[c] / T);
      }
    }
    double se = 0.0, sa = 0.0, sb = 0.0;
    for (int c = 0; c < C; ++c) {
      se += exp((double)row[c] - mx);
      if (kd) {
        sa += exp((double)row[c] / T - ma);
        sb += exp((double)tea[c] / T - mb);
      }
    }
    const double lse = mx + log(se), lsa = kd ? ma + log(sa) : 0.0, lsb = kd ? mb + log(sb) : 0.0;
    const int64_t lab = y[b];
    double wt_sum = 0.0, nll = 0.0, kl = 0.0;
    for (int c = 0; c < C; ++c) {
      const double wt = (weight ? (double)weight[c] : 1.0) * (keep * (c == lab ? 1.0 : 0.0) + uni);
      wt_sum += wt;
      nll += wt * (lse - (double)row[c]);
      if (kd) {
        const double lp = (double)row[c] / T - lsa, lq = (double)tea[c] / T - lsb;
        kl += exp(lq) * (lq - lp);
      }
    }
    acc_h += nll;
    acc_k += kl;
    if (dz)
      for (int c = 0; c < C; ++c) {
        const double wt = (weight ? (double)weight[c] : 1.0) * (keep * (c == lab ? 1.0 : 0.0) + uni);
        double g = hw * (exp((double)row[c] - lse) * wt_sum - wt);
        if (kd) g += kw * T * (exp((double)row[c] / T - lsa) - exp((double)tea[c] / T - lsb));
        dz[(size_t)b * C + c] = (float)(gs * g);
      }
  }
  __shared__ double red[4][2];
  acc_h = wave_sum_d(acc_h);
  acc_k = wave_sum_d(acc_k);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = acc_h;
    red[threadIdx.x >> 6][1] = acc_k;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double hard = (((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]) / (double)B;
    const double kdl = T * T * ((((red[0][1] + red[1][1]) + red[2][1]) + red[3][1]) / (double)B);
    loss[0] = (float)(hw * hard + kw * kdl);
    loss[1] = (float)hard;
    loss[2] = (float)kdl;
  }
}

extern "C" int mi355_ce_distill(const float* z, const int64_t* y, const float* v, const float* weight, float* loss, float* dz,
                                const float* gscale, int B, int C, float smoothing, float hard_weight, float kd_weight,
                                float temperature, mi355_stream_t s) {
  MI355_CHECK_ARG(z && y && loss, "ce_distill: null pointer");
  MI355_CHECK_ARG(B > 0 && C > 0, "ce_distill: B > 0 and C > 0 expected (B=%d, C=%d)", B, C);
  MI355_CHECK_ARG(kd_finite(hard_weight) && hard_weight >= 0.f && smoothing >= 0.f && smoothing <= 1.f,
                  "ce_distill: a finite hard_weight >= 0 and a smoothing in [0, 1] expected (%g, %g)", (double)hard_weight,
                  (double)smoothing);
  KD_CHECK_T("ce_distill");
  MI355_CHECK_ARG(v || kd_weight == 0.f, "ce_distill: null pointer (teacher logits with kd_weight > 0)");
  hipLaunchKernelGGL(ce_distill_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, z, y, v, weight, loss, dz, gscale, B, C, smoothing,
                     hard_weight, kd_weight, temperature);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
