// Dice / BCE + Dice segmentation loss on [B][per] fp32 logits and targets (the reference's DiceLoss / CombinedLoss,
// utils/clip_seg_finetuner.py:40-74, plus a per-image Dice mode).  With p = sigmoid(z), I = sum p t, P = sum p, T = sum t,
// D = P + T + smooth, num = 2 I + smooth:
//
//   loss  = bce_weight * mean(BCEWithLogits(z, t)) + dice_weight * (1 - num / D)
//   dz_i  = gs * (bce_weight (p_i - t_i) / n  -  (a t_i - c) p_i (1 - p_i)),   a = dice_weight 2 / D,  c = dice_weight num / D^2
//
// Two streaming passes over z and t, no more: the forward leaves one partial row (BCE, p t, p, t) per workgroup and SAMPLE, a
// one-workgroup finalize folds the rows in a fixed order in double and leaves loss[0] and one (a_b, c_b) pair per sample in
// `state` (batch mode: every sample gets the same pair; per-sample mode: each image's own sums, 1 / B folded in), the backward
// reads the pairs and the device-side gradient scale and writes dz — it never recomputes the loss.  No floating-point atomics
// anywhere: loss and gradient are bit-identical from run to run.  Nothing is allocated, nothing synchronises, every scalar the
// backward needs lives in device memory, so a launch plan or a captured graph can replay the three launches.
#include "rowred.hpp"

template <int E> struct alignas(4 * E) SegVec { float v[E]; };

// e = exp(-|x|) never overflows; s = 1 / (1 + e) in (0.5, 1]; sigmoid(x) = s (x >= 0) or e s (x < 0); p (1 - p) = e s^2 for both
// signs.  |x| = 100 gives e = 0: p is exactly 0 or 1, the BCE term max(x, 0) - x t + log1p(e) stays finite.
__device__ __forceinline__ void seg_sigmoid(float x, float& e, float& s, float& p) {
  e = __expf(-fabsf(x));
  s = __builtin_amdgcn_rcpf(1.f + e);
  p = x >= 0.f ? s : e * s;
}

template <int E>
__device__ __forceinline__ void seg_fwd_terms(const SegVec<E>& a, const SegVec<E>& y, float (&acc)[4][E]) {
#pragma unroll
  for (int k = 0; k < E; ++k) {
    float e, s, p;
    seg_sigmoid(a.v[k], e, s, p);
    acc[0][k] += fmaxf(a.v[k], 0.f) - a.v[k] * y.v[k] + log1pf(e);
    acc[1][k] += p * y.v[k];
    acc[2][k] += p;
    acc[3][k] += y.v[k];
  }
}

// grid (gx, B): workgroup (g, b) strides over sample b's vectors; four vectors of z and four of t in flight per thread
// (unconditional loads; the rows behind the last whole trip go through the one-vector loop).
// partial[(b * gx + g) * 4 + {0, 1, 2, 3}] = the workgroup's sums of BCE, p t, p, t.
template <int E>
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const float* __restrict__ z, const float* __restrict__ t, long long per,
                                                           float* __restrict__ partial) {
  typedef SegVec<E> V;
  const int b = blockIdx.y;
  const V* __restrict__ zv = reinterpret_cast<const V*>(z + (size_t)b * per);
  const V* __restrict__ tv = reinterpret_cast<const V*>(t + (size_t)b * per);
  const long long nv = per / E;
  const long long st = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  float acc[4][E];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int k = 0; k < E; ++k) acc[q][k] = 0.f;
  for (; i + 3 * st < nv; i += 4 * st) {
    V a[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = zv[i + k * st];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = tv[i + k * st];
#pragma unroll
    for (int k = 0; k < 4; ++k) seg_fwd_terms<E>(a[k], y[k], acc);
  }
  for (; i < nv; i += st) seg_fwd_terms<E>(zv[i], tv[i], acc);
  // thread -> wave -> workgroup, in double, always in the same order
  __shared__ double red[4][4];
  double d[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) v += (double)acc[q][k];
    d[q] = wave_sum_d(v);
  }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int q = 0; q < 4; ++q) red[threadIdx.x >> 6][q] = d[q];
  __syncthreads();
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    partial[((size_t)b * gridDim.x + blockIdx.x) * 4 + q] = (float)((red[0][q] + red[1][q]) + (red[2][q] + red[3][q]));
  }
}

// One workgroup.  Wave w folds the rows of samples w, w + 4, ... (lanes stride over a sample's gx rows, then the shuffle tree), the
// four waves' totals meet in LDS and are added in wave order.
__global__ __launch_bounds__(256) void seg_loss_finalize_kernel(const float* __restrict__ partial, int B, int gx, long long per,
                                                                float bce_weight, float dice_weight, float smooth, int per_sample,
                                                                float* __restrict__ state, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double bw = bce_weight, dw = dice_weight, sm = smooth;
  double bce = 0, dice = 0, I = 0, P = 0, T = 0;
  for (int b = wave; b < B; b += 4) {
    double q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    for (int g = lane; g < gx; g += 64) {
      const f32x4 r = *reinterpret_cast<const f32x4*>(partial + ((size_t)b * gx + g) * 4);
      q0 += (double)r[0];
      q1 += (double)r[1];
      q2 += (double)r[2];
      q3 += (double)r[3];
    }
    q0 = wave_sum_d(q0);
    q1 = wave_sum_d(q1);
    q2 = wave_sum_d(q2);
    q3 = wave_sum_d(q3);
    bce += q0;
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
  __shared__ double red[4][5];
  if (lane == 0) {
    red[wave][0] = bce;
    red[wave][1] = dice;
    red[wave][2] = I;
    red[wave][3] = P;
    red[wave][4] = T;
  }
  __syncthreads();
  double tot[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) tot[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
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
  if (threadIdx.x == 0) loss[0] = (float)(bw * tot[0] / ((double)B * (double)per) + dw * dice_loss);
}

template <int E>
__device__ __forceinline__ SegVec<E> seg_bwd_terms(const SegVec<E>& x, const SegVec<E>& y, float bwn, float a, float c, float gs) {
  SegVec<E> o;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    float e, s, p;
    seg_sigmoid(x.v[k], e, s, p);
    // p - t without cancellation where the logit is saturated: on the side where p rounds to 1, p - t = (1 - t) - e s
    // (exact for t = 1, where p - t in fp32 would be 0 instead of -e); p (1 - p) = (e s) s on both sides
    const float q = e * s;
    const float d = x.v[k] >= 0.f ? (1.f - y.v[k]) - q : q - y.v[k];
    o.v[k] = gs * (bwn * d - (a * y.v[k] - c) * (q * s));
  }
  return o;
}

// grid (gx, B), the forward's sweep: dz = gscale[0] * (bwn (p - t) - (a_b t - c_b) p (1 - p)), bwn = bce_weight / n.
template <int E>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t, long long per,
                                                           float bwn, const float* __restrict__ state,
                                                           const float* __restrict__ gscale, float* __restrict__ dz) {
  typedef SegVec<E> V;
  const int b = blockIdx.y;
  const V* __restrict__ zv = reinterpret_cast<const V*>(z + (size_t)b * per);
  const V* __restrict__ tv = reinterpret_cast<const V*>(t + (size_t)b * per);
  V* __restrict__ dv = reinterpret_cast<V*>(dz + (size_t)b * per);
  const float a = state[2 * b], c = state[2 * b + 1];
  const float gs = gscale ? gscale[0] : 1.f;
  const long long nv = per / E;
  const long long st = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * st < nv; i += 4 * st) {
    V x[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = zv[i + k * st];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = tv[i + k * st];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // (left alone, the scheduler sinks the last pair of loads behind the first pair's full wait: rowred.hpp, has_pin)
      if constexpr (E == 4) {
        pin16(x[k]);
        pin16(y[k]);
      }
      dv[i + k * st] = seg_bwd_terms<E>(x[k], y[k], bwn, a, c, gs);
    }
  }
  for (; i < nv; i += st) dv[i] = seg_bwd_terms<E>(zv[i], tv[i], bwn, a, c, gs);
}

// Workgroups per sample: one trip of the four-vector loop per thread where the sample is large enough, at most ~1024 workgroups
// in all (four per CU) and at most 256 per sample.  A function of (B, per) alone: forward, finalize and backward agree on it.
static int seg_loss_gx(int B, long long per) {
  long long gx = per / (4 * 256 * 4);
  const long long cap = 1024 / B;
  if (gx > cap) gx = cap;
  if (gx > 256) gx = 256;
  return (int)(gx < 1 ? 1 : gx);
}

#define SEG_LOSS_MAX_B 65535      /* the sample index is the grid's y coordinate */

extern "C" int mi355_seg_loss_rows(int B, long long per) {
  MI355_CHECK_ARG(B > 0 && B <= SEG_LOSS_MAX_B && per > 0, "seg_loss_rows: 0 < B <= %d and per > 0 expected (B=%d, per=%lld)",
                  SEG_LOSS_MAX_B, B, per);
  return B * seg_loss_gx(B, per);
}

static bool seg_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

extern "C" int mi355_seg_loss_fwd(const float* z, const float* t, int B, long long per, float bce_weight, float dice_weight,
                                  float smooth, int per_sample, float* partial, float* state, float* loss, mi355_stream_t s) {
  MI355_CHECK_ARG(z && t && partial && state && loss, "seg_loss_fwd: null pointer");
  MI355_CHECK_ARG(B > 0 && B <= SEG_LOSS_MAX_B && per > 0, "seg_loss_fwd: 0 < B <= %d and per > 0 expected (B=%d, per=%lld)",
                  SEG_LOSS_MAX_B, B, per);
  MI355_CHECK_ARG(bce_weight >= 0.f && dice_weight >= 0.f && smooth >= 0.f,
                  "seg_loss_fwd: bce_weight, dice_weight and smooth must not be negative (%g, %g, %g)", (double)bce_weight,
                  (double)dice_weight, (double)smooth);
  MI355_CHECK_ARG(seg_aligned16(partial), "seg_loss_fwd: partial must be 16-byte aligned");
  const int gx = seg_loss_gx(B, per);
  if (per % 4 == 0 && seg_aligned16(z) && seg_aligned16(t))
    hipLaunchKernelGGL((seg_loss_fwd_kernel<4>), dim3(gx, B), dim3(256), 0, (hipStream_t)s, z, t, per, partial);
  else
    hipLaunchKernelGGL((seg_loss_fwd_kernel<1>), dim3(gx, B), dim3(256), 0, (hipStream_t)s, z, t, per, partial);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partial, B, gx, per, bce_weight, dice_weight,
                     smooth, per_sample ? 1 : 0, state, loss);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_seg_loss_bwd(const float* z, const float* t, int B, long long per, float bce_weight, const float* state,
                                  const float* gscale, float* dz, mi355_stream_t s) {
  MI355_CHECK_ARG(z && t && state && dz, "seg_loss_bwd: null pointer");
  MI355_CHECK_ARG(B > 0 && B <= SEG_LOSS_MAX_B && per > 0, "seg_loss_bwd: 0 < B <= %d and per > 0 expected (B=%d, per=%lld)",
                  SEG_LOSS_MAX_B, B, per);
  MI355_CHECK_ARG(bce_weight >= 0.f, "seg_loss_bwd: bce_weight must not be negative (%g)", (double)bce_weight);
  const int gx = seg_loss_gx(B, per);
  const float bwn = (float)((double)bce_weight / ((double)B * (double)per));
  if (per % 4 == 0 && seg_aligned16(z) && seg_aligned16(t) && seg_aligned16(dz))
    hipLaunchKernelGGL((seg_loss_bwd_kernel<4>), dim3(gx, B), dim3(256), 0, (hipStream_t)s, z, t, per, bwn, state, gscale, dz);
  else
    hipLaunchKernelGGL((seg_loss_bwd_kernel<1>), dim3(gx, B), dim3(256), 0, (hipStream_t)s, z, t, per, bwn, state, gscale, dz);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
