// Focal + (focal-)Tversky loss on [B][per] fp32 logits and targets, and the focal cross-entropy of the classifiers (Lin et al. 2017 in
// torchvision's sigmoid_focal_loss convention; Salehi et al. 2017; Abraham & Khan 2019; nothing in the reference).  The target is
// binarised here, t = (target > 0.5).  With x = (2 t - 1) z the logit seen from the target's side:
//
//   p_t = sigmoid(x),  u = 1 - p_t = sigmoid(-x),  ce = softplus(-x),  log u = -softplus(x)
//   focal_i = alpha_t u^gamma ce            d focal_i / dz = alpha_t u^gamma (2 t - 1) (-gamma p_t ce - u)
//   TI = Num / Den, Num = I + smooth, Den = (1 - a - b) I + a P + b T + smooth      (I = sum p t, P = sum p, T = sum t)
//   loss = focal_weight mean(focal_i) + tversky_weight (1 - TI)^g
//   dz_i = gs (focal_weight / n d focal_i / dz - (A t - C (a + (1 - a - b) t)) p (1 - p)),  A = tversky_weight g (1 - TI)^(g-1) / Den,  C = A TI
//
// Everything per element comes from e = exp(-|z|) and L = log1p(e): with `agree` = (z >= 0) == t, sigmoid(|z|) = 1 / (1 + e) = s and
// sigmoid(-|z|) = e s, so u = agree ? e s : s, ce = (agree ? 0 : |z|) + L, softplus(x) = (agree ? |z| : 0) + L, and
// u^gamma = exp(-gamma softplus(x)): no 1 - p anywhere, no log of u, one exp more than BCE + Dice.  gamma = 0 gives exp(-0) = 1.
//
// The passes are those of the Dice loss (seg_loss.hip): a forward sweep that leaves one row (focal, p t, p, t) per workgroup and
// sample, a one-workgroup finalize in double with a fixed fold order that leaves loss[0] and (A_b, C_b) per sample in `state`, a
// backward sweep that reads `state` and the device-side gradient scale.  No floating-point atomics, no allocation, no
// synchronisation: bit-reproducible, replayable from a launch plan or a captured graph.
#include "rowred.hpp"

template <int E> struct alignas(4 * E) FtvVec { float v[E]; };

// what every term of one element is made of (header comment)
struct FtvElem {
  float q, s, az, L;      // e s, 1 / (1 + e), |z|, log1p(e)
  bool pos, tb, agree;
};

template <bool FOCAL>
__device__ __forceinline__ FtvElem ftv_elem(float z, float traw) {
  FtvElem r;
  r.az = fabsf(z);
  const float e = __expf(-r.az);
  r.s = __builtin_amdgcn_rcpf(1.f + e);
  r.q = e * r.s;
  r.L = FOCAL ? log1pf(e) : 0.f;
  r.pos = z >= 0.f;
  r.tb = traw > 0.5f;
  r.agree = r.pos == r.tb;
  return r;
}

// u^gamma = exp(-gamma softplus(x)), exactly 1 at gamma = 0 and exactly 0 at u = 0 with gamma > 0 (the accurate expf: its argument
// reaches gamma |z|, where the fast one's argument scaling alone would cost |arg| 2^-24 of relative error)
__device__ __forceinline__ float ftv_pow_u(const FtvElem& r, float u, float gamma) {
  const float sp = (r.agree ? r.az : 0.f) + r.L;
  const float w = expf(-gamma * sp);
  return (u == 0.f && gamma > 0.f) ? 0.f : w;
}

struct FtvFocal {
  float a1, a0, gamma;      // alpha_t for t = 1 / t = 0 (both 1 when alpha < 0), the focusing exponent
};

template <int E, bool FOCAL>
__device__ __forceinline__ void ftv_fwd_terms(const FtvVec<E>& a, const FtvVec<E>& y, const FtvFocal f, float (&acc)[4][E]) {
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const FtvElem r = ftv_elem<FOCAL>(a.v[k], y.v[k]);
    if constexpr (FOCAL) {
      const float u = r.agree ? r.q : r.s;
      const float ce = (r.agree ? 0.f : r.az) + r.L;
      acc[0][k] += (r.tb ? f.a1 : f.a0) * ftv_pow_u(r, u, f.gamma) * ce;
    }
    const float p = r.pos ? r.s : r.q;
    acc[1][k] += r.tb ? p : 0.f;
    acc[2][k] += p;
    acc[3][k] += r.tb ? 1.f : 0.f;
  }
}

// grid (gx, B): workgroup (g, b) strides over sample b's vectors, four vectors of z and four of t in flight per thread; the vectors
// behind the last whole trip go through the one-vector loop.  partial[(b * gx + g) * 4 + {0, 1, 2, 3}] = sums of focal, p t, p, t.
template <int E, bool FOCAL>
__global__ __launch_bounds__(256) void ftv_loss_fwd_kernel(const float* __restrict__ z, const float* __restrict__ t, long long per,
                                                           FtvFocal f, float* __restrict__ partial) {
  typedef FtvVec<E> V;
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
    for (int k = 0; k < 4; ++k) ftv_fwd_terms<E, FOCAL>(a[k], y[k], f, acc);
  }
  for (; i < nv; i += st) ftv_fwd_terms<E, FOCAL>(zv[i], tv[i], f, acc);
  // thread -> wave -> workgroup, in double, always in the same order
  __shared__ double red[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) v += (double)acc[q][k];
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    partial[((size_t)b * gridDim.x + blockIdx.x) * 4 + q] = (float)((red[0][q] + red[1][q]) + (red[2][q] + red[3][q]));
  }
}

struct FtvTversky {
  double w, a, b, g, smooth;
};

// (1 - TI)^g and the pair (A, C) of one set of sums; `div`: B in per-sample mode.  1 - TI = (a FP + b FN) / Den is formed from the
// false counts, not as 1 - Num / Den; at 1 - TI <= 0 (or Den = 0) the term and its sub-gradient are 0.
__device__ __forceinline__ double ftv_tversky(const FtvTversky k, double I, double P, double T, double div, float& A, float& C) {
  const double num = I + k.smooth, den = I + k.a * (P - I) + k.b * (T - I) + k.smooth;
  const double ome = den > 0 ? (k.a * (P - I) + k.b * (T - I)) / den : 0.0;
  if (!(ome > 0)) {
    A = 0.f;
    C = 0.f;
    return 0.0;
  }
  const double Ad = k.w * k.g * (k.g == 1.0 ? 1.0 : pow(ome, k.g - 1.0)) / (den * div);
  A = (float)Ad;
  C = (float)(Ad * num / den);
  return k.g == 1.0 ? ome : pow(ome, k.g);
}

// One workgroup.  Wave w folds the rows of samples w, w + 4, ... (lanes stride over a sample's gx rows, then the shuffle tree); the
// four waves' totals meet in LDS and are added in wave order.
__global__ __launch_bounds__(256) void ftv_loss_finalize_kernel(const float* __restrict__ partial, int B, int gx, long long per,
                                                                float focal_weight, FtvTversky k, int per_sample,
                                                                float* __restrict__ state, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double foc = 0, tvs = 0, I = 0, P = 0, T = 0;
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
    foc += q0;
    if (per_sample) {
      float A, C;
      tvs += ftv_tversky(k, q1, q2, q3, (double)B, A, C);
      if (lane == 0) {
        state[2 * b] = A;
        state[2 * b + 1] = C;
      }
    } else {
      I += q1;
      P += q2;
      T += q3;
    }
  }
  __shared__ double red[4][5];
  if (lane == 0) {
    red[wave][0] = foc;
    red[wave][1] = tvs;
    red[wave][2] = I;
    red[wave][3] = P;
    red[wave][4] = T;
  }
  __syncthreads();
  double tot[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) tot[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  double tv_loss;
  if (per_sample) {
    tv_loss = tot[1] / (double)B;
  } else {
    float A, C;
    tv_loss = ftv_tversky(k, tot[2], tot[3], tot[4], 1.0, A, C);
    for (int b = threadIdx.x; b < B; b += 256) {
      state[2 * b] = A;
      state[2 * b + 1] = C;
    }
  }
  if (threadIdx.x == 0) loss[0] = (float)((double)focal_weight * tot[0] / ((double)B * (double)per) + k.w * tv_loss);
}

// fwn = focal_weight / n; k1 = A - C (1 - b), k0 = -C a: the Tversky coefficient of an element with t = 1 / t = 0
template <int E, bool FOCAL>
__device__ __forceinline__ FtvVec<E> ftv_bwd_terms(const FtvVec<E>& x, const FtvVec<E>& y, const FtvFocal f, float fwn, float k1,
                                                   float k0, float gs) {
  FtvVec<E> o;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const FtvElem r = ftv_elem<FOCAL>(x.v[k], y.v[k]);
    float d = -(r.tb ? k1 : k0) * (r.q * r.s);      // p (1 - p) = (e s) s on both sides
    if constexpr (FOCAL) {
      const float u = r.agree ? r.q : r.s, pt = r.agree ? r.s : r.q;
      const float ce = (r.agree ? 0.f : r.az) + r.L;
      const float fa = fwn * (r.tb ? f.a1 : -f.a0);      // focal_weight / n * alpha_t * (2 t - 1)
      d += fa * ftv_pow_u(r, u, f.gamma) * (-f.gamma * pt * ce - u);
    }
    o.v[k] = gs * d;
  }
  return o;
}

// grid (gx, B), the forward's sweep
template <int E, bool FOCAL>
__global__ __launch_bounds__(256) void ftv_loss_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t, long long per,
                                                           FtvFocal f, float fwn, float tv_a, float tv_b,
                                                           const float* __restrict__ state, const float* __restrict__ gscale,
                                                           float* __restrict__ dz) {
  typedef FtvVec<E> V;
  const int b = blockIdx.y;
  const V* __restrict__ zv = reinterpret_cast<const V*>(z + (size_t)b * per);
  const V* __restrict__ tv = reinterpret_cast<const V*>(t + (size_t)b * per);
  V* __restrict__ dv = reinterpret_cast<V*>(dz + (size_t)b * per);
  const float A = state[2 * b], C = state[2 * b + 1];
  const float k1 = A - C * (1.f - tv_b), k0 = -C * tv_a;
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
      // (all eight loads issued before the first store: rowred.hpp, has_pin)
      if constexpr (E == 4) {
        pin16(x[k]);
        pin16(y[k]);
      }
      dv[i + k * st] = ftv_bwd_terms<E, FOCAL>(x[k], y[k], f, fwn, k1, k0, gs);
    }
  }
  for (; i < nv; i += st) dv[i] = ftv_bwd_terms<E, FOCAL>(zv[i], tv[i], f, fwn, k1, k0, gs);
}

#define FTV_MAX_B 65535      /* the sample index is the grid's y coordinate */
#define FTV_TRIP (4 * 256 * 4) /* floats one workgroup covers in one trip of the four-vector loop */
#define FTV_MAX_WGS 1024     /* four workgroups per CU */

// Workgroups per sample, a function of (B, per) alone (forward, finalize and backward agree on it): a whole trip per thread where the
// sample is long enough, within FTV_MAX_WGS over the batch and 256 per sample.
static int ftv_gx(int B, long long per) {
  const long long want = per / FTV_TRIP, cap = FTV_MAX_WGS / B < 256 ? FTV_MAX_WGS / B : 256;
  const long long gx = want < cap ? want : cap;
  return (int)(gx < 1 ? 1 : gx);
}

static bool ftv_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

static FtvFocal ftv_focal(float alpha, float gamma) {
  FtvFocal f;
  f.a1 = alpha < 0.f ? 1.f : alpha;
  f.a0 = alpha < 0.f ? 1.f : 1.f - alpha;
  f.gamma = gamma;
  return f;
}

#define FTV_CHECK_SHAPE(who)                                                                                                        \
  MI355_CHECK_ARG(B > 0 && B <= FTV_MAX_B && per > 0, who ": 0 < B <= %d and per > 0 expected (B=%d, per=%lld)", FTV_MAX_B, B, per)
#define FTV_CHECK_FOCAL(who)                                                                                                        \
  MI355_CHECK_ARG(focal_weight >= 0.f && focal_gamma >= 0.f && focal_alpha <= 1.f,                                                  \
                  who ": focal_weight >= 0, focal_gamma >= 0 and focal_alpha <= 1 expected (%g, %g, %g)", (double)focal_weight,      \
                  (double)focal_gamma, (double)focal_alpha)
#define FTV_CHECK_AB(who)                                                                                                           \
  MI355_CHECK_ARG(tv_a >= 0.f && tv_b >= 0.f && tv_a + tv_b > 0.f, who ": tv_a, tv_b >= 0 with tv_a + tv_b > 0 expected (%g, %g)",  \
                  (double)tv_a, (double)tv_b)

extern "C" int mi355_ftv_loss_rows(int B, long long per) {
  FTV_CHECK_SHAPE("ftv_loss_rows");
  return B * ftv_gx(B, per);
}

extern "C" int mi355_ftv_loss_fwd(const float* z, const float* t, int B, long long per, float focal_weight, float focal_alpha,
                                  float focal_gamma, float tversky_weight, float tv_a, float tv_b, float tv_exp, float smooth,
                                  int per_sample, float* partial, float* state, float* loss, mi355_stream_t s) {
  MI355_CHECK_ARG(z && t && partial && state && loss, "ftv_loss_fwd: null pointer");
  FTV_CHECK_SHAPE("ftv_loss_fwd");
  FTV_CHECK_FOCAL("ftv_loss_fwd");
  FTV_CHECK_AB("ftv_loss_fwd");
  MI355_CHECK_ARG(tversky_weight >= 0.f && smooth >= 0.f && tv_exp > 0.f,
                  "ftv_loss_fwd: tversky_weight >= 0, smooth >= 0 and tv_exp > 0 expected (%g, %g, %g)", (double)tversky_weight,
                  (double)smooth, (double)tv_exp);
  MI355_CHECK_ARG(ftv_aligned16(partial), "ftv_loss_fwd: partial must be 16-byte aligned");
  const int gx = ftv_gx(B, per);
  const dim3 grid(gx, B);
  const bool vec = per % 4 == 0 && ftv_aligned16(z) && ftv_aligned16(t);
  const FtvFocal f = ftv_focal(focal_alpha, focal_gamma);
  // focal_weight = 0 (the Tversky losses): the sweep leaves the log and the second exp out, column 0 of `partial` is 0
  if (focal_weight > 0.f) {
    if (vec)
      hipLaunchKernelGGL((ftv_loss_fwd_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)s, z, t, per, f, partial);
    else
      hipLaunchKernelGGL((ftv_loss_fwd_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)s, z, t, per, f, partial);
  } else {
    if (vec)
      hipLaunchKernelGGL((ftv_loss_fwd_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)s, z, t, per, f, partial);
    else
      hipLaunchKernelGGL((ftv_loss_fwd_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)s, z, t, per, f, partial);
  }
  MI355_LAUNCH_CHECK();
  FtvTversky k;
  k.w = tversky_weight;
  k.a = tv_a;
  k.b = tv_b;
  k.g = tv_exp;
  k.smooth = smooth;
  hipLaunchKernelGGL(ftv_loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partial, B, gx, per, focal_weight, k,
                     per_sample ? 1 : 0, state, loss);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_ftv_loss_bwd(const float* z, const float* t, int B, long long per, float focal_weight, float focal_alpha,
                                  float focal_gamma, float tv_a, float tv_b, const float* state, const float* gscale, float* dz,
                                  mi355_stream_t s) {
  MI355_CHECK_ARG(z && t && state && dz, "ftv_loss_bwd: null pointer");
  FTV_CHECK_SHAPE("ftv_loss_bwd");
  FTV_CHECK_FOCAL("ftv_loss_bwd");
  FTV_CHECK_AB("ftv_loss_bwd");
  const int gx = ftv_gx(B, per);
  const dim3 grid(gx, B);
  const bool vec = per % 4 == 0 && ftv_aligned16(z) && ftv_aligned16(t) && ftv_aligned16(dz);
  const FtvFocal f = ftv_focal(focal_alpha, focal_gamma);
  const float fwn = (float)((double)focal_weight / ((double)B * (double)per));
  if (focal_weight > 0.f) {
    if (vec)
      hipLaunchKernelGGL((ftv_loss_bwd_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)s, z, t, per, f, fwn, tv_a, tv_b, state, gscale, dz);
    else
      hipLaunchKernelGGL((ftv_loss_bwd_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)s, z, t, per, f, fwn, tv_a, tv_b, state, gscale, dz);
  } else {
    if (vec)
      hipLaunchKernelGGL((ftv_loss_bwd_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)s, z, t, per, f, fwn, tv_a, tv_b, state, gscale, dz);
    else
      hipLaunchKernelGGL((ftv_loss_bwd_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)s, z, t, per, f, fwn, tv_a, tv_b, state, gscale, dz);
  }
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- focal cross-entropy of the classifiers -------------------------------------------------------------------------------------------
// Everything in double, rounded to float once on store; thread b % 256 owns row b, the block fold runs in a fixed order.  With
// u = sum_{c != y} p_c and G = u^gamma (gamma py log py - u):  dz_y = gs w G  and  dz_c = -gs w r_c G for c != y, where
// r_c = p_c / u is formed as the softmax over the classes other than y: nothing divides by u, u = 0 gives G = 0 (gamma > 0).
__global__ __launch_bounds__(256) void ce_focal_kernel(const float* __restrict__ z, const int64_t* __restrict__ y,
                                                       const float* __restrict__ weight, float* __restrict__ loss, float* __restrict__ dz,
                                                       const float* __restrict__ gscale, int B, int C, float gamma_f) {
  const double gs = (gscale ? (double)gscale[0] : 1.0) / (double)B;
  const double gamma = gamma_f;
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* row = z + (size_t)b * C;
    const int64_t lab = y[b];
    if (lab < 0 || lab >= C) {
      if (dz)
        for (int c = 0; c < C; ++c) dz[(size_t)b * C + c] = 0.f;
      continue;
    }
    double mx = -INFINITY, mo = -INFINITY;      // maximum over all classes / over the classes other than y
    for (int c = 0; c < C; ++c) {
      mx = fmax(mx, (double)row[c]);
      if (c != lab) mo = fmax(mo, (double)row[c]);
    }
    double se = 0.0, so = 0.0;
    for (int c = 0; c < C; ++c) {
      se += exp((double)row[c] - mx);
      if (c != lab) so += exp((double)row[c] - mo);
    }
    const double lse = mx + log(se);
    const double logpy = (double)row[lab] - lse, py = exp(logpy);
    const double u = so > 0.0 ? so * exp(mo - lse) : 0.0;      // sum_{c != y} exp(z_c - lse), the common factor taken out (C = 1: 0)
    const double w = weight ? (double)weight[lab] : 1.0;
    const double ug = gamma == 0.0 ? 1.0 : (u > 0.0 ? pow(u, gamma) : 0.0);
    acc += w * ug * -logpy;
    if (dz) {
      const double G = gs * w * ug * (gamma * py * logpy - u);
      for (int c = 0; c < C; ++c)
        dz[(size_t)b * C + c] = (float)(c == lab ? G : -(exp((double)row[c] - mo) / so) * G);
    }
  }
  __shared__ double red[4];
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / (double)B);
}

extern "C" int mi355_ce_focal(const float* z, const int64_t* y, const float* weight, float* loss, float* dz, const float* gscale, int B,
                              int C, float gamma, mi355_stream_t s) {
  MI355_CHECK_ARG(z && y && loss, "ce_focal: null pointer");
  MI355_CHECK_ARG(B > 0 && C > 0, "ce_focal: B > 0 and C > 0 expected (B=%d, C=%d)", B, C);
  MI355_CHECK_ARG(gamma >= 0.f, "ce_focal: gamma must not be negative (%g)", (double)gamma);
  hipLaunchKernelGGL(ce_focal_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, z, y, weight, loss, dz, gscale, B, C, gamma);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
