// Test-time augmentation (utils/tta.py; nothing in the reference): predict on K mirrored / slightly rotated and rescaled views of a
// batch, map the predictions back and merge them.
//   warp_f32       : the view of a normalised fp32 NCHW batch under a per-sample dst -> src affine map (bilinear, reflect-101: what
//                    the train-mode warp does to the uint8 image, csrc/warp_sample.hpp, without the rounding to bytes)
//   tta_fold       : K one-channel logit maps -> mean, population variance, vote counts and the thresholded mask of the views that
//                    are valid at each pixel, sampled back through the source -> view maps
//   cls_tta_decide : K logit rows per sample -> mean softmax, its argmax, confidence, agreement of the views, kept samples
// Every floating-point operation is rounded on its own (no FMA contraction), nothing is atomic and every sum runs in a fixed
// order: the outputs are bit-identical run to run and equal tests/tta_ref.py's float32 restatement.
// Both image kernels stream: one thread per pixel, the threads of a wave on consecutive x of one row, so the identity and the
// mirrored view read whole rows and every store is a contiguous run of the wave.
#include "common.hpp"
#include "decide.hpp"
#include "warp_sample.hpp"

#define TTA_MAX_VIEWS 16

// the four taps of one plane [H][W] at (x0, y0), (x1, y0), (x0, y1), (x1, y1) blended by (ax, ay): warp_sample_u8's formula
__device__ __forceinline__ float bilinear_f32(const float* __restrict__ p, int W, int x0, int x1, int y0, int y1, float ax, float ay) {
#pragma clang fp contract(off)
  const float top = p[(size_t)y0 * W + x0] * (1.f - ax) + p[(size_t)y0 * W + x1] * ax;
  const float bot = p[(size_t)y1 * W + x0] * (1.f - ax) + p[(size_t)y1 * W + x1] * ax;
  return top * (1.f - ay) + bot * ay;
}

// reflect101 at any distance: the index is first reduced by the period 2 n - 2, so the helper's loop runs at most once
__device__ __forceinline__ int reflect101_far(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  i %= p;
  return reflect101(i < 0 ? i + p : i, n);
}

// m: [N][6] row-major 2x3, dst pixel (x, y) -> src coordinates
__global__ void warp_f32_kernel(const float* __restrict__ src, int C, int H, int W, const float* __restrict__ m, float* __restrict__ dst,
                                long long total) {
#pragma clang fp contract(off)
  const size_t plane = (size_t)H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    long long r = i / W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    const float* mm = m + (size_t)n * 6;
    const float sx = (mm[0] * (float)x + mm[1] * (float)y) + mm[2], sy = (mm[3] * (float)x + mm[4] * (float)y) + mm[5];
    const float fx = floorf(sx), fy = floorf(sy);
    const float ax = sx - fx, ay = sy - fy;
    const int xi = (int)fminf(fmaxf(fx, -1048576.f), 1048576.f), yi = (int)fminf(fmaxf(fy, -1048576.f), 1048576.f);   // any matrix, NaN included: an int
    const int x0 = reflect101_far(xi, W), x1 = reflect101_far(xi + 1, W);
    const int y0 = reflect101_far(yi, H), y1 = reflect101_far(yi + 1, H);
    const float* s = src + (size_t)n * C * plane;
    float* d = dst + (size_t)n * C * plane + (size_t)y * W + x;
    for (int c = 0; c < C; ++c) d[c * plane] = bilinear_f32(s + c * plane, W, x0, x1, y0, y1, ax, ay);
  }
}

extern "C" int mi355_warp_f32(const float* src, int N, int C, int H, int W, const float* m, float* dst, mi355_stream_t s) {
  MI355_CHECK_ARG(src && m && dst && src != dst && N > 0 && C > 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768,
                  "warp_f32: bad arguments (N=%d C=%d H=%d W=%d)", N, C, H, W);
  const long long total = (long long)N * H * W;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(warp_f32_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)s, src, C, H, W, m, dst, total);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// z: [K][N][H][W]; s2d: [K][6], source pixel -> its place in view k.  The K samples of a pixel stay in registers (the loop is
// unrolled to the cap and guarded by k < K): the variance needs the mean first and nothing is sampled twice.
__global__ void tta_fold_kernel(const float* __restrict__ z, int K, int N, int H, int W, const float* __restrict__ s2d, int prob, float thr,
                                const int32_t* __restrict__ idx, float* __restrict__ mean, float* __restrict__ var,
                                uint8_t* __restrict__ votes, uint8_t* __restrict__ mask, long long total) {
#pragma clang fp contract(off)
  const size_t plane = (size_t)H * W;
  const float xmax = (float)(W - 1), ymax = (float)(H - 1);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    long long r = i / W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    const size_t q = (size_t)y * W + x;
    float v[TTA_MAX_VIEWS];
    unsigned valid = 0;
    int cnt = 0, pos = 0;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < TTA_MAX_VIEWS; ++k) {
      v[k] = 0.f;
      if (k < K) {
        const float* mm = s2d + k * 6;
        const float px = (mm[0] * (float)x + mm[1] * (float)y) + mm[2], py = (mm[3] * (float)x + mm[4] * (float)y) + mm[5];
        if (px >= 0.f && px <= xmax && py >= 0.f && py <= ymax) {
          const float fx = floorf(px), fy = floorf(py);
          const int x0 = (int)fx, y0 = (int)fy;
          const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);       // a clamped tap has weight 0
          float s = bilinear_f32(z + ((size_t)k * N + n) * plane, W, x0, x1, y0, y1, px - fx, py - fy);
          if (prob) s = sigmoid_f32(s);
          if (votes) pos += (prob ? s : sigmoid_f32(s)) > thr;
          v[k] = s;
          valid |= 1u << k;
          sum += s;
          ++cnt;
        }
      }
    }
    const float fcnt = (float)cnt;                  // cnt = 0 (no identity view among the maps): 0 / 0, the caller's contract
    const float mu = sum / fcnt;
    mean[(size_t)n * plane + q] = mu;
    if (var) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < TTA_MAX_VIEWS; ++k)
        if (valid >> k & 1u) {
          const float d = v[k] - mu;
          acc += d * d;
        }
      var[(size_t)n * plane + q] = acc / fcnt;
    }
    if (votes) {
      votes[((size_t)n * 2 + 0) * plane + q] = (uint8_t)pos;
      votes[((size_t)n * 2 + 1) * plane + q] = (uint8_t)cnt;
    }
    if (mask) mask[(size_t)(idx ? idx[n] : n) * plane + q] = (prob ? mu : sigmoid_f32(mu)) > thr ? 255 : 0;
  }
}

extern "C" int mi355_tta_fold(const float* z, int K, int N, int H, int W, const float* s2d, int prob, float thr, const int32_t* idx,
                              float* mean, float* var, uint8_t* votes, uint8_t* mask, mi355_stream_t s) {
  MI355_CHECK_ARG(z && s2d && mean && K >= 1 && K <= TTA_MAX_VIEWS && N > 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768,
                  "tta_fold: bad arguments (K=%d N=%d H=%d W=%d)", K, N, H, W);
  const long long total = (long long)N * H * W;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(tta_fold_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)s, z, K, N, H, W, s2d, prob, thr, idx, mean, var, votes,
                     mask, total);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// logits: [K][B][C].  Thread b: probs[b][.] accumulates the views' softmax rows in order k (its own row of the output is the
// accumulator), then the argmax of the mean, then the confidence and the agreement from a second pass over the K rows.
__global__ void cls_tta_decide_kernel(const float* __restrict__ logits, int K, int B, int C, int keep_class, float* __restrict__ probs,
                                      int32_t* __restrict__ pred, float* __restrict__ conf, int32_t* __restrict__ agree,
                                      int32_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
#pragma clang fp contract(off)
  __shared__ int flag[1024];
  const int b = threadIdx.x;
  int mine = 0;
  if (b < B) {
    float* p = probs + (size_t)b * C;
    for (int c = 0; c < C; ++c) p[c] = 0.f;
    for (int k = 0; k < K; ++k) {
      const float* z = logits + ((size_t)k * B + b) * C;
      float m, den;
      int am;
      softmax_row_stats(z, C, m, am, den);
      for (int c = 0; c < C; ++c) p[c] += expf(z[c] - m) / den;
    }
    const float fk = (float)K;
    for (int c = 0; c < C; ++c) p[c] = p[c] / fk;
    float best = p[0];
    int am = 0;
    for (int c = 1; c < C; ++c)
      if (p[c] > best) { best = p[c]; am = c; }          // first maximum
    float pct = 0.f;
    int ag = 0;
    for (int k = 0; k < K; ++k) {
      const float* z = logits + ((size_t)k * B + b) * C;
      float m, den;
      int amk;
      softmax_row_stats(z, C, m, amk, den);
      pct += (100.f * expf(z[am] - m)) / den;              // K = 1: z[am] = m, 100 / den: cls_decide's expression
      ag += amk == am;
    }
    pred[b] = am;
    conf[b] = pct / fk;
    agree[b] = ag;
    mine = am == keep_class;
  }
  compact_kept(flag, b, B, mine, kept, n_kept);
}

extern "C" int mi355_cls_tta_decide(const float* logits, int K, int B, int C, int keep_class, float* probs, int32_t* pred, float* conf,
                                    int32_t* agree, int32_t* kept, int32_t* n_kept, mi355_stream_t s) {
  MI355_CHECK_ARG(logits && probs && pred && conf && agree && kept && n_kept && K >= 1 && K <= TTA_MAX_VIEWS && B > 0 && B <= 1024 && C > 0,
                  "cls_tta_decide: bad arguments (K=%d B=%d)", K, B);
  hipLaunchKernelGGL(cls_tta_decide_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, logits, K, B, C, keep_class, probs, pred, conf, agree,
                     kept, n_kept);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
