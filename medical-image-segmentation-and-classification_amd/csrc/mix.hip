// Batch mixing (utils/mix.py; nothing in the reference): mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) on the normalised fp32
// NCHW batch, where it lies after the GPU input pipeline.
//   mix_batch : out[n] = x[perm[n]] inside the sample's box, lam[n] * x[n] + (1 - lam[n]) * x[perm[n]] outside it
// Every floating-point operation is rounded on its own (no FMA contraction) and nothing is atomic: the output is bit-identical run to
// run and equals tests/mix_ref.py's float32 restatement.
// Pure streaming, two reads and one write per element.  blockIdx.y is the sample, so perm / lam / box are uniform in a workgroup (scalar
// loads, once); blockIdx.x strides over the sample's C H W elements, the threads of a wave on consecutive addresses.  The partner's
// read is a second use of bytes another workgroup streams as its own `a`: plain loads, so that it can be served from the caches.
#include "common.hpp"

// VEC: a thread owns 4 consecutive elements of one image row (W % 4 == 0, x and out 16-byte aligned; `per` = C H W is then a multiple of
// 4, so every sample starts aligned too).  The box test stays per element: box edges do not align to 4.
template <bool VEC>
__global__ __launch_bounds__(256) void mix_batch_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm,
                                                        const float* __restrict__ lam, const int32_t* __restrict__ box,
                                                        float* __restrict__ out, int N, int H, int W, unsigned per) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  int p = perm[n];
  if ((unsigned)p >= (unsigned)N) p = n;                  // the caller's contract; never an out-of-bounds read
  const float l = lam[n], oml = 1.0f - l;
  const int y0 = box[4 * n], x0 = box[4 * n + 1], y1 = box[4 * n + 2], x1 = box[4 * n + 3];
  const float* __restrict__ a = x + (size_t)n * per;
  const float* __restrict__ b = x + (size_t)p * per;
  float* __restrict__ o = out + (size_t)n * per;
  const unsigned step = gridDim.x * 256u;
  if constexpr (VEC) {
    const unsigned per4 = per >> 2, w4 = (unsigned)W >> 2;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < per4; q += step) {
      const unsigned row = q / w4;
      const int j = (int)(q - row * w4) << 2, i = (int)(row % (unsigned)H);
      const bool in_rows = i >= y0 && i < y1;
      const Vec16<float> va = ld16(a + 4 * (size_t)q), vb = ld16(b + 4 * (size_t)q);
      Vec16<float> r;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float m = l * va.v[k] + oml * vb.v[k];
        r.v[k] = (in_rows && j + k >= x0 && j + k < x1) ? vb.v[k] : m;
      }
      st16(o + 4 * (size_t)q, r);
    }
  } else {
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < per; e += step) {
      const unsigned row = e / (unsigned)W;
      const int j = (int)(e - row * (unsigned)W), i = (int)(row % (unsigned)H);
      const float va = a[e], vb = b[e];
      const float m = l * va + oml * vb;
      o[e] = (i >= y0 && i < y1 && j >= x0 && j < x1) ? vb : m;
    }
  }
}

extern "C" int mi355_mix_batch_f32(const float* x, const int32_t* perm, const float* lam, const int32_t* box, float* out, int N, int C,
                                   int H, int W, mi355_stream_t s) {
  MI355_CHECK_ARG(x && perm && lam && box && out, "mix_batch: null pointer");
  MI355_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && N <= 65535, "mix_batch: bad sizes (N=%d C=%d H=%d W=%d)", N, C, H, W);
  const long long per = (long long)C * H * W;
  MI355_CHECK_ARG(per < (1LL << 31), "mix_batch: C H W = %lld does not fit 31 bits", per);
  const uintptr_t xb = (uintptr_t)x, ob = (uintptr_t)out, bytes = (uintptr_t)N * (uintptr_t)per * sizeof(float);
  MI355_CHECK_ARG(xb + bytes <= ob || ob + bytes <= xb, "mix_batch: x and out overlap (out of place only)");
  const bool vec = (W & 3) == 0 && ((xb | ob) & 15) == 0;
  const long long work = vec ? per >> 2 : per;
  long long gx = (work + 255) / 256;
  const long long cap = (2048 + N - 1) / N;               // about 2048 workgroups in all, the rest is strided
  if (gx > cap) gx = cap;
  const dim3 grid((unsigned)gx, (unsigned)N);
  if (vec)
    hipLaunchKernelGGL(mix_batch_kernel<true>, grid, dim3(256), 0, (hipStream_t)s, x, perm, lam, box, out, N, H, W, (unsigned)per);
  else
    hipLaunchKernelGGL(mix_batch_kernel<false>, grid, dim3(256), 0, (hipStream_t)s, x, perm, lam, box, out, N, H, W, (unsigned)per);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
