// Grad-CAM of the classifiers and the pipeline's image overlays (utils/explain.py, utils/pipeline.py process_images).
//
//   mi355_cam_seed           one-hot dL/dlogits of the explained class (given, or the first maximum of the logits)
//   mi355_gradcam            alpha = mean_hw dA, relu(sum_c alpha A), min-max normalised: one workgroup per image
//   mi355_resize_bilinear_f32  F.interpolate(mode="bilinear", align_corners=False) of fp32 maps
//   mi355_overlay_mask       the reference's red blend of the segmentation mask (pipeline.py:399-407)
//   mi355_overlay_heatmap    (1 - alpha) * image + alpha * 255 * jet(cam)
//
// All of it is latency-bound work on maps of a few thousand values: the kernels are plain, one thread per output element
// except the Grad-CAM reduction.  The overlays round with two separately rounded float operations (__fmul_rn / __fadd_rn: no
// contraction into an fma) so that their bytes are exactly what the same float32 arithmetic in numpy gives.
#include "common.hpp"

// ---- seed ------------------------------------------------------------------------------------------------------------
__global__ void cam_seed_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target, int B, int K,
                                float* __restrict__ dout, int32_t* __restrict__ target_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* z = logits + (size_t)b * K;
  int t;
  if (target) {
    t = target[b];
    if (t < 0 || t >= K) t = -1;                   // out of range: no class, a zero seed (the host validates before launching)
  } else {
    float m = z[0];
    t = 0;
    for (int c = 1; c < K; ++c)
      if (z[c] > m) { m = z[c]; t = c; }           // first maximum (the tie rule of cls_decide_kernel / torch.max)
  }
  for (int c = 0; c < K; ++c) dout[(size_t)b * K + c] = c == t ? 1.f : 0.f;
  target_out[b] = t;
}

extern "C" int mi355_cam_seed(const float* logits, const int32_t* target, int B, int K, float* dout, int32_t* target_out,
                              mi355_stream_t s) {
  MI355_CHECK_ARG(logits && dout && target_out && B > 0 && K > 0, "cam_seed: bad arguments (B=%d, K=%d)", B, K);
  hipLaunchKernelGGL(cam_seed_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, (hipStream_t)s, logits, target, B, K, dout, target_out);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- Grad-CAM --------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads (four waves) per image; LDS holds alpha[C] then raw[HW] (fp32).
constexpr int CAM_THREADS = 256;
constexpr int CAM_LDS_BYTES = 48 * 1024;

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

template <typename T>
__global__ __launch_bounds__(CAM_THREADS) void gradcam_kernel(const T* __restrict__ A, int ldA, const T* __restrict__ dA, int lddA,
                                                              int HW, int C, float* __restrict__ cam) {
  extern __shared__ float lds[];
  float* alpha = lds;                 // [C]
  float* raw = lds + C;               // [HW]
  __shared__ float red[2][CAM_THREADS / MI355_WAVE];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & (MI355_WAVE - 1), wave = tid / MI355_WAVE;
  constexpr int NW = CAM_THREADS / MI355_WAVE;
  const size_t row0 = (size_t)n * HW;
  // alpha[c] = mean over the pixels of dA[., c]: lanes run over channels (coalesced NHWC rows), fp32 sum
  const float inv_hw = 1.f / (float)HW;
  for (int c = tid; c < C; c += CAM_THREADS) {
    float acc = 0.f;
    for (int p = 0; p < HW; ++p) acc += to_f32<T>(dA[(row0 + p) * lddA + c]);
    alpha[c] = acc * inv_hw;
  }
  __syncthreads();
  // raw[p] = relu(sum_c alpha[c] A[p, c]): one wave per pixel, lanes over channels, wave64 butterfly
  for (int p = wave; p < HW; p += NW) {
    const T* a = A + (row0 + p) * ldA;
    float acc = 0.f;
    for (int c = lane; c < C; c += MI355_WAVE) acc += alpha[c] * to_f32<T>(a[c]);
    acc = wave_sum(acc);
    if (lane == 0) raw[p] = fmaxf(acc, 0.f);
  }
  __syncthreads();
  // min / max over the map: per thread, per wave (shuffles), across the waves (LDS)
  float lo = INFINITY, hi = -INFINITY;
  for (int p = tid; p < HW; p += CAM_THREADS) {
    lo = fminf(lo, raw[p]);
    hi = fmaxf(hi, raw[p]);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane == 0) {
    red[0][wave] = lo;
    red[1][wave] = hi;
  }
  __syncthreads();
  lo = red[0][0];
  hi = red[1][0];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    lo = fminf(lo, red[0][w]);
    hi = fmaxf(hi, red[1][w]);
  }
  // pytorch-grad-cam's scale_cam_image: img - min, then / (1e-7 + max(img - min)); max(raw - min) == fl(hi - lo) (rounding is monotone)
  const float den = 1e-7f + (hi - lo);
  for (int p = tid; p < HW; p += CAM_THREADS) cam[row0 + p] = (raw[p] - lo) / den;
}

extern "C" int mi355_gradcam(const void* A, int ldA, const void* dA, int lddA, int N, int HW, int C, int dtype, float* cam_lowres,
                             mi355_stream_t s) {
  MI355_CHECK_ARG(A && dA && cam_lowres && N > 0 && HW > 0 && C > 0 && ldA >= C && lddA >= C,
                  "gradcam: bad arguments (N=%d, HW=%d, C=%d, ldA=%d, lddA=%d)", N, HW, C, ldA, lddA);
  const long long lds = 4LL * ((long long)HW + C);
  if (lds > CAM_LDS_BYTES)
    MI355_FAIL(MI355_ERR_UNSUPPORTED, "gradcam: HW=%d and C=%d need %lld bytes of LDS, more than the %d this kernel uses", HW, C, lds,
               CAM_LDS_BYTES);
  return dispatch_dtype(dtype, "gradcam", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((gradcam_kernel<T>), dim3(N), dim3(CAM_THREADS), (size_t)lds, (hipStream_t)s, (const T*)A, ldA, (const T*)dA,
                       lddA, HW, C, cam_lowres);
    MI355_LAUNCH_CHECK();
    return (int)MI355_OK;
  });
}

// ---- bilinear resize (align_corners=False) -----------------------------------------------------------------------------
// source coordinate (dst + 0.5) * in / out - 0.5, clamped below at 0; the upper neighbour is clamped to the last row / column
__device__ __forceinline__ void bilinear_src(int d, float scale, int in, int& i0, int& i1, float& l1) {
  float src = scale * ((float)d + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

__global__ void resize_bilinear_kernel(const float* __restrict__ src, int h, int w, float* __restrict__ dst, int H, int W,
                                       float sy, float sx, long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const long long r = i / W;
    const int y = (int)(r % H);
    const long long n = r / H;
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_src(y, sy, h, y0, y1, ly);
    bilinear_src(x, sx, w, x0, x1, lx);
    const float* s = src + (size_t)n * h * w;
    const float top = (1.f - lx) * s[y0 * w + x0] + lx * s[y0 * w + x1];
    const float bot = (1.f - lx) * s[y1 * w + x0] + lx * s[y1 * w + x1];
    dst[i] = (1.f - ly) * top + ly * bot;
  }
}

extern "C" int mi355_resize_bilinear_f32(const float* src, int N, int h, int w, float* dst, int H, int W, mi355_stream_t s) {
  MI355_CHECK_ARG(src && dst && N > 0 && h > 0 && w > 0 && H > 0 && W > 0, "resize_bilinear_f32: bad arguments");
  const long long total = (long long)N * H * W;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)s, src, h, w, dst, H, W, (float)h / (float)H,
                     (float)w / (float)W, total);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---- overlays on uint8 RGB HWC images ------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t sat_u8(float v) {
  v = __builtin_rintf(v);                           // round half to even (cv2's saturate_cast)
  return (uint8_t)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

// pipeline.py:399-407: mask resized nearest (src = dst * h / H in integers); where it is 255, R += 255 * opacity, saturated
__global__ void overlay_mask_kernel(const uint8_t* __restrict__ img, int H, int W, const uint8_t* __restrict__ mask, int h, int w,
                                    float red, uint8_t* __restrict__ out, long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const long long r = i / W;
    const int y = (int)(r % H);
    const long long n = r / H;
    const int my = (int)(((long long)y * h) / H), mx = (int)(((long long)x * w) / W);
    const bool on = mask[((size_t)n * h + my) * w + mx] == 255;
    const uint8_t* p = img + (size_t)i * 3;
    uint8_t* q = out + (size_t)i * 3;
    q[0] = on ? sat_u8(__fadd_rn((float)p[0], red)) : p[0];
    q[1] = p[1];
    q[2] = p[2];
  }
}

extern "C" int mi355_overlay_mask(const uint8_t* img, int B, int H, int W, const uint8_t* mask, int h, int w, float opacity, uint8_t* out,
                                  mi355_stream_t s) {
  MI355_CHECK_ARG(img && mask && out && B > 0 && H > 0 && W > 0 && h > 0 && w > 0, "overlay_mask: bad arguments");
  const long long total = (long long)B * H * W;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const float red = 255.f * opacity;                // (host multiply: one rounding, as numpy's float32 255 * opacity)
  hipLaunchKernelGGL(overlay_mask_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)s, img, H, W, mask, h, w, red, out, total);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// matplotlib's 256-entry "jet" (LinearSegmentedColormap._create_lookup_table of its segment data, x = linspace(0, 1, 256)),
// evaluated at compile time in double and stored as float
struct JetLut {
  float v[256][3];
};
struct JetSeg {
  int n;
  double x[6], y[6];
};
constexpr double jet_eval(const JetSeg& s, double xi) {
  if (xi <= s.x[0]) return s.y[0];
  int j = 1;
  while (j < s.n - 1 && s.x[j] < xi) ++j;           // first point with x >= xi (np.searchsorted, side "left")
  const double d = (xi - s.x[j - 1]) / (s.x[j] - s.x[j - 1]);
  const double v = d * (s.y[j] - s.y[j - 1]) + s.y[j - 1];
  return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}
constexpr JetLut make_jet() {
  JetLut t{};
  const JetSeg r{5, {0.0, 0.35, 0.66, 0.89, 1.0}, {0.0, 0.0, 1.0, 1.0, 0.5}};
  const JetSeg g{6, {0.0, 0.125, 0.375, 0.64, 0.91, 1.0}, {0.0, 0.0, 1.0, 1.0, 0.0, 0.0}};
  const JetSeg b{5, {0.0, 0.11, 0.34, 0.65, 1.0}, {0.5, 1.0, 1.0, 0.0, 0.0}};
  const double step = 1.0 / 255.0;
  for (int i = 0; i < 256; ++i) {
    const double xi = i == 255 ? 1.0 : i * step;    // numpy.linspace: i * step, the last point exactly the end
    t.v[i][0] = (float)jet_eval(r, xi);
    t.v[i][1] = (float)jet_eval(g, xi);
    t.v[i][2] = (float)jet_eval(b, xi);
  }
  return t;
}
__constant__ JetLut c_jet = make_jet();

__global__ void overlay_heatmap_kernel(const uint8_t* __restrict__ img, const float* __restrict__ cam, float keep, float alpha255,
                                       uint8_t* __restrict__ out, long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const float v = cam[i];
    int k = v > 0.f ? (int)(v * 256.f) : 0;         // (NaN -> entry 0)
    if (k > 255) k = 255;
    const uint8_t* p = img + (size_t)i * 3;
    uint8_t* q = out + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = sat_u8(__fadd_rn(__fmul_rn(keep, (float)p[c]), __fmul_rn(alpha255, c_jet.v[k][c])));
  }
}

extern "C" int mi355_overlay_heatmap(const uint8_t* img, int B, int H, int W, const float* cam, float alpha, uint8_t* out,
                                     mi355_stream_t s) {
  MI355_CHECK_ARG(img && cam && out && B > 0 && H > 0 && W > 0, "overlay_heatmap: bad arguments");
  const long long total = (long long)B * H * W;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  // (host operations, one rounding each, as numpy's float32 1 - alpha and alpha * 255)
  hipLaunchKernelGGL(overlay_heatmap_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)s, img, cam, 1.f - alpha, alpha * 255.f, out,
                     total);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
