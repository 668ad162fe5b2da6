// CLAHE (contrast-limited adaptive histogram equalisation; A.CLAHE / cv2.createCLAHE) for the GPU input pipeline, as two entry points
// over interleaved uint8 batches [N][H][W][C] (the layout warp_u8 writes), every channel plane equalised on its own:
//   clahe_lut_u8   : one 256-entry LUT per (sample, channel, tile): histogram, clip, redistribute, prefix sum, scale.
//   clahe_apply_u8 : every pixel through the bilinear blend of its four neighbouring tiles' LUTs.
// The rules (padding quirk included) are in the header; they restate OpenCV's clahe.cpp.
//
// LUT kernel.  One workgroup of 256 threads per (sample, channel, tile); the threads walk the tile's pixels in steps of 256, so a
// 2 x 2 tile keeps 4 threads busy and a 300-column tile takes as many passes as it needs.  Pixels of the padded border read the
// mirrored index.  Each wave adds into a 256-bin histogram of its own in LDS: chest films fill a narrow band of grey levels, and
// four waves on one histogram would queue on the same few banks; within a wave the lanes that meet in one bin still serialise.
// Then one bin per thread: fold the four histograms, clip, block-reduce the excess, redistribute, inclusive scan (wave scan plus
// the totals of the waves before), one fp32 multiply, one byte stored.  All of it integer arithmetic up to that multiply.
//
// Apply kernel.  Purely streaming: a thread owns four consecutive bytes of the interleaved stream (one 4-byte load and store when
// both pointers allow it), and per byte gathers four LUT entries straight from global memory.  The LUTs of a 32 x 3 x 8 x 8 batch are
// 1.5 MB and sit in every XCD's 4 MiB L2 next to the streamed image; the 1 KiB a 32 x 32 tile quadrant needs per channel stays in
// the CU's L1.  No LDS staging: a workgroup's bytes would have to be cut along half-tile boundaries for it to need four LUTs
// only, which any tile size from 1 up defeats; the gather's address rate, not bandwidth, bounds the kernel.
#include "common.hpp"

#define CLAHE_MAX_GRID 64
#define CLAHE_MAX_AREA (1 << 24)

struct ClaheGeom {
  int th, tw;         // tile
};

// padded extents and tile of an H x W plane under a gy x gx grid; false when the rules of the header reject it
static bool clahe_geometry(int H, int W, int gy, int gx, ClaheGeom* g, const char** why) {
  int ph = 0, pw = 0;
  if (H % gy != 0 || W % gx != 0) {
    ph = gy - H % gy;
    pw = gx - W % gx;
  }
  if (ph > H - 1 || pw > W - 1) {
    *why = "the padding exceeds the plane";
    return false;
  }
  g->th = (H + ph) / gy;
  g->tw = (W + pw) / gx;
  if ((long long)g->th * g->tw > CLAHE_MAX_AREA) {
    *why = "a tile holds more than 2^24 pixels";
    return false;
  }
  return true;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid: N * C * gy * gx workgroups of 256 threads; block b = ((n * C + c) * gy + ty) * gx + tx, the order of the LUTs
__global__ __launch_bounds__(256) void clahe_lut_kernel(const uint8_t* __restrict__ src, int H, int W, int C, int gy, int gx, int th, int tw,
                                                        int lim, float scale, uint8_t* __restrict__ luts) {
  __shared__ int hist[4][256];
  __shared__ int part[8];                                // [0..3]: excess per wave, [4..7]: histogram total per wave
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int b = blockIdx.x;
  const int tx = b % gx; b /= gx;
  const int ty = b % gy; b /= gy;
  const int c = b % C;
  const int n = b / C;
#pragma unroll
  for (int w = 0; w < 4; ++w) hist[w][tid] = 0;
  __syncthreads();
  const uint8_t* plane = src + (size_t)n * H * W * C + c;
  const int area = th * tw, y0 = ty * th, x0 = tx * tw;
  for (int p = tid; p < area; p += 256) {
    int y = y0 + p / tw, x = x0 + p % tw;
    if (y >= H) y = 2 * (H - 1) - y;                     // BORDER_REFLECT_101; the launcher keeps the pad <= extent - 1, so >= 0
    if (x >= W) x = 2 * (W - 1) - x;
    // integer adds: whatever order the LDS serves them in, the counts are the same
    atomicAdd(&hist[wv][plane[((size_t)y * W + x) * C]], 1);
  }
  __syncthreads();
  int h = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
  if (lim > 0) {
    const int over = wave_sum_i(max(h - lim, 0));
    if (lane == 0) part[wv] = over;
    __syncthreads();
    const int excess = part[0] + part[1] + part[2] + part[3];
    h = min(h, lim) + (excess >> 8);
    const int res = excess & 255;
    if (res) {
      const int step = max(256 / res, 1);
      if (tid % step == 0 && tid / step < res) h += 1;
    }
  }
  int sum = h;                                           // inclusive scan over the wave's 64 bins
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(sum, o, 64);
    if (lane >= o) sum += up;
  }
  if (lane == 63) part[4 + wv] = sum;
  __syncthreads();
  for (int w = 0; w < wv; ++w) sum += part[4 + w];
  const float v = __builtin_rintf((float)sum * scale);       // one multiply: nothing to fuse with
  luts[(size_t)blockIdx.x * 256 + tid] = (uint8_t)fminf(fmaxf(v, 0.f), 255.f);
}

// floor of the tile coordinate of pixel i, its two clamped tile indices and weights (header: the order of the operations)
__device__ __forceinline__ void clahe_axis(int i, float inv_t, int g, int& t1, int& t2, float& a, float& a1) {
  // plain operators under contract(off), not __fmul_rn / __fsub_rn: those are inline functions compiled under the file's default
  // (contract fast), and their products did fuse with the sums after inlining
#pragma clang fp contract(off)
  const float tf = (float)i * inv_t - 0.5f;
  const float fl = floorf(tf);
  a = tf - fl;
  a1 = 1.f - a;
  t1 = (int)fl;
  t2 = min(t1 + 1, g - 1);
  t1 = max(t1, 0);
}

__device__ __forceinline__ uint8_t clahe_blend(const uint8_t* __restrict__ l11, const uint8_t* __restrict__ l12, const uint8_t* __restrict__ l21,
                                               const uint8_t* __restrict__ l22, int v, float xa, float xa1, float ya, float ya1) {
#pragma clang fp contract(off)      // every product rounded before its sum, as the header states (a fused form moves .5 ties)
  const float top = (float)l11[v] * xa1 + (float)l12[v] * xa;
  const float bot = (float)l21[v] * xa1 + (float)l22[v] * xa;
  const float r = __builtin_rintf(top * ya1 + bot * ya);
  return (uint8_t)fminf(fmaxf(r, 0.f), 255.f);
}

// A thread owns bytes 4 i .. 4 i + 3 of the interleaved stream [N H][W C]; `words`: src and dst are 4-byte aligned
__global__ __launch_bounds__(256) void clahe_apply_kernel(const uint8_t* __restrict__ src, int H, int W, int C, int gy, int gx, float inv_th,
                                                          float inv_tw, const uint8_t* __restrict__ luts, uint8_t* __restrict__ dst,
                                                          long long total, int words) {
  const int rowb = W * C;
  const long long quads = (total + 3) >> 2;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long long)gridDim.x * blockDim.x) {
    const long long i0 = q << 2;
    const int nb = (int)min(4LL, total - i0);
    uint32_t in = 0, out = 0;                            // byte k of the quad in bits 8 k .. 8 k + 7
    if (words && nb == 4) {
      in = *reinterpret_cast<const uint32_t*>(src + i0);
    } else {
      for (int j = 0; j < nb; ++j) in |= (uint32_t)src[i0 + j] << (8 * j);
    }
    long long row = i0 / rowb;                           // n * H + y
    int col = (int)(i0 - row * rowb);                    // x * C + c
    int k = 0;
    while (k < nb) {
      const int y = (int)(row % H), n = (int)(row / H);
      int ty1, ty2;
      float ya, ya1;
      clahe_axis(y, inv_th, gy, ty1, ty2, ya, ya1);
      for (; k < nb && col < rowb; ++k, ++col) {
        const int x = col / C, c = col - x * C;
        int tx1, tx2;
        float xa, xa1;
        clahe_axis(x, inv_tw, gx, tx1, tx2, xa, xa1);
        const uint8_t* l = luts + (size_t)(n * C + c) * gy * gx * 256;
        out |= (uint32_t)clahe_blend(l + (ty1 * gx + tx1) * 256, l + (ty1 * gx + tx2) * 256, l + (ty2 * gx + tx1) * 256,
                                     l + (ty2 * gx + tx2) * 256, (in >> (8 * k)) & 255, xa, xa1, ya, ya1)
               << (8 * k);
      }
      col = 0;
      ++row;
    }
    if (words && nb == 4) {
      *reinterpret_cast<uint32_t*>(dst + i0) = out;
    } else {
      for (int j = 0; j < nb; ++j) dst[i0 + j] = (uint8_t)(out >> (8 * j));
    }
  }
}

// the checks both entry points share; fills the geometry
static int clahe_check(const char* who, int N, int H, int W, int C, int gy, int gx, ClaheGeom* g) {
  MI355_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: N, H, W must be positive (%d, %d, %d)", who, N, H, W);
  MI355_CHECK_ARG(C == 1 || C == 3, "%s: C = %d, must be 1 or 3", who, C);
  MI355_CHECK_ARG(gy >= 1 && gy <= CLAHE_MAX_GRID && gx >= 1 && gx <= CLAHE_MAX_GRID, "%s: grid %d x %d outside 1 .. %d", who, gy, gx,
                  CLAHE_MAX_GRID);
  MI355_CHECK_ARG(H <= (1 << 28) && W <= (1 << 28), "%s: H, W above 2^28 (%d, %d)", who, H, W);
  const char* why = "";
  MI355_CHECK_ARG(clahe_geometry(H, W, gy, gx, g, &why), "%s: %d x %d under a %d x %d grid: %s", who, H, W, gy, gx, why);
  MI355_CHECK_ARG((long long)N * C * gy * gx <= 0x7fffffLL, "%s: %d x %d planes of %d x %d tiles are more than 2^23 - 1 LUTs", who, N, C, gy, gx);
  MI355_CHECK_ARG((long long)W * C <= 0x7fffffffLL, "%s: a row of %d x %d bytes is above 2^31 - 1", who, W, C);
  return MI355_OK;
}

extern "C" int mi355_clahe_lut_u8(const uint8_t* src, int N, int H, int W, int C, int gy, int gx, int clip_count, uint8_t* luts,
                                  mi355_stream_t s) {
  MI355_CHECK_ARG(src, "clahe_lut_u8: null pointer (src)");
  MI355_CHECK_ARG(luts, "clahe_lut_u8: null pointer (luts)");
  MI355_CHECK_ARG((const void*)src != (const void*)luts, "clahe_lut_u8: src and luts must not alias");
  MI355_CHECK_ARG(clip_count >= 0, "clahe_lut_u8: clip_count %d is negative", clip_count);
  ClaheGeom g;
  if (int rc = clahe_check("clahe_lut_u8", N, H, W, C, gy, gx, &g)) return rc;
  const float scale = 255.f / (float)(g.th * g.tw);
  hipLaunchKernelGGL(clahe_lut_kernel, dim3((unsigned)(N * C * gy * gx)), dim3(256), 0, (hipStream_t)s, src, H, W, C, gy, gx, g.th, g.tw,
                     clip_count, scale, luts);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_clahe_apply_u8(const uint8_t* src, int N, int H, int W, int C, int gy, int gx, const uint8_t* luts, uint8_t* dst,
                                    mi355_stream_t s) {
  MI355_CHECK_ARG(src, "clahe_apply_u8: null pointer (src)");
  MI355_CHECK_ARG(luts, "clahe_apply_u8: null pointer (luts)");
  MI355_CHECK_ARG(dst, "clahe_apply_u8: null pointer (dst)");
  MI355_CHECK_ARG((const void*)src != (const void*)dst, "clahe_apply_u8: src and dst must not alias");
  MI355_CHECK_ARG((const void*)luts != (const void*)dst, "clahe_apply_u8: luts and dst must not alias");
  ClaheGeom g;
  if (int rc = clahe_check("clahe_apply_u8", N, H, W, C, gy, gx, &g)) return rc;
  const float inv_th = 1.f / (float)g.th, inv_tw = 1.f / (float)g.tw;
  const long long total = (long long)N * H * W * C;
  long long blocks = ((total + 3) / 4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const int words = ((uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0) ? 1 : 0;
  hipLaunchKernelGGL(clahe_apply_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)s, src, H, W, C, gy, gx, inv_th, inv_tw, luts, dst, total,
                     words);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
