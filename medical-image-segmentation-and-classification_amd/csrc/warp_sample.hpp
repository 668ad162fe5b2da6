// The sampling step of the uint8 warps, shared by warp_u8_kernel (input_pipeline.hip) and warp_field_u8_kernel (elastic.hip):
// given the source coordinates (sx, sy) of one destination pixel, write its C bytes.  One definition, so that a warp with a
// zero displacement field is the affine warp byte for byte.
#pragma once
#include "common.hpp"

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// s: one sample [Hs][Ws][C] uint8; d: the C bytes of the destination pixel.  Bilinear with cv2's rounding, or nearest; border =
// replicate or reflect-101.
__device__ __forceinline__ void warp_sample_u8(const uint8_t* __restrict__ s, int Hs, int Ws, int C, float sx, float sy,
                                               uint8_t* __restrict__ d, int nearest, int reflect) {
#pragma clang fp contract(off)      // no FMA contraction: the interpolation is then bit-reproducible against a plain IEEE evaluation
  auto at = [&](int yy, int xx, int c) -> float {
    if (reflect) { yy = reflect101(yy, Hs); xx = reflect101(xx, Ws); }
    else { yy = min(max(yy, 0), Hs - 1); xx = min(max(xx, 0), Ws - 1); }
    return (float)s[((size_t)yy * Ws + xx) * C + c];
  };
  if (nearest) {
    const int xi = (int)floorf(sx + 0.5f), yi = (int)floorf(sy + 0.5f);
    for (int c = 0; c < C; ++c) d[c] = (uint8_t)at(yi, xi, c);
  } else {
    const float fx = floorf(sx), fy = floorf(sy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float ax = sx - fx, ay = sy - fy;
    for (int c = 0; c < C; ++c) {
      const float top = at(y0, x0, c) * (1.f - ax) + at(y0, x0 + 1, c) * ax;
      const float bot = at(y0 + 1, x0, c) * (1.f - ax) + at(y0 + 1, x0 + 1, c) * ax;
      d[c] = (uint8_t)fminf(fmaxf(rintf(top * (1.f - ay) + bot * ay), 0.f), 255.f);
    }
  }
}
