// Weight gradient of a 3x3 / stride-1 / pad-1 convolution, bf16 / fp16, gfx950 — all nine taps, 512-thread workgroups.
//
// The eight-wave form of wgrad3x3_halo_kernel (wgrad3x3_halo.hpp; reference call site: `convolution_backward` under
// utils/helpers.py:329 for the 3x3 layers of models/segmentation_models/AttentionUNet.py:4-13).  A workgroup still
// owns ONE 64(co) x 64(ci) tile of dW for all nine taps, but walks 64-pixel row segments: waves 0-3 take the left 32 pixels
// of a row as their MFMA K block, waves 4-7 the right 32, each wave with the 32 x 32 quadrant x 9 taps = 144 accumulator
// registers of the four-wave kernel and the same row-step program (wgrad3x3_rows.hpp).  What that buys:
//   * two waves per SIMD: one wave's fragment reads, counted waits and the per-row barrier sit in the shadow of its
//     partner's MFMAs (the four-wave kernel ran one wave per SIMD: matrix pipes 62 % busy);
//   * ONE halo per 64 pixels: a row image is 72 pixels of X for 64 pixels of dY (the four-wave kernel: 40 for 32), so the
//     L2 -> LDS stream and the HBM fetch of X shrink by 10 %, and the 17-18 DMA pieces of a row are spread over eight
//     waves with no dummy pieces (a wave issues two or three per row and counts its own);
//   * the two halves' partial tiles are added inside the workgroup (through the dead row rings in LDS) before anything
//     is written: one fp32 slab per workgroup as before, but a workgroup now covers twice the pixels per unit time.
// W32: images 32 pixels wide.  A 64-pixel "row" is then row y of TWO images side by side (work item = image pair x row
// band): the X row image holds two 40-pixel segments with their own halos, waves 4-7 read the second one.
#pragma once
#include "wgrad3x3_rows.hpp"

// X row images of 80 pixels (72 used at W % 64 == 0, 2 x 40 at W == 32); rings of six rows, row r + 5 fetched during step r:
// every ring offset fits the 16-bit immediate of a ds_read — eight-row rings of 80 + 64 pixels spilled ten registers
template <bool W32> using Wgrad8Geo = WgradRowsGeo<8, W32, 80, 6, 5, false>;
struct Wgrad8Lds {                                   // dynamic LDS of wgrad3x3_halo8_kernel (shared with its launcher)
  static constexpr int BYTES = Wgrad8Geo<false>::LDS_BYTES;
};

template <typename T, bool W32>
__global__ __launch_bounds__(512, 2) void wgrad3x3_halo8_kernel(const Wgrad3Args a) {
  using G = Wgrad8Geo<W32>;
  static_assert(Wgrad8Lds::BYTES == G::LDS_BYTES && G::LDS_BYTES == 6 * (80 + 64) * 128 + 4096, "launcher and kernel disagree on the LDS size");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = wave >> 2, w4 = wave & 3;
  const int ciTiles = (a.Ci + 63) / 64;
  const int bid = xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int bx = bid % gridDim.x, by = bid / gridDim.x;
  // Tile order inside one row band: an XCD owns Q = grid / 8 consecutive `bid`s (xcd_tile), i.e. Q tiles of one band when the
  // band has at least Q.  As a BH x BW block of the (Co / 64) x (Ci / 64) tile grid they fetch BH / coT of dY and BW / ciT of X
  // through that XCD's L2 — least for the squarest block (1024 -> 512 @32²: 4 x 4 instead of 1 x 16 = a quarter of X + half of dY
  // instead of all of X + an eighth of dY).  -DWG8_ROW_TILES: row-major tiles as before (A/B).
  int tco = bx / ciTiles, tci = bx % ciTiles;
#ifndef WG8_ROW_TILES
  {
    const int coT = gridDim.x / ciTiles, Q = (int)(gridDim.x * gridDim.y) >> 3;
    if (Q >= 4 && (int)gridDim.x % Q == 0 && ((gridDim.x * gridDim.y) & 7) == 0) {
      int BW = 0, best = 1 << 30;
      for (int w = 1; w <= Q; w <<= 1) {
        const int h = Q / w;
        if (w * h == Q && ciTiles % w == 0 && coT % h == 0 && w + h < best) { best = w + h; BW = w; }
      }
      if (BW) {
        const int BH = Q / BW, blk = bx / Q, j = bx % Q, bpr = ciTiles / BW;
        tco = (blk / bpr) * BH + j / BW;
        tci = (blk % bpr) * BW + j % BW;
      }
    }
  }
#endif
  const int co0 = tco * 64, ci0 = tci * 64;
  if (tid < 256) *reinterpret_cast<uint4*>(lds + G::ZERO_IMG + tid * 16) = make_uint4(0, 0, 0, 0);      // the all-zero dY row image (32 pixels)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                       // (written before the first item's barrier)

  f32x4 acc[9][2][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  wgrad3_rows<T, G>(a, co0, ci0, by, acc);

  // The right half's partial tile joins the left half's through the dead rings, five taps and then four: block (tap, ao, bi)
  // of quadrant w4 at [block][w4][lane] x 16 B — consecutive lanes, consecutive 16-byte slots — and ALWAYS left + right:
  // a fixed order, so the result does not depend on timing.
  static_assert(5 * 4 * 256 * 16 <= G::ZERO_IMG, "five taps of the half-tile exchange fit in the dead rings");
  float4* const xch = reinterpret_cast<float4*>(lds) + w4 * 64 + lane;
  float* __restrict__ ws = a.ws + (size_t)by * a.Co * 9 * a.Ci;
  auto exchange = [&](auto t0_tag, auto t1_tag) {
    constexpr int T0 = decltype(t0_tag)::value, T1 = decltype(t1_tag)::value;
    if (half == 1) {
#pragma unroll
      for (int t = T0; t < T1; ++t)
#pragma unroll
        for (int ao = 0; ao < 2; ++ao)
#pragma unroll
          for (int bi = 0; bi < 2; ++bi) {
            const f32x4 v = acc[t][ao][bi];
            xch[(((t - T0) * 2 + ao) * 2 + bi) * 256] = make_float4(v[0], v[1], v[2], v[3]);
          }
    }
    __syncthreads();
    if (half == 0) {
#pragma unroll
      for (int t = T0; t < T1; ++t)
#pragma unroll
        for (int ao = 0; ao < 2; ++ao)
#pragma unroll
          for (int bi = 0; bi < 2; ++bi) {
            const float4 o = xch[(((t - T0) * 2 + ao) * 2 + bi) * 256];
            wgrad3_store_block(a, ws, co0, ci0, t, ao, bi, acc[t][ao][bi] + f32x4{o.x, o.y, o.z, o.w});
          }
    }
  };
  exchange(std::integral_constant<int, 0>{}, std::integral_constant<int, 5>{});
  __syncthreads();                                   // (the left half has read the first five taps)
  exchange(std::integral_constant<int, 5>{}, std::integral_constant<int, 9>{});
}
