// Weight gradient of a 3x3 / stride-1 / pad-1 convolution, bf16 / fp16, gfx950 — all nine taps per workgroup, four waves.
//
// A workgroup owns a 64(co) x 64(ci) tile of dW for ALL nine taps (wave w = 32x32 quadrant) and walks 32-pixel row segments
// of the image with the row-step program of wgrad3x3_rows.hpp: 9x less L2->LDS traffic than the per-tap split-K kernel (which
// is L2-bound for C <= 128).  The MFMA consumes a whole 32-pixel row segment per instruction and the wave tile is 2 x 2 blocks
// of 16 x 16 (the chip holds a higher clock on this shape, MI355X_MICROARCH.md DVFS item 7).
// W16: images 16 pixels wide.  A 32-pixel "row" is then row y of TWO images side by side: the X row image holds two 24-pixel
// segments, the dY row image the two 16-pixel rows back to back; lanes of the upper half of a K block (c4 >= 2) read the
// second segment.
#pragma once
#include "wgrad3x3_rows.hpp"

// Rings of eight rows, row r + PF fetched during step r (its slot held row r - 1).  PF = 3 left the waves waiting at the
// counted vmcnt of every step (a timing-only build without the per-step wait + barrier ran 10-18 % faster, and exactly as
// fast as the no-DMA build once the DMA was gone too: the wait was for rows, not for waves) — a row step is ~0.4 us, an
// LDS-DMA row under load takes longer than three of them.  The X row is 5 (W16: 6) DMA pieces on four waves: every wave
// moves three pieces per row, the spare ones as zeros into the zero image.
#ifndef WG3_PF
#define WG3_PF 7
#endif
template <bool W16> using Wgrad4Geo = WgradRowsGeo<4, W16, W16 ? 48 : 40, 8, WG3_PF, true>;
template <bool W16> struct Wgrad3Lds {              // dynamic LDS of wgrad3x3_halo_kernel (shared with its launcher)
  static constexpr int BYTES = Wgrad4Geo<W16>::LDS_BYTES;
};

template <typename T, bool W16 = false>
__global__ __launch_bounds__(256, 2) void wgrad3x3_halo_kernel(const Wgrad3Args a) {
  using G = Wgrad4Geo<W16>;
  static_assert(Wgrad3Lds<W16>::BYTES == 8 * ((W16 ? 48 : 40) + 32) * 128 + 4096, "launcher and kernel disagree on the LDS size");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int ciTiles = (a.Ci + 63) / 64;
  const int bid = xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int bx = bid % gridDim.x, by = bid / gridDim.x;
  const int co0 = (bx / ciTiles) * 64, ci0 = (bx % ciTiles) * 64;
  *reinterpret_cast<uint4*>(lds + G::ZERO_IMG + threadIdx.x * 16) = make_uint4(0, 0, 0, 0);      // the all-zero dY row image

  f32x4 acc[9][2][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  wgrad3_rows<T, G>(a, co0, ci0, by, acc);

  float* __restrict__ ws = a.ws + (size_t)by * a.Co * 9 * a.Ci;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int ao = 0; ao < 2; ++ao)
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) wgrad3_store_block(a, ws, co0, ci0, t, ao, bi, acc[t][ao][bi]);
}
