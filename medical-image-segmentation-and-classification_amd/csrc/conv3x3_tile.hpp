// What the 3x3 halo-family kernels (conv3x3_halo.hpp, _halo_pp.hpp, _halo_pp128.hpp, conv3x3_ws.hpp) share around their K loops:
// the tile decode, the weight-row / tap addressing, the statistics fold and the launcher — and, written down
// once, the contract of the epilogues.
//
// THE STAGED C TILE (every kernel's `finish` and what follows it).  The MFMAs run with the weight fragment as the A operand, so a
// lane holds, per 16x16 block, FOUR CONSECUTIVE CHANNELS (4*c4 .. +3) of ONE pixel (l16): bias / ReLU / rounding happen once per
// value in registers, a block is staged with ONE 8-byte LDS write per lane (conflict-free at the row pitches in use: BN * 2 + 16
// bytes, BN * 2 + 8 in the weight-stationary kernel), and the tile leaves as 16-byte row-contiguous stores (whole 128-B lines;
// 8-byte stores straight from the registers were measured: 4x the line accesses, -10 %).  Everything behind the staging works on
// the ROUNDED values:
//   * statistics (a.stats: per-channel sum and sum of squares for a fused BatchNorm) are of the rounded outputs, summed two
//     channels at a time (packed fp32 adds / fmas), folded over the 16 pixel lanes of a row with DPP adds (no LDS traffic), then
//     over the waves that share a channel through red[wave rows][2][BN] behind the C tile(s);
//   * the 2x2 sum (a.pool2: gradient of a fused nearest x2 up-sampling) reads the four rounded tile values of a group back from
//     LDS, adds them in fp32 and rounds again, as the separate mi355_upsample2_bwd pass did;
//   * accumulation (a.accumulate) adds the destination to the rounded value and rounds again.
// ReLU and the statistics are workgroup-uniform switches: four straight-line variants of `finish` instead of 64 dead v_max / a
// test per block.  The kernels differ only in the tile pixel of block mb (rw, pp: wm * WTM + mb * 16 + l16; pp128: mb * TW +
// wm * 16 + l16; ws: mb * 16 + l16), in where the bias joins (pp128: in `finish`; the others: as the first MFMA's C operand), in
// whether the sums are per tile or run across the workgroup's tiles (ws), and in the order of old-value loads against stores.
//
// Which kernel shares which piece, and why the others keep their copies: DESIGN.md, below the kernel table.
#pragma once
#include "common.hpp"

// workgroup -> (image n, tile origin (y0, x0), first output channel n0), channel tiles fastest: the channel tiles of one patch
// are neighbours in xcd_tile's order.  sp = spatial tile index = the tile's row of partial statistics.
struct HaloTile { int sp, n, y0, x0, n0; };
template <int TH, int TW, int BN> __device__ __forceinline__ HaloTile halo_tile(const ConvArgs& a) {
  const int NT = a.Co / BN, TXN = a.Wo / TW, TYN = a.Ho / TH;
  int t = xcd_tile(blockIdx.x, gridDim.x);
  const int nt = t % NT; t /= NT;
  const int sp = t;
  const int tx = t % TXN; t /= TXN;
  const int ty = t % TYN;
  return {sp, t / TYN, ty * TH, tx * TW, nt * BN};
}

// A DMA lane's source inside weight row `row` (wrow = 9 * Ci elements per row), in ELEMENTS of T from the row block's base: the
// lane's 16-byte chunk sits in slot chunk ^ (((row >> 2) & 1) << 1) of the slab image
template <typename T> __device__ __forceinline__ size_t weight_row_offset(int row, size_t wrow, int slot) {
  return (size_t)row * wrow + (slot ^ (((row >> 2) & 1) << 1)) * (16 / sizeof(T));
}
// tap (ph, pw) of the 3x3 window; mirrored for the data gradient
__device__ __forceinline__ int tap_index(bool flip, int ph, int pw) { return flip ? (2 - ph) * 3 + (2 - pw) : ph * 3 + pw; }

// behind the barrier that ends the staging: red[ROWS][2][BN] -> the tile's row of partial statistics
template <int ROWS, int BN> __device__ __forceinline__ void fold_tile_stats(const ConvArgs& a, const float* red, int tid, const HaloTile& t) {
  if (a.stats && tid < 2 * BN) {
    const int q = tid / BN, c = tid - q * BN;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < ROWS; ++w) v += red[(w * 2 + q) * BN + c];
    a.stats[((size_t)t.sp * 2 + q) * a.Co + t.n0 + c] = v;
  }
}

// The LDS reservation is made once per process and kernel instantiation (kernel and LDS size are template parameters, so every
// instantiation has a static of its own): a function-local static is initialised exactly once even when two threads launch
// concurrently (forward on the main thread, backward on the autograd worker).
template <auto KERNEL, int LDS_BYTES, typename... Args>
static int launch_with_lds(const char* name, int grid, int block, hipStream_t s, const Args&... args) {
  static const hipError_t configured = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  if (configured != hipSuccess) MI355_FAIL((int)configured, "%s: cannot reserve %d B of LDS: %s", name, LDS_BYTES, hipGetErrorString(configured));
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), LDS_BYTES, s, args...);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
