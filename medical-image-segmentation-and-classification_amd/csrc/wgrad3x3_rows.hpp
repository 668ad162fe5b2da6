// The row-step program of the nine-tap 3x3 weight gradient (bf16 / fp16, gfx950), shared by the four-wave kernel
// (wgrad3x3_halo.hpp) and the eight-wave kernel (wgrad3x3_halo8.hpp).
//
//   dW[co][tap][ci] = sum_{n,y,x} dY[n,y,x,co] * X[n, y+kh-1, x+kw-1, ci]
//
// A wave owns a 32(co) x 32(ci) quadrant of a 64 x 64 tile of dW for ALL nine taps (2 x 2 MFMA blocks of 16x16, 144
// accumulator registers per lane) and a 32-pixel K block of every row segment; four waves share a K block.  Per row step a
// workgroup needs ONE new dY row segment and ONE new X row segment (a rolling window with a 1-pixel halo serves the nine
// shifted reads), so dY and X are streamed from L2 once per 36 MFMAs per wave.  Rows arrive by LDS-DMA (asm-issued, counted
// vmcnt, PF rows ahead into rings of NR rows); fragments are fetched with the hardware transpose read ds_read_b64_tr_b16
// from [pixel][64 ch] row images.  Nearest x2 up-sampling of X is folded into the row gather.
//
// What a kernel brings: a geometry (WgradRowsGeo), its (co0, ci0) tile, the zero image behind the rings, and the epilogue.
#pragma once
#include <type_traits>
#include <utility>
#include "common.hpp"
#include "dma.hpp"

struct Wgrad3Args {
  // up to six (x, dy) pairs of ONE shared convolution (the recurrent blocks apply a conv six times, R2AttU_Net.py:41-44):
  // their weight gradients are one sum, so the pairs are simply more work items of the same launch
  const void* xs[6];
  const void* dys[6];
  int items_per_app;             // work items of one pair
  float* ws;
  int N, Hi, Wi, Ci, ldx;        // physical X
  int H, W, Co, ldy;             // dY / logical X grid
  int up;
  int RB;                        // rows per work item (even)
  int items, items_per_block;
};

typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;

// Row geometry of a kernel.  WAVES / 4 K blocks of 32 pixels side by side make a dY row image; the X row image is XPX_ pixels
// with a 4-pixel halo in front.  PAIRED: the images are half a dY row wide and a "row" is row y of TWO images side by side
// (work item = image pair x row band): the X row image then holds two segments of SEG pixels (half a row + 4 + 4 halo each, so
// that the kw shifts of one image never read the other).  FIXED3: every wave moves three 1-KiB DMA pieces per row, the ones
// past the X row's end into the zero image (as zeros); otherwise a wave moves two or three and counts its own.
template <int WAVES_, bool PAIRED_, int XPX_, int NR_, int PF_, bool FIXED3_> struct WgradRowsGeo {
  static constexpr int WAVES = WAVES_, DPX = 8 * WAVES_, XPX = XPX_, NR = NR_, PF = PF_;
  static constexpr bool PAIRED = PAIRED_, FIXED3 = FIXED3_;
  static constexpr int IMGW = DPX / 2, SEG = IMGW + 8;
  static constexpr int XPIECES = (PAIRED ? 2 * SEG : DPX + 8) / 8;      // 1-KiB pieces per X row: waves 0 .. WAVES-1, then the first few again
  static constexpr int XROW = XPX * 128, DROW = DPX * 128;
  static constexpr int X_BYTES = NR * XROW, D_BYTES = NR * DROW, ZERO_IMG = X_BYTES + D_BYTES;
  static constexpr int LDS_BYTES = ZERO_IMG + 4096;                      // the rings and an all-zero K block of dY
  static_assert(XPIECES * 8 <= XPX && XPIECES <= 2 * WAVES, "an X row is at most two pieces per wave, inside its row image");
  static_assert(PF >= 3 && PF < NR && NR % 2 == 0, "row r + PF lands in the slot of a row <= r - 1; the X register sets swap per step");
  // RB in {8, 16, 32}: RB + 2 = 10 / 18 / 34 row steps = whole trips of NR and a tail, which finds the ring back at slot 0
  static constexpr int TAIL = 10 % NR;
  static_assert((18 % NR == 0 || 18 % NR == TAIL) && (34 % NR == 0 || 34 % NR == TAIL), "one tail length serves every band height");
  // pixel p of a dY row image -> image of the pair, and its pixel in the X row image (minus the 4-pixel halo)
  static __device__ __forceinline__ int img(int p) { return PAIRED ? p / IMGW : 0; }
  static __device__ __forceinline__ int xpx(int p) { return PAIRED ? (p / IMGW) * SEG + p % IMGW : p; }
};

// XOR on the 16-B chunk index of a pixel's 128-B line.  Operand map of the 16x16x32 MFMA: row (channel) = lane & 15,
// K = 8*(lane >> 4) .. +7, so one transpose read covers pixels 8*b + 0..3 (b = lane >> 4) of a 16-channel block and a wave
// instruction touches pixels {s..s+3, s+8..s+11, s+16.., s+24..}: the 32-B channel slot is XOR-ed with
// f(px) = bit1(px) | bit3(px) << 1, which keeps the four same-parity pixels of every 32-lane group in four distinct 32-B
// slots of the 256-B bank period for ANY pixel shift s (the three kw taps).
__device__ __forceinline__ int wgrad3_swz(int px) { return (((px >> 1) & 1) | (((px >> 3) & 1) << 1)) << 1; }

// MFMA fragment of pixels px .. px+3, px+4 .. px+7 x channels col .. col+3 of the row image at LDS byte `img_off`
__device__ __forceinline__ bf16x8 wgrad3_frag(unsigned char* lds, int img_off, int px, int col) {
  auto rd = [&](int p) {
    const int chunk = (col >> 3) ^ wgrad3_swz(p);
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(lds + img_off + p * 128 + chunk * 16 + (col & 7) * 2));
  };
  const s16x4 v0 = rd(px), v1 = rd(px + 4);
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <class F, int... S> __device__ __forceinline__ void wgrad3_steps(int r, F&& step, std::integer_sequence<int, S...>) {
  (step(r, std::integral_constant<int, S>{}), ...);
}

// All work items [by * items_per_block, ...) of one workgroup, accumulated into `acc` (tap, co block, ci block).
// A dY row meets three consecutive X rows (kh = 0, 1, 2), so its two fragments are read from LDS ONCE and ride a three-row
// register window; per row step only the six X fragments and two new dY fragments are read: 8 fragment reads per 36 MFMAs (a
// dY-row-major loop on 32x32x16 needed 20 per 18 twice as large ones and was 13 % slower).  A row step runs in three phases by
// tap column kw (12 MFMAs each), the X fragments of the next phase loading while the current one computes; the workgroup
// barrier sits between phases 1 and 2, so that the first fragments of the next row load behind phase 2.
template <typename T, class G>
__device__ __forceinline__ void wgrad3_rows(const Wgrad3Args& a, int co0, int ci0, int by, f32x4 (&acc)[9][2][2]) {
  static_assert(sizeof(T) == 2, "bf16 / fp16 only");
  constexpr int NR = G::NR, PF = G::PF, XROW = G::XROW, DROW = G::DROW, X_BYTES = G::X_BYTES, ZERO_IMG = G::ZERO_IMG;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const unsigned lds_x = lds_addr(lds), lds_d = lds_addr(lds + X_BYTES), lds_dump = lds_addr(lds + ZERO_IMG);      // DMA destinations: LDS byte addresses

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = G::WAVES > 4 ? wave >> 2 : 0, w4 = wave & 3;      // the wave's K block of the row, its quadrant of the tile
  const int l16 = lane & 15, c4 = lane >> 4;
  const int lpx = lane >> 3, slot = lane & 7;       // DMA: a 1-KiB piece = 8 pixels x 128 B; lane -> (pixel, 16-B slot)
  const int TXN = G::PAIRED ? 1 : a.W / G::DPX, BANDS = a.H / a.RB;
  const bool three = G::WAVES + wave < G::XPIECES;   // this wave's third piece of a row is real (wave-uniform)

  // transpose-read lane geometry: 16-lane block b = c4 reads pixels 8b + tq (+4), channels col0 + 4*tp .. +3
  const int tq = l16 >> 2, tp = l16 & 3;
  const int pl = 8 * c4 + tq;                      // this lane's first pixel inside its 32-pixel K block
  const int plx = G::xpx(32 * half + pl);          // ... and inside the X row image (minus the 4-pixel halo)
  const int dhalf = half * 32 * 128;               // byte offset of the K block inside a dY row image (32 | px: same swizzle)
  const int colA = (w4 >> 1) * 32 + 4 * tp, colB = (w4 & 1) * 32 + 4 * tp;     // + 16 * block

  const int item0 = by * a.items_per_block;
  const int item1 = min(a.items, item0 + a.items_per_block);
  for (int item = item0; item < item1; ++item) {
    const int app = item / a.items_per_app;
    const T* __restrict__ x = reinterpret_cast<const T*>(a.xs[app]);
    const T* __restrict__ dy = reinterpret_cast<const T*>(a.dys[app]);
    int t = item - app * a.items_per_app;
    const int band = t % BANDS; t /= BANDS;
    const int tx = t % TXN;
    const int n = t / TXN;
    const int ya = band * a.RB, yb = ya + a.RB, x0 = tx * G::DPX;
    const int nbase = G::PAIRED ? 2 * n : n;        // (PAIRED: `n` counts image pairs)
    // per-lane pixel geometry of this item, shared by the prologue rows and the running pointers below
    const int px_d = 8 * wave + lpx;                 // pixel of the dY row image
    const int c_d = co0 + 8 * (slot ^ wgrad3_swz(px_d));
    const bool lane_ok_d = c_d < a.Co;
    const int dpix = G::PAIRED ? G::img(px_d) * a.H * a.W + px_d % G::IMGW : x0 + px_d;      // pixel offset from (image nbase, row r, x 0)
    int xpix[2], c_x[2], xpiece[2];
    bool lane_ok_x[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      xpiece[k] = k == 0 ? wave : G::WAVES + wave;
      const int q = 8 * xpiece[k] + lpx;             // pixel of the X row image
      const int xx = G::PAIRED ? q % G::SEG - 4 : x0 - 4 + q;
      c_x[k] = ci0 + 8 * (slot ^ wgrad3_swz(q));
      lane_ok_x[k] = (k == 0 || three) && (unsigned)xx < (unsigned)a.W && c_x[k] < a.Ci;
      xpix[k] = (G::PAIRED ? q / G::SEG : 0) * a.Hi * a.Wi + (xx >> a.up);
    }

    // DMA sources: a buffer descriptor per tensor whose base is image `nbase` (wave-uniform), a scalar row offset, and ONE
    // 32-bit register per piece holding the lane's offset inside the row — or the always-out-of-range offset where the lane is
    // padding (image column / channel range), so that the hardware's range check writes the zeros; a row outside the image
    // (X) or the band (dY) takes a descriptor with num_records = 0.  Nothing per-lane is computed or selected per row.
    const bufdesc_t desc_d = make_buf(dy + (size_t)nbase * a.H * a.W * a.ldy);
    const bufdesc_t desc_x = make_buf(x + (size_t)nbase * a.Hi * a.Wi * a.ldx);
    const unsigned voff_d = lane_ok_d ? (unsigned)((dpix * a.ldy + c_d) * (int)sizeof(T)) : DMA_PAD;
    unsigned voff_x[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) voff_x[k] = lane_ok_x[k] ? (unsigned)((xpix[k] * a.ldx + c_x[k]) * (int)sizeof(T)) : DMA_PAD;
    const unsigned d_stride = (unsigned)(a.W * a.ldy) * (unsigned)sizeof(T), x_stride = (unsigned)(a.Wi * a.ldx) * (unsigned)sizeof(T);
    auto with_rows = [](bufdesc_t d, bool ok) { d[2] = ok ? (int)DMA_PAD : 0; return d; };
    // piece 0: this wave's KiB of dY row r; piece 1: its KiB of X row r; piece 2: its KiB of the X row's tail, if it has one
    // (FIXED3: or a KiB of zeros into the zero image — every wave issues the same count).  xs / ds: ring slots of X row r / dY row r
    auto issue_piece = [&](int piece, int r, unsigned d_soff, unsigned x_soff, int xs, int ds) {
      if (piece == 0) {
        dma16_buf(with_rows(desc_d, r >= ya && r < yb), voff_d, d_soff, lds_d + ds * DROW + wave * 1024);
      } else if (G::FIXED3 || piece == 1 || three) {
        const int k = piece - 1;
        dma16_buf(with_rows(desc_x, (unsigned)r < (unsigned)a.H), voff_x[k], x_soff,
                  k == 0 || three ? lds_x + xs * XROW + xpiece[k] * 1024 : lds_dump + wave * 1024);
      }
    };
    auto issue_row = [&](int r, int xs, int ds) {
#pragma unroll
      for (int piece = 0; piece < 3; ++piece)
        issue_piece(piece, r, (unsigned)r * d_stride, (unsigned)(r >> a.up) * x_stride, xs, ds);      // (r = -1: a dead offset under num_records = 0)
    };
    // at most K rows of this wave's pieces may still be in flight (a wave counts its own two or three pieces per row)
    auto wait_rows = [&](auto ktag) {
      constexpr int K = decltype(ktag)::value;
      if (G::FIXED3 || three) wait_vmcnt<3 * K>(); else wait_vmcnt<2 * K>();
    };
    // X fragments of tap column kw: [ci block]; dY fragments of a row: [co block]
    auto load_x = [&](int xs, int kw, bf16x8 (&bf)[2]) {
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) bf[bi] = wgrad3_frag(lds, xs * XROW, plx + 3 + kw, colB + 16 * bi);
    };
    auto load_dy = [&](int off, bf16x8 (&af)[2]) {
#pragma unroll
      for (int ao = 0; ao < 2; ++ao) af[ao] = wgrad3_frag(lds, off, pl, colA + 16 * ao);
    };
    bf16x8 dp[2], dc[2], dm[2], dn[2];              // dY rows r+1, r, r-1 (kh = 0, 1, 2) and the incoming r+2
    // twelve MFMAs of tap column kw; `between(kh)` runs behind the four MFMAs of tap row kh (a DMA piece rides there: in the
    // matrix pipe's shadow, one at a time — three back to back stall the pipe for their issue time)
    auto mfma12 = [&](int kw, const bf16x8 (&xk)[2], auto between) {
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
        for (int ao = 0; ao < 2; ++ao)
#pragma unroll
          for (int bi = 0; bi < 2; ++bi)
            mfma_16x16x32_acc<T>(kh == 0 ? dp[ao] : (kh == 1 ? dc[ao] : dm[ao]), xk[bi], acc[kh * 3 + kw][ao][bi]);
        between(kh);
      }
    };
    // The rows the main loop fetches are CONSECUTIVE (ya + 2, ya + 3, ...): their per-lane source pointers advance by a row
    // stride instead of being rebuilt from (n, r, x) with 64-bit multiplies each time, and the lane part of the bounds test
    // (channel / image-column range) is taken once per item; only the row part, wave-uniform, is evaluated per row.
    unsigned d_soff_next = (unsigned)(ya - 1 + PF) * d_stride, x_soff_next = (unsigned)((ya - 1 + PF) >> a.up) * x_stride;      // scalar registers
    int r_next = ya - 1 + PF;
    auto issue_next_piece = [&](int piece, int xs, int ds) {      // row r_next into ring slots xs / ds; the last piece advances
#ifndef WG3_T_NODMA                                            // (timing-only build: stale rows, the no-DMA ceiling of the loop)
      issue_piece(piece, r_next, d_soff_next, x_soff_next, xs, ds);
#endif
      if (piece == 2) {
        d_soff_next += d_stride;
        if (!a.up || (r_next & 1)) x_soff_next += x_stride;  // the source row of an up-sampled input advances every second row
        ++r_next;
      }
    };

    // ring slots: X row q -> (q - (ya-1)) mod NR, dY row q -> the same: X row q and dY row q share the slot index
#pragma unroll
    for (int k = 0; k < PF; ++k) issue_row(ya - 1 + k, k, k);
    wait_rows(std::integral_constant<int, PF - 3>{});          // rows ya - 1, ya, ya + 1 have landed
    __builtin_amdgcn_s_barrier();

    bf16x8 x0f[2], x1f[2];
    load_x(0, 0, x0f);
    load_dy(X_BYTES + DROW + dhalf, dp);           // r = ya-1: dY row ya is the only one of the window inside the band
    load_dy(ZERO_IMG, dc);
    load_dy(ZERO_IMG, dm);
    // One row step, of row r0 + S.  The ring slot S of the row is a COMPILE-TIME constant (NR step bodies per trip), so every LDS
    // offset of the step is an instruction immediate.  The two X register sets swap every step: `xa` holds X(r)[kw = 0]; on
    // return `xb` holds X(r+1)[kw = 0].
    auto row_step = [&](int r0, auto slot_tag) {
      constexpr int S = decltype(slot_tag)::value;
      const int r = r0 + S;
      bf16x8 (&xa)[2] = S % 2 == 0 ? x0f : x1f, (&xb)[2] = S % 2 == 0 ? x1f : x0f;
      // Row r + PF is fetched from inside the MFMA stream, always: past the band it brings zeros (a descriptor with no records:
      // no memory access) into ring slots that are dead by then, which keeps vmcnt uniform.  Its ring slot held row r - 1, whose
      // last reads returned before the barrier of step r - 1.
      constexpr int SN = (S + PF) % NR;
      auto none = [](int) {};
      load_x(S, 1, xb);                                       // the next tap column's fragments first, then this one's MFMAs
      __builtin_amdgcn_sched_barrier(0);
      mfma12(0, xa, [&](int kh) { if (kh < 2) issue_next_piece(kh, SN, SN); });
      load_x(S, 2, xa);
      __builtin_amdgcn_sched_barrier(0);
      mfma12(1, xb, [&](int kh) { if (kh == 0) issue_next_piece(2, SN, SN); });
      __builtin_amdgcn_sched_barrier(0);
#ifndef WG3_T_NOBARRIER                                        // (timing-only build: what the per-row synchronisation costs)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // every read of X row r has returned: its slot is reused by row r + NR
      wait_rows(std::integral_constant<int, PF - 2>{});       // rows <= r+2 have landed
      __builtin_amdgcn_s_barrier();
#endif
      const int on = r + 2 < yb ? X_BYTES + ((S + 2) % NR) * DROW + dhalf : ZERO_IMG;      // dY row r+2 (or the zero image)
      load_x((S + 1) % NR, 0, xb);                            // (past the last row: harmless reads, never used)
      load_dy(on, dn);
      __builtin_amdgcn_sched_barrier(0);
      mfma12(2, xa, none);
#pragma unroll
      for (int ao = 0; ao < 2; ++ao) {
        dm[ao] = dc[ao];
        dc[ao] = dp[ao];
        dp[ao] = dn[ao];
      }
    };
    int r = ya - 1;                                 // RB + 2 row steps: rows ya - 1 .. yb
    for (; r + NR - 1 <= yb; r += NR) wgrad3_steps(r, row_step, std::make_integer_sequence<int, NR>{});
    if (r <= yb) wgrad3_steps(r, row_step, std::make_integer_sequence<int, G::TAIL>{});
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vmcnt<0>();                               // (the trailing rows issued past the band)
    __builtin_amdgcn_s_barrier();                  // the next item's DMA overwrites the slots read last
  }
  mfma_results_ready();                              // (in-place asm MFMAs: the wait states in front of the stores' reads are ours)
}

// One 16 x 16 block (tap t, co block ao, ci block bi) of this wave's quadrant, to the slab `ws`, inside the channel ranges.
// C/D map of the MFMA: row = 4*(lane >> 4) + reg, col = lane & 15.
__device__ __forceinline__ void wgrad3_store_block(const Wgrad3Args& a, float* __restrict__ ws, int co0, int ci0, int t, int ao, int bi, const f32x4& v) {
  const int lane = threadIdx.x & 63, w4 = (threadIdx.x >> 6) & 3;
  const int ci = ci0 + (w4 & 1) * 32 + bi * 16 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = co0 + (w4 >> 1) * 32 + ao * 16 + 4 * (lane >> 4) + r;
    if (co < a.Co && ci < a.Ci) ws[((size_t)co * 9 + t) * a.Ci + ci] = v[r];
  }
}
