// Segmented stable argsort of fp32 keys: perm[s][k] = index within segment s of its k-th smallest key, the order of
// np.argsort(kind="stable") after -0 -> +0 (ascending as floats, equal keys in ascending index, the infinities in their natural
// places).  A least-significant-digit radix sort, four passes of 8 bits over the keys as order-preserving unsigned integers, the
// index travelling with its key.  Per pass:
//
//   segsort_hist_kernel      grid (tiles, S): the 256 digit counts of one tile of SEGSORT_TILE keys -> hist[s][digit][tile].  LDS
//                            integer adds: a count does not depend on their order.
//   segsort_rowscan_kernel   grid (256, S): row (s, digit) of hist becomes its exclusive prefix over the tiles, its sum goes to
//                            bintot[s][digit]
//   segsort_scatter_kernel   grid (tiles, S): every key of the tile gets its stable rank among the tile's keys of the same digit
//                            (below), the tile is put in digit order in LDS and leaves it as runs of consecutive addresses:
//                            position = (keys of smaller digits in the segment) + (same digit, earlier tiles) + (same digit, earlier
//                            in this tile)
//
// A segment of one tile (len <= SEGSORT_TILE) needs neither of the first two: the scatter kernel's own counts are the segment's.
//
// Stable by construction, no returning atomic anywhere.  Wave w of a tile owns the contiguous keys [512 w, 512 w + 512) and walks
// them 64 at a time; in a step, the lanes that hold the same digit find each other with eight ballots, their rank among themselves
// is a population count of the lower lanes, and the count of that digit in the wave's earlier steps is a per-wave LDS counter that
// the lowest of them advances.  Wave order, step order and lane order are index order, so equal digits keep their order — and an
// LSD sort of stable passes is stable.  The four waves' counters are then prefixed across waves by one thread per digit.
//
// Grids are functions of (S, len) alone, nothing is allocated, nothing synchronises, nothing is read back: a launch plan or a
// captured graph replays the sequence.  A NaN key is an unsigned integer like any other: unsupported as an order, but the result is
// still a permutation and nothing outside perm and ws is written.
#include "segsort.hpp"

#define SEGSORT_KPT (SEGSORT_TILE / 256)        /* keys per thread */
#define SEGSORT_WCHUNK (SEGSORT_TILE / 4)       /* contiguous keys of one wave */

// fp32 -> unsigned with the same order; both zeros become +0 first
__device__ __forceinline__ uint32_t segsort_key(float x) {
  uint32_t b = __builtin_bit_cast(uint32_t, x);
  if ((b << 1) == 0u) b = 0u;
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

template <bool FIRST> __device__ __forceinline__ uint32_t segsort_load(const void* __restrict__ kin, long long i) {
  if constexpr (FIRST) return segsort_key(static_cast<const float*>(kin)[i]);
  else return static_cast<const uint32_t*>(kin)[i];
}

__device__ __forceinline__ int segsort_wave_incl(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// exclusive prefix of v over the 256 threads of the workgroup, `total` = the sum; red = 4 ints of LDS, free again on return
__device__ __forceinline__ int segsort_block_excl(int v, int* red, int& total) {
  const int incl = segsort_wave_incl(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) red[w] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = red[q];
    base += q < w ? r : 0;
    tot += r;
  }
  __syncthreads();
  total = tot;
  return base + incl - v;
}

// grid (ntiles, S), 256 threads
template <bool FIRST>
__global__ __launch_bounds__(256) void segsort_hist_kernel(const void* __restrict__ kin, int len, int ntiles, int shift,
                                                           int* __restrict__ hist) {
  __shared__ int h[256];
  const int s = blockIdx.y, tile = blockIdx.x;
  const long long seg = (long long)s * len;
  const int t0 = tile * SEGSORT_TILE;
  h[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SEGSORT_KPT; ++j) {
    const int k = t0 + j * 256 + threadIdx.x;
    if (k < len) atomicAdd(&h[(segsort_load<FIRST>(kin, seg + k) >> shift) & 255u], 1);
  }
  __syncthreads();
  hist[((size_t)s * 256 + threadIdx.x) * ntiles + tile] = h[threadIdx.x];
}

// grid (gx, gy), 256 threads: row r = blockIdx.y * gx + blockIdx.x of n ints -> its exclusive prefix in place, totals[r] = its sum
__global__ __launch_bounds__(256) void segsort_rowscan_kernel(int* __restrict__ rows, int* __restrict__ totals, int n) {
  __shared__ int red[4];
  const size_t r = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  int* __restrict__ row = rows + r * n;
  int running = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < n ? row[i] : 0;
    int total;
    const int ex = segsort_block_excl(v, red, total);
    if (i < n) row[i] = running + ex;
    running += total;
  }
  if (threadIdx.x == 0) totals[r] = running;
}

// grid (ntiles, S), 256 threads.  FIRST: kin holds the fp32 keys and the value is the key's index; LAST: the keys are not written.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void segsort_scatter_kernel(const void* __restrict__ kin, const int* __restrict__ vin,
                                                              uint32_t* __restrict__ kout, int* __restrict__ vout,
                                                              const int* __restrict__ rowoff, const int* __restrict__ bintot,
                                                              int len, int ntiles, int shift) {
  __shared__ int cnt[4][256];                   // per wave: the digit's count so far, then its start among the tile's waves
  __shared__ int tstart[256];                   // the digit's start within the tile
  __shared__ int gbase[256];                    // the digit's start for this tile within the segment, minus tstart
  __shared__ int red[4];
  __shared__ uint32_t skey[SEGSORT_TILE];
  __shared__ int sval[SEGSORT_TILE];
  const int s = blockIdx.y, tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long seg = (long long)s * len;
  const int t0 = tile * SEGSORT_TILE;
  const int nvalid = len - t0 < SEGSORT_TILE ? len - t0 : SEGSORT_TILE;
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[q][tid] = 0;
  __syncthreads();

  uint32_t key[SEGSORT_KPT];
  int val[SEGSORT_KPT], off[SEGSORT_KPT];
  const unsigned long long lt = (1ull << lane) - 1ull;
  volatile int* wc = cnt[w];
#pragma unroll
  for (int j = 0; j < SEGSORT_KPT; ++j) {
    const int k = w * SEGSORT_WCHUNK + j * 64 + lane;
    const bool valid = k < nvalid;
    key[j] = valid ? segsort_load<FIRST>(kin, seg + t0 + k) : 0u;
    val[j] = FIRST ? t0 + k : (valid ? vin[seg + t0 + k] : 0);
    const unsigned d = (key[j] >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    off[j] = 0;
    if (valid) {
      const int prior = wc[d];
      off[j] = prior + __popcll(peers & lt);
      if ((peers & lt) == 0ull) wc[d] = prior + __popcll(peers);      // the lowest lane of the group; LDS serves a wave in order
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  // thread = digit: counts of the four waves -> starts across waves, the tile's count -> starts across digits
  int mine;
  {
    const int c0 = cnt[0][tid], c1 = cnt[1][tid], c2 = cnt[2][tid], c3 = cnt[3][tid];
    cnt[0][tid] = 0;
    cnt[1][tid] = c0;
    cnt[2][tid] = c0 + c1;
    cnt[3][tid] = c0 + c1 + c2;
    mine = c0 + c1 + c2 + c3;
  }
  int total;
  const int ts = segsort_block_excl(mine, red, total);
  int gb = ts;                                  // one tile: the tile's digit starts are the segment's
  if (ntiles > 1) {
    const int below = segsort_block_excl(bintot[(size_t)s * 256 + tid], red, total);
    gb = below + rowoff[((size_t)s * 256 + tid) * ntiles + tile];
  }
  tstart[tid] = ts;
  gbase[tid] = gb - ts;
  __syncthreads();

#pragma unroll
  for (int j = 0; j < SEGSORT_KPT; ++j) {
    const int k = w * SEGSORT_WCHUNK + j * 64 + lane;
    if (k < nvalid) {
      const unsigned d = (key[j] >> shift) & 255u;
      const int p = tstart[d] + cnt[w][d] + off[j];      // < nvalid: the counts are those of these very keys
      skey[p] = key[j];
      sval[p] = val[j];
    }
  }
  __syncthreads();
  for (int i = tid; i < nvalid; i += 256) {
    const uint32_t kq = skey[i];
    const int pos = gbase[(kq >> shift) & 255u] + i;      // < len: hist counted the same buffer with the same digit
    if constexpr (!LAST) kout[seg + pos] = kq;
    vout[seg + pos] = sval[i];
  }
}

long long segsort_ws_need(int S, long long len) {
  const long long n = (long long)S * len;
  const long long nt = segsort_ntiles(len);
  return 3 * n + (nt > 1 ? (long long)S * 256 * (nt + 1) : 0);
}

int segsort_rowscan_launch(int32_t* rows, int32_t* totals, int n, int gx, int gy, hipStream_t st) {
  hipLaunchKernelGGL(segsort_rowscan_kernel, dim3(gx, gy), dim3(256), 0, st, rows, totals, n);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ws = [K0 : n | K1 : n | V0 : n | hist : S 256 ntiles | bintot : S 256]; the values alternate between V0 and perm so that the
// fourth pass lands in perm.
int segsort_launch(const float* keys, int S, long long len, int32_t* ws, int32_t* perm, hipStream_t st) {
  const long long n = (long long)S * len;
  const int nt = segsort_ntiles(len);
  uint32_t* k0 = reinterpret_cast<uint32_t*>(ws);
  uint32_t* k1 = k0 + n;
  int* v0 = ws + 2 * n;
  int* hist = ws + 3 * n;
  int* bintot = hist + (size_t)S * 256 * nt;
  const dim3 grid(nt, S), block(256);
  const int L = (int)len;
  for (int p = 0; p < 4; ++p) {
    const int shift = 8 * p;
    const void* kin = p == 0 ? (const void*)keys : (const void*)((p & 1) ? k0 : k1);
    uint32_t* kout = (p & 1) ? k1 : k0;
    const int* vin = (p & 1) ? v0 : perm;
    int* vout = (p & 1) ? perm : v0;
    if (nt > 1) {
      if (p == 0) hipLaunchKernelGGL((segsort_hist_kernel<true>), grid, block, 0, st, kin, L, nt, shift, hist);
      else hipLaunchKernelGGL((segsort_hist_kernel<false>), grid, block, 0, st, kin, L, nt, shift, hist);
      MI355_LAUNCH_CHECK();
      const int rc = segsort_rowscan_launch(hist, bintot, nt, 256, S, st);
      if (rc != MI355_OK) return rc;
    }
    if (p == 0)
      hipLaunchKernelGGL((segsort_scatter_kernel<true, false>), grid, block, 0, st, kin, vin, kout, vout, hist, bintot, L, nt, shift);
    else if (p == 3)
      hipLaunchKernelGGL((segsort_scatter_kernel<false, true>), grid, block, 0, st, kin, vin, kout, vout, hist, bintot, L, nt, shift);
    else
      hipLaunchKernelGGL((segsort_scatter_kernel<false, false>), grid, block, 0, st, kin, vin, kout, vout, hist, bintot, L, nt, shift);
    MI355_LAUNCH_CHECK();
  }
  return MI355_OK;
}

#define SEGSORT_CHECK_SHAPE(who)                                                                                                  \
  MI355_CHECK_ARG(segsort_shape_ok(S, len), who ": 1 <= S <= %d, len >= 1 and S * len <= 2^26 expected (S=%d, len=%lld)",         \
                  SEGSORT_MAX_S, S, len)

extern "C" int mi355_segsort_tile(void) { return SEGSORT_TILE; }

extern "C" int mi355_segsort_ws_ints(int S, long long len) {
  SEGSORT_CHECK_SHAPE("segsort_ws_ints");
  return (int)segsort_ws_need(S, len);
}

extern "C" int mi355_segsort_f32(const float* keys, int S, long long len, int32_t* ws, long long ws_ints, int32_t* perm,
                                 mi355_stream_t s) {
  MI355_CHECK_ARG(keys, "segsort_f32: null pointer (keys)");
  MI355_CHECK_ARG(ws, "segsort_f32: null pointer (ws)");
  MI355_CHECK_ARG(perm, "segsort_f32: null pointer (perm)");
  SEGSORT_CHECK_SHAPE("segsort_f32");
  const long long need = segsort_ws_need(S, len);
  MI355_CHECK_ARG(ws_ints >= need, "segsort_f32: workspace ws of %lld int32 elements is too short, %lld needed (S=%d, len=%lld)",
                  ws_ints, need, S, len);
  return segsort_launch(keys, S, len, ws, perm, (hipStream_t)s);
}
