// Connected components of binary segmentation masks: labelling, hole filling, small-object removal, keep-largest-K and per-component
// area / bounding box / coordinate sums — every result an integer, equal to scipy.ndimage.label / binary_fill_holes / find_objects
// (tests/components_ref.py restates the definition, DESIGN.md "Connected components" gives it in words).
//
// A row of a mask is its 64-pixel ballot words; a RUN is a maximal stretch of set bits of a row (it may cross words), named by the
// linear index y W + x of its first pixel.  parent[] is a union-find forest over run names in which a link always goes from the larger
// root to the smaller one (atomicMin), so the root of a component is its smallest linear index — scipy's `first` — however the merges
// interleave.  Launches on the caller's stream, every one a barrier for the next, no workgroup ever waits for another:
//
//   cc_binarise_kernel   the expression of surface_on / seg_counts_kernel -> words of the mask and of its complement
//   cc_init_kernel       parent[s] = s at every run start
//   cc_merge_kernel      every run against the runs of the row above that it touches (widened by one pixel for 8-connectivity): one
//                        union per STRETCH of overlap, found with word arithmetic
//   cc_flatten_kernel    parent[s] = root at every run start; roots per row counted (labelling) or "touches the frame" marked on the
//                        root (hole filling)
//   cc_fill_kernel       background runs whose root does not touch the frame are or-ed into the mask (then init / merge / flatten again)
//   cc_scan_kernel       exclusive scan of the per-row root counts: component id = number of roots before it in raster order
//   cc_assign_kernel     parent[root] = -(id + 1), statistics of id reset
//   cc_stats_kernel      area, box and coordinate sums per component from the runs (integer atomics, which commute)
//   cc_select_kernel     one workgroup per sample: counts, the keep-largest threshold and the max_report leading components by a radix
//                        select on (area descending, id ascending), out_i and out_c
//   cc_mask_kernel       mask_out and labels_out
//
// Every find / union loop spends from a budget of a few H W steps and checks every index it follows; running out or leaving the
// sample sets the status word of out_i and ends the loop: a bug is a wrong answer, never a hang or a stray access.
#include "common.hpp"

#define CC_MAX_SIDE 1024
#define CC_MAX_B 65535        /* the sample index is a grid coordinate */
#define CC_MAX_REPORT 16
#define CC_HDR 16             /* ints per sample: [2] components, [3] status, [4] [5] the keep-largest threshold (area, id) */
#define CC_STATUS_BUDGET 1
#define CC_STATUS_INDEX 2
#define CC_STATUS_COUNT 4
typedef unsigned long long cc_word;

__device__ __forceinline__ bool cc_on(float v, int is_logit, float thr) {
  if (is_logit) v = 1.f / (1.f + __expf(-v));
  return v > thr;
}

// first pixel of the run that holds the set pixel x of a row
__device__ __forceinline__ int cc_run_start(const cc_word* __restrict__ row, int x) {
  int k = x >> 6;
  cc_word z = ~row[k] & ((2ull << (x & 63)) - 1ull);      // clear bits at or below x (2 << 63 wraps to 0: every bit)
  while (!z) {
    if (--k < 0) return 0;
    z = ~row[k];
  }
  return k * 64 + 64 - __builtin_clzll(z);
}

// last pixel of the run that holds the set pixel x (bits past W are clear)
__device__ __forceinline__ int cc_run_end(const cc_word* __restrict__ row, int WW, int x) {
  int k = x >> 6;
  cc_word z = ~row[k] & (~0ull << (x & 63));
  while (!z) {
    if (++k >= WW) return WW * 64 - 1;
    z = ~row[k];
  }
  return k * 64 + __builtin_ctzll(z) - 1;
}

__device__ __forceinline__ int cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of x with path halving.  Every write is an atomicMin with an ancestor, so parent[] only ever decreases towards the root.
__device__ int cc_find(int* __restrict__ P, int x, int N, int& budget, int* __restrict__ status) {
  while (budget-- > 0) {
    const int p = cc_ld(P + x);
    if ((unsigned)p >= (unsigned)N) {
      atomicOr(status, CC_STATUS_INDEX);
      return x;
    }
    if (p == x) return x;
    const int g = cc_ld(P + p);
    if ((unsigned)g >= (unsigned)N) {
      atomicOr(status, CC_STATUS_INDEX);
      return x;
    }
    if (g == p) return p;
    atomicMin(P + x, g);
    x = g;
  }
  atomicOr(status, CC_STATUS_BUDGET);
  return x;
}

// The larger root is linked to the smaller.  A root that stopped being one between the find and the atomicMin hands back its new
// parent, and the union goes on from there: no link is lost.
__device__ void cc_union(int* __restrict__ P, int a, int b, int N, int* __restrict__ status) {
  int budget = 4 * N + 64;
  while (budget-- > 0) {
    a = cc_find(P, a, N, budget, status);
    b = cc_find(P, b, N, budget, status);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(P + a, b);
    if (old == a) return;
    if ((unsigned)old >= (unsigned)N) {
      atomicOr(status, CC_STATUS_INDEX);
      return;
    }
    a = old;
  }
  atomicOr(status, CC_STATUS_BUDGET);
}

// The three kernels below and cc_fill / cc_stats / cc_mask: grid (ceil(WW / 4), H, B), 256 threads, one wave per 64-pixel word.
__global__ __launch_bounds__(256) void cc_binarise_kernel(const float* __restrict__ src, int H, int W, int WW, int is_logit, float thr,
                                                          cc_word* __restrict__ bits_f, cc_word* __restrict__ bits_i,
                                                          int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6), y = blockIdx.y, b = blockIdx.z;
  if (blockIdx.x == 0 && y == 0 && threadIdx.x < CC_HDR) hdr[(size_t)b * CC_HDR + threadIdx.x] = 0;
  if (wi >= WW) return;
  const int x = wi * 64 + lane;
  const float v = src[((size_t)b * H + y) * W + (x < W ? x : W - 1)];      // (a clamped address, not a load under a condition)
  const bool on = x < W && cc_on(v, is_logit, thr);
  const cc_word m = __ballot(on), valid = __ballot(x < W);
  if (lane == 0) {
    const size_t o = ((size_t)b * H + y) * WW + wi;
    bits_f[o] = m;
    bits_i[o] = ~m & valid;
  }
}

__device__ __forceinline__ cc_word cc_starts(const cc_word* __restrict__ row, int wi) {
  const cc_word m = row[wi], prev = wi > 0 ? row[wi - 1] : 0ull;
  return m & ~((m << 1) | (prev >> 63));
}

template <bool HOLES>
__global__ __launch_bounds__(256) void cc_init_kernel(const cc_word* __restrict__ bits, int H, int W, int WW, int* __restrict__ parent,
                                                      int* __restrict__ flag) {
  const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6), y = blockIdx.y, b = blockIdx.z;
  if (wi >= WW) return;
  const cc_word starts = cc_starts(bits + ((size_t)b * H + y) * WW, wi);
  if ((starts >> lane) & 1ull) {
    const int s = y * W + wi * 64 + lane;
    parent[(size_t)b * H * W + s] = s;
    if (HOLES) flag[(size_t)b * H * W + s] = 0;
  }
}

// m = this row, u = the row above, L / R = the same rows seen from one pixel to the left / right.  A union is needed where a stretch
// of vertical overlap begins; for 8-connectivity also where a pixel with nothing above it has a pixel above-left (above-right) that
// the stretch ending (beginning) next to it does not already join to this run.
__global__ __launch_bounds__(256) void cc_merge_kernel(const cc_word* __restrict__ bits, int H, int W, int WW, int conn,
                                                       int* __restrict__ parent, int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6), y = blockIdx.y, b = blockIdx.z;
  if (wi >= WW || y == 0) return;
  const cc_word* __restrict__ row = bits + ((size_t)b * H + y) * WW;
  const cc_word* __restrict__ up = row - WW;
  const cc_word m = row[wi], u = up[wi];
  const cc_word mp = wi > 0 ? row[wi - 1] : 0ull, mn = wi + 1 < WW ? row[wi + 1] : 0ull;
  const cc_word upv = wi > 0 ? up[wi - 1] : 0ull, un = wi + 1 < WW ? up[wi + 1] : 0ull;
  const cc_word mL = (m << 1) | (mp >> 63), mR = (m >> 1) | (mn << 63);
  const cc_word uL = (u << 1) | (upv >> 63), uR = (u >> 1) | (un << 63);
  const cc_word vert = m & u & ~(mL & uL);
  const cc_word dl = conn == 8 ? (m & ~u & uL & ~mL) : 0ull;
  const cc_word dr = conn == 8 ? (m & ~u & uR & ~mR) : 0ull;
  if (!(((vert | dl | dr) >> lane) & 1ull)) return;
  const int N = H * W, x = wi * 64 + lane;
  int* __restrict__ P = parent + (size_t)b * N;
  int* __restrict__ status = hdr + (size_t)b * CC_HDR + 3;
  const int a = y * W + cc_run_start(row, x);
  if ((vert >> lane) & 1ull) cc_union(P, a, (y - 1) * W + cc_run_start(up, x), N, status);
  if ((dl >> lane) & 1ull) cc_union(P, a, (y - 1) * W + cc_run_start(up, x - 1), N, status);
  if ((dr >> lane) & 1ull) cc_union(P, a, (y - 1) * W + cc_run_start(up, x + 1), N, status);
}

// grid (H, B), 256 threads: the waves share the words of one row
template <bool HOLES>
__global__ __launch_bounds__(256) void cc_flatten_kernel(const cc_word* __restrict__ bits, int H, int W, int WW, int* __restrict__ parent,
                                                         int* __restrict__ flag, int* __restrict__ rowcnt, int* __restrict__ hdr) {
  __shared__ int cnt_s[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, y = blockIdx.x, b = blockIdx.y;
  const int N = H * W;
  const cc_word* __restrict__ row = bits + ((size_t)b * H + y) * WW;
  int* __restrict__ P = parent + (size_t)b * N;
  int* __restrict__ status = hdr + (size_t)b * CC_HDR + 3;
  int cnt = 0;
  for (int wi = wave; wi < WW; wi += 4) {
    const cc_word starts = cc_starts(row, wi);
    bool root = false;
    if ((starts >> lane) & 1ull) {
      const int x = wi * 64 + lane, s = y * W + x;
      int budget = 2 * N + 64;
      const int r = cc_find(P, s, N, budget, status);
      atomicMin(P + s, r);
      root = r == s;
      if (HOLES && (y == 0 || y == H - 1 || x == 0 || cc_run_end(row, WW, x) == W - 1)) flag[(size_t)b * N + r] = 1;
    }
    cnt += __popcll(__ballot(root));
  }
  if (!HOLES) {
    if (lane == 0) cnt_s[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) rowcnt[(size_t)b * H + y] = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
  }
}

__global__ __launch_bounds__(256) void cc_fill_kernel(const cc_word* __restrict__ bits_i, int H, int W, int WW,
                                                      const int* __restrict__ parent, const int* __restrict__ flag,
                                                      cc_word* __restrict__ bits_f, int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6), y = blockIdx.y, b = blockIdx.z;
  if (wi >= WW) return;
  const int N = H * W;
  const cc_word* __restrict__ row = bits_i + ((size_t)b * H + y) * WW;
  bool fill = false;
  if ((row[wi] >> lane) & 1ull) {
    const int r = parent[(size_t)b * N + y * W + cc_run_start(row, wi * 64 + lane)];
    if ((unsigned)r < (unsigned)N) fill = flag[(size_t)b * N + r] == 0;
    else atomicOr(hdr + (size_t)b * CC_HDR + 3, CC_STATUS_INDEX);
  }
  const cc_word add = __ballot(fill);
  if (lane == 0 && add) bits_f[((size_t)b * H + y) * WW + wi] |= add;
}

// grid (B), 1024 threads (H <= 1024: one row per thread)
__global__ __launch_bounds__(1024) void cc_scan_kernel(int H, int* __restrict__ rowcnt, int* __restrict__ hdr) {
  __shared__ int buf[1024];
  const int t = threadIdx.x, b = blockIdx.x;
  const int v = t < H ? rowcnt[(size_t)b * H + t] : 0;
  buf[t] = v;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int a = t >= o ? buf[t - o] : 0;
    __syncthreads();
    buf[t] += a;
    __syncthreads();
  }
  if (t < H) rowcnt[(size_t)b * H + t] = buf[t] - v;
  if (t == 1023) hdr[(size_t)b * CC_HDR + 2] = buf[1023];
}

// grid (H, B), 64 threads: one wave walks its row from the left.  stats = [area | first | y0 | x0 | y1 | x1 | sum_y | sum_x], C each.
__global__ __launch_bounds__(64) void cc_assign_kernel(const cc_word* __restrict__ bits, int H, int W, int WW, int C,
                                                       int* __restrict__ parent, const int* __restrict__ rowbase, int* __restrict__ stats,
                                                       int* __restrict__ hdr) {
  const int lane = threadIdx.x, y = blockIdx.x, b = blockIdx.y;
  const int N = H * W;
  const cc_word* __restrict__ row = bits + ((size_t)b * H + y) * WW;
  int* __restrict__ P = parent + (size_t)b * N;
  int* __restrict__ S = stats + (size_t)b * 8 * C;
  int base = rowbase[(size_t)b * H + y];
  for (int wi = 0; wi < WW; ++wi) {
    const cc_word starts = cc_starts(row, wi);
    const int s = y * W + wi * 64 + lane;
    const bool root = ((starts >> lane) & 1ull) && P[s] == s;
    const cc_word bal = __ballot(root);
    if (root) {
      const int id = base + __popcll(bal & ((1ull << lane) - 1ull));
      if (id < C) {
        P[s] = -(id + 1);
        S[id] = 0;
        S[C + id] = s;
        S[2 * C + id] = H;
        S[3 * C + id] = W;
        S[4 * C + id] = -1;
        S[5 * C + id] = -1;
        S[6 * C + id] = 0;
        S[7 * C + id] = 0;
      } else {
        atomicOr(hdr + (size_t)b * CC_HDR + 3, CC_STATUS_COUNT);
      }
    }
    base += __popcll(bal);
  }
}

// component id of the run that starts at s, -1 (and the status word) if the forest does not say
__device__ __forceinline__ int cc_id_of(const int* __restrict__ P, int s, int N, int C, int* __restrict__ status) {
  int p = P[s];
  if (p >= 0) p = p < N ? P[p] : 0;
  const int id = -p - 1;
  if ((unsigned)id >= (unsigned)C) {
    atomicOr(status, CC_STATUS_INDEX);
    return -1;
  }
  return id;
}

__global__ __launch_bounds__(256) void cc_stats_kernel(const cc_word* __restrict__ bits, int H, int W, int WW, int C,
                                                       const int* __restrict__ parent, int* __restrict__ stats, int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6), y = blockIdx.y, b = blockIdx.z;
  if (wi >= WW) return;
  const cc_word* __restrict__ row = bits + ((size_t)b * H + y) * WW;
  if (!((cc_starts(row, wi) >> lane) & 1ull)) return;
  const int N = H * W, x0 = wi * 64 + lane;
  const int id = cc_id_of(parent + (size_t)b * N, y * W + x0, N, C, hdr + (size_t)b * CC_HDR + 3);
  if (id < 0) return;
  const int x1 = cc_run_end(row, WW, x0), len = x1 - x0 + 1;
  int* __restrict__ S = stats + (size_t)b * 8 * C;
  atomicAdd(S + id, len);
  atomicMin(S + 2 * C + id, y);
  atomicMin(S + 3 * C + id, x0);
  atomicMax(S + 4 * C + id, y);
  atomicMax(S + 5 * C + id, x1);
  atomicAdd(S + 6 * C + id, y * len);
  atomicAdd(S + 7 * C + id, (x0 + x1) * len / 2);      // x0 + ... + x1
}

__device__ __forceinline__ int cc_block_sum(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < 16; ++w) t += red[w];
  return t;
}
__device__ __forceinline__ int cc_block_max(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = red[0];
  for (int w = 1; w < 16; ++w) t = max(t, red[w]);
  return t;
}

// The K-th (1 <= K <= n) component in the order (area descending, id ascending): its area and its id.  A radix select, eight bits a
// sweep from the top of a 24-bit key, first on the area, then on the id among the components of that area (LDS histograms filled with
// integer atomics, which commute): no component is compared with another.  Called by the whole workgroup with uniform arguments.
__device__ void cc_select(const int* __restrict__ area, int n, int K, int* hist, int* bc, int& A, int& I) {
  int prefix = 0, before = 0;
  for (int shift = 16; shift >= 0; shift -= 8) {
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) {
      const int a = area[i];
      if (shift == 16 || (a >> (shift + 8)) == prefix) atomicAdd(&hist[(a >> shift) & 255], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = before, bin = 255;
      for (; bin > 0; --bin) {
        if (acc + hist[bin] >= K) break;
        acc += hist[bin];
      }
      bc[0] = bin;
      bc[1] = acc;
    }
    __syncthreads();
    prefix = (prefix << 8) | bc[0];
    before = bc[1];
    __syncthreads();
  }
  A = prefix;
  const int T = K - before;      // the T-th smallest id among the components of area A
  prefix = 0;
  before = 0;
  for (int shift = 16; shift >= 0; shift -= 8) {
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024)
      if (area[i] == A && (shift == 16 || (i >> (shift + 8)) == prefix)) atomicAdd(&hist[(i >> shift) & 255], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = before, bin = 0;
      for (; bin < 255; ++bin) {
        if (acc + hist[bin] >= T) break;
        acc += hist[bin];
      }
      bc[0] = bin;
      bc[1] = acc;
    }
    __syncthreads();
    prefix = (prefix << 8) | bc[0];
    before = bc[1];
    __syncthreads();
  }
  I = prefix;
}

__device__ __forceinline__ bool cc_leads(int a, int i, int A, int I) { return a > A || (a == A && i <= I); }

// grid (B), 1024 threads
__global__ __launch_bounds__(1024) void cc_select_kernel(const cc_word* __restrict__ bits_f, const cc_word* __restrict__ bits_i, int H, int W,
                                                         int WW, int C, const int* __restrict__ stats, int min_area, int keep_largest,
                                                         int max_report, int* __restrict__ hdr, int* __restrict__ out_i,
                                                         int* __restrict__ out_c) {
  __shared__ int red[16];
  __shared__ int hist[256];
  __shared__ int bc[2];
  __shared__ int sel[CC_MAX_REPORT];
  __shared__ int nsel;
  const int b = blockIdx.x, N = H * W;
  const int* __restrict__ S = stats + (size_t)b * 8 * C;
  int* __restrict__ hd = hdr + (size_t)b * CC_HDR;
  const int n = min(max(hd[2], 0), C);
  const cc_word* __restrict__ bf = bits_f + (size_t)b * H * WW;
  const cc_word* __restrict__ bi = bits_i + (size_t)b * H * WW;
  int cf = 0, ci = 0;
  for (int i = threadIdx.x; i < H * WW; i += 1024) {
    cf += __popcll(bf[i]);
    ci += __popcll(bi[i]);
  }
  const int fg_filled = cc_block_sum(cf, red);
  const int fg_thr = N - cc_block_sum(ci, red);
  int largest = 0;
  for (int i = threadIdx.x; i < n; i += 1024) largest = max(largest, S[i]);
  largest = cc_block_max(largest, red);
  // keep-largest: the keep_largest leading components of the order; -1 = every component leads
  int A = -1, I = 0;
  if (keep_largest > 0 && keep_largest < n) cc_select(S, n, keep_largest, hist, bc, A, I);
  int kept = 0, kept_px = 0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const int a = S[i];
    if (a >= min_area && cc_leads(a, i, A, I)) {
      ++kept;
      kept_px += a;
    }
  }
  kept = cc_block_sum(kept, red);
  kept_px = cc_block_sum(kept_px, red);
  // the kept components are a prefix of the order (both conditions are), so its first R entries are the rows to report
  const int R = min(kept, max_report);
  if (threadIdx.x == 0) nsel = 0;
  if (R > 0) {
    int A2 = -1, I2 = 0;
    if (R < n) cc_select(S, n, R, hist, bc, A2, I2);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) {
      if (cc_leads(S[i], i, A2, I2)) {
        const int k = atomicAdd(&nsel, 1);
        if (k < CC_MAX_REPORT) sel[k] = i;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {      // at most 16 entries, gathered in any order: sorted here
      const int m = min(nsel, CC_MAX_REPORT);
      for (int i = 1; i < m; ++i) {
        const int v = sel[i], av = S[v];
        int j = i - 1;
        for (; j >= 0 && (S[sel[j]] < av || (S[sel[j]] == av && sel[j] > v)); --j) sel[j + 1] = sel[j];
        sel[j + 1] = v;
      }
      if (m != R) atomicOr(hd + 3, CC_STATUS_COUNT);
    }
  }
  __syncthreads();
  const int rows = min(R, min(nsel, CC_MAX_REPORT));
  if ((int)threadIdx.x < max_report * 8) {
    const int r = threadIdx.x >> 3, c = threadIdx.x & 7;
    out_c[(size_t)b * max_report * 8 + threadIdx.x] = r < rows ? S[c * C + sel[r]] : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    hd[4] = A;
    hd[5] = I;
    int* __restrict__ o = out_i + (size_t)b * 8;
    o[0] = fg_thr;
    o[1] = fg_filled - fg_thr;
    o[2] = n;
    o[3] = kept;
    o[4] = kept_px;
    o[5] = largest;
    o[6] = R;
    o[7] = hd[3];
  }
}

__global__ __launch_bounds__(256) void cc_mask_kernel(const cc_word* __restrict__ bits, int H, int W, int WW, int C,
                                                      const int* __restrict__ parent, const int* __restrict__ stats, int min_area,
                                                      int* __restrict__ hdr, uint8_t* __restrict__ mask_out, int* __restrict__ labels_out) {
  const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6), y = blockIdx.y, b = blockIdx.z;
  const int x = wi * 64 + lane;
  if (x >= W) return;
  const int N = H * W;
  const cc_word* __restrict__ row = bits + ((size_t)b * H + y) * WW;
  int label = 0;
  bool keep = false;
  if ((row[wi] >> lane) & 1ull) {
    const int* __restrict__ hd = hdr + (size_t)b * CC_HDR;
    const int id = cc_id_of(parent + (size_t)b * N, y * W + cc_run_start(row, x), N, C, hdr + (size_t)b * CC_HDR + 3);
    if (id >= 0) {
      const int a = stats[(size_t)b * 8 * C + id];
      label = id + 1;
      keep = a >= min_area && cc_leads(a, id, hd[4], hd[5]);
    }
  }
  const size_t o = (size_t)b * N + (size_t)y * W + x;
  mask_out[o] = keep ? (uint8_t)255 : (uint8_t)0;
  if (labels_out) labels_out[o] = label;
}

// ws = [hdr: B 16][row counts: B H][mask words: B H WW x 2][complement words: the same][parent: B H W][stats: B 8 C], every part a
// multiple of four ints.  C = (H W + 1) / 2 + 1 bounds the components of a sample (4-connectivity, checkerboard); during hole filling
// the statistics part (8 C >= 4 H W) holds the "touches the frame" word per pixel.
struct cc_layout {
  long long rowcnt, bits_f, bits_i, parent, stats, total;
  int WW, C;
};
static cc_layout cc_layout_of(int B, int H, int W) {
  const auto up4 = [](long long v) { return (v + 3) & ~3LL; };
  cc_layout L;
  const long long n = (long long)B * H * W;
  L.WW = (W + 63) / 64;
  L.C = (H * W + 1) / 2 + 1;
  L.rowcnt = up4((long long)B * CC_HDR);
  L.bits_f = L.rowcnt + up4((long long)B * H);
  L.bits_i = L.bits_f + up4((long long)B * H * L.WW * 2);
  L.parent = L.bits_i + up4((long long)B * H * L.WW * 2);
  L.stats = L.parent + up4(n);
  L.total = L.stats + up4((long long)B * 8 * L.C);
  return L;
}

#define CC_CHECK_SHAPE(who)                                                                                              \
  MI355_CHECK_ARG(B > 0 && B <= CC_MAX_B && H >= 1 && H <= CC_MAX_SIDE && W >= 1 && W <= CC_MAX_SIDE &&                   \
                      cc_layout_of(B > 0 ? B : 1, H, W).total <= 0x7fffffffLL,                                            \
                  who ": 1 <= H, W <= %d, 0 < B <= %d and a workspace below 2^31 elements expected (B=%d, H=%d, W=%d)",   \
                  CC_MAX_SIDE, CC_MAX_B, B, H, W)

extern "C" int mi355_components_ws_ints(int B, int H, int W) {
  CC_CHECK_SHAPE("components_ws_ints");
  return (int)cc_layout_of(B, H, W).total;
}

template <bool HOLES>
static int cc_label(const cc_word* bits, int B, int H, int W, int WW, int conn, int* parent, int* flag, int* rowcnt, int* hdr,
                    hipStream_t st) {
  const dim3 words((WW + 3) / 4, H, B);
  hipLaunchKernelGGL(cc_init_kernel<HOLES>, words, dim3(256), 0, st, bits, H, W, WW, parent, flag);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_merge_kernel, words, dim3(256), 0, st, bits, H, W, WW, conn, parent, hdr);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel<HOLES>, dim3(H, B), dim3(256), 0, st, bits, H, W, WW, parent, flag, rowcnt, hdr);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_components(const float* src, int B, int H, int W, int is_logit, float thr, int connectivity, int fill_holes,
                                int min_area, int keep_largest, int max_report, int32_t* ws, long long ws_ints, uint8_t* mask_out,
                                int32_t* labels_out, int32_t* out_i, int32_t* out_c, mi355_stream_t s) {
  MI355_CHECK_ARG(src && ws && mask_out && out_i && (out_c || max_report == 0), "components: null pointer");
  CC_CHECK_SHAPE("components");
  MI355_CHECK_ARG(connectivity == 4 || connectivity == 8, "components: connectivity=%d, 4 or 8 expected", connectivity);
  MI355_CHECK_ARG(fill_holes == 0 || fill_holes == 4 || fill_holes == 8, "components: fill_holes=%d, 0, 4 or 8 expected", fill_holes);
  MI355_CHECK_ARG(max_report >= 0 && max_report <= CC_MAX_REPORT, "components: max_report=%d outside 0..%d", max_report, CC_MAX_REPORT);
  MI355_CHECK_ARG(min_area >= 0 && keep_largest >= 0, "components: min_area=%d and keep_largest=%d must not be negative", min_area,
                  keep_largest);
  const cc_layout L = cc_layout_of(B, H, W);
  MI355_CHECK_ARG(ws_ints >= L.total, "components: workspace of %lld int32 elements is too short, %lld needed (B=%d, H=%d, W=%d)", ws_ints,
                  L.total, B, H, W);
  MI355_CHECK_ARG(((uintptr_t)ws % 16) == 0, "components: ws must be 16-byte aligned");
  int* hdr = ws;
  int* rowcnt = ws + L.rowcnt;
  cc_word* bits_f = reinterpret_cast<cc_word*>(ws + L.bits_f);
  cc_word* bits_i = reinterpret_cast<cc_word*>(ws + L.bits_i);
  int* parent = ws + L.parent;
  int* stats = ws + L.stats;
  const int WW = L.WW, C = L.C;
  const dim3 words((WW + 3) / 4, H, B);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(cc_binarise_kernel, words, dim3(256), 0, st, src, H, W, WW, is_logit ? 1 : 0, thr, bits_f, bits_i, hdr);
  MI355_LAUNCH_CHECK();
  if (fill_holes) {
    // the same labelling on the complement under the structure of the fill; a background component is a hole unless it touches the frame
    const int rc = cc_label<true>(bits_i, B, H, W, WW, fill_holes, parent, stats, rowcnt, hdr, st);
    if (rc != MI355_OK) return rc;
    hipLaunchKernelGGL(cc_fill_kernel, words, dim3(256), 0, st, bits_i, H, W, WW, parent, stats, bits_f, hdr);
    MI355_LAUNCH_CHECK();
  }
  const int rc = cc_label<false>(bits_f, B, H, W, WW, connectivity, parent, stats, rowcnt, hdr, st);
  if (rc != MI355_OK) return rc;
  hipLaunchKernelGGL(cc_scan_kernel, dim3(B), dim3(1024), 0, st, H, rowcnt, hdr);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_assign_kernel, dim3(H, B), dim3(64), 0, st, bits_f, H, W, WW, C, parent, rowcnt, stats, hdr);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_stats_kernel, words, dim3(256), 0, st, bits_f, H, W, WW, C, parent, stats, hdr);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_select_kernel, dim3(B), dim3(1024), 0, st, bits_f, bits_i, H, W, WW, C, stats, min_area, keep_largest, max_report,
                     hdr, out_i, out_c);
  MI355_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_mask_kernel, words, dim3(256), 0, st, bits_f, H, W, WW, C, parent, stats, min_area, hdr, mask_out, labels_out);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
