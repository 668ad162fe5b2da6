// The decision steps shared by the joint-pipeline glue (head.hip: cls_decide, mask_scatter) and test-time augmentation (tta.hip:
// cls_tta_decide, tta_fold): the sigmoid, one row's softmax statistics and the in-order compaction of the kept samples.  One
// definition each, so that a one-view TTA is the plain decision bit for bit.
#pragma once
#include "common.hpp"

__device__ __forceinline__ float sigmoid_f32(float v) { return 1.f / (1.f + expf(-v)); }

// z[0..C): m = max, am = its first index (torch.max tie rule), den = sum_c expf(z[c] - m) in ascending c
__device__ __forceinline__ void softmax_row_stats(const float* __restrict__ z, int C, float& m, int& am, float& den) {
  m = z[0];
  am = 0;
  for (int c = 1; c < C; ++c)
    if (z[c] > m) { m = z[c]; am = c; }
  den = 0.f;
  for (int c = 0; c < C; ++c) den += expf(z[c] - m);
}

// One block of >= B threads, thread b holding `mine` (0 for b >= B): kept[0..n) = the b with mine != 0 in ascending order,
// n_kept[0] = n.  flag: 1024 ints of LDS.
__device__ __forceinline__ void compact_kept(int* flag, int b, int B, int mine, int32_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
  flag[b] = mine;
  __syncthreads();
  if (b == 0) {
    int n = 0;
    for (int i = 0; i < B; ++i)
      if (flag[i]) kept[n++] = i;
    n_kept[0] = n;
  }
}
