// What lovasz.hip shares with segsort.hip: the tile, the workspace size and the launch sequences (validated by the callers).
#pragma once
#include "common.hpp"

#define SEGSORT_TILE 2048                       /* keys one workgroup handles per pass: 256 threads x 8 */
#define SEGSORT_MAX_S 65535                     /* the segment index is a grid coordinate */
#define SEGSORT_MAX_N (1ll << 26)               /* S * len: every index and every count fits an int32 with room to spare */

static inline int segsort_ntiles(long long len) { return (int)((len + SEGSORT_TILE - 1) / SEGSORT_TILE); }
static inline bool segsort_shape_ok(int S, long long len) {
  return S >= 1 && S <= SEGSORT_MAX_S && len >= 1 && len <= SEGSORT_MAX_N && (long long)S * len <= SEGSORT_MAX_N;
}
long long segsort_ws_need(int S, long long len);

// keys [S][len] -> perm [S][len]; ws holds segsort_ws_need(S, len) int32 elements.  Launches only.
int segsort_launch(const float* keys, int S, long long len, int32_t* ws, int32_t* perm, hipStream_t st);
// rows[r][0 .. n) becomes its exclusive prefix sum in place, totals[r] the row's sum; grid = (gx, gy), r = blockIdx.y * gx + blockIdx.x.
int segsort_rowscan_launch(int32_t* rows, int32_t* totals, int n, int gx, int gy, hipStream_t st);
