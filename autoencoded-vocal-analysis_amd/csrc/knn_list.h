// The running neighbour lists of the kNN kernels: pj_knn_kernel, pj_knn_corr_kernel (projection.hip) and
// kp_knn_masked_kernel (knn_predict.hip).  A list is ordered by (distance, index), a strict total order, so the list
// for k' < k is the first k' slots of the list for k.  Device-only inline code.
#pragma once
#include "sqdist_tile.h"

#define PJ_DLD 65        // distance tile row stride (doubles)
#define PJ_MAX_K 64

// (d1, i1) before (d2, i2); an empty slot (i2 < 0) comes after everything
__device__ __forceinline__ bool pj_before(double d1, int i1, double d2, int i2) {
  if (i2 < 0) return true;
  return d1 < d2 || (d1 == d2 && i1 < i2);
}

// one thread folds the candidates of a distance tile's row (references r0 + c at distance row[c], c < cn, in reference
// order) into the running list of local query t (global row q): m slots ordered by (distance, index), slot s at
// [s * 64 + t]; with exclude_self reference q is skipped
__device__ __forceinline__ void pj_fold_tile(const double* row, int r0, int cn, int q, int exclude_self, int m,
                                             double* ld, int* li, int t) {
  double wd = ld[(m - 1) * SQD_T + t];
  int wi = li[(m - 1) * SQD_T + t];
  for (int c = 0; c < cn; ++c) {
    const int r = r0 + c;
    const double dd = row[c];
    if ((exclude_self && r == q) || !pj_before(dd, r, wd, wi)) continue;
    int s = m - 1;
    while (s > 0 && pj_before(dd, r, ld[(s - 1) * SQD_T + t], li[(s - 1) * SQD_T + t])) {
      ld[s * SQD_T + t] = ld[(s - 1) * SQD_T + t];
      li[s * SQD_T + t] = li[(s - 1) * SQD_T + t];
      --s;
    }
    ld[s * SQD_T + t] = dd;
    li[s * SQD_T + t] = r;
    wd = ld[(m - 1) * SQD_T + t];
    wi = li[(m - 1) * SQD_T + t];
  }
}

// the lists of local query t (global row q, output row orow) to the table: with exclude_self column 0 is the row itself
__device__ __forceinline__ void pj_write_list(size_t orow, int q, int k, int exclude_self, const double* ld,
                                              const int* li, int t, int64_t* __restrict__ out_idx,
                                              double* __restrict__ out_dist) {
  const size_t o = orow * k;
  const int m = k - exclude_self;
  if (exclude_self) {
    out_idx[o] = q;
    out_dist[o] = 0.0;
  }
  for (int s = 0; s < m; ++s) {
    out_idx[o + exclude_self + s] = li[s * SQD_T + t];
    out_dist[o + exclude_self + s] = ld[s * SQD_T + t];
  }
}
