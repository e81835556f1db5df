// The 64 x 64 fp64 squared-distance tile of nn_eucl_kernel (neighbors.hip), pj_knn_kernel (projection.hip) and
// mmd_pair_kernel (mmd.hip): direct differences sum_k (x_k - y_k)^2, no |x|^2 + |y|^2 - 2xy expansion (which cancels
// for near pairs).  Device-only inline pieces; the kernels keep their own barriers and epilogues.
//
// Order contract: every pair's sum starts at 0 and takes one fma(x_k - y_k, x_k - y_k, sum) per k, k ascending from 0
// to d - 1, whatever tile, stage or kernel the pair falls in.  So the three kernels give the same bits for the same
// pair of rows (and the bits of the scalar loop of pair_sqdist_kernel), and no result depends on the tiling.
// mmd_perm_stat_kernel (mmd_perm.hip) forms its tiles of exp(A d^2) from the same pieces (sqd_stage_rows), so its
// kernel values have the bits of mmd_pair_kernel's; what it adds to the contract -- a column of K0 S depends on the
// latent rows, sigma and its membership vector only -- is stated in the header of mmd_perm.hip.
//
// 256 threads; thread (ty, tx) = (t >> 4, t & 15) owns the pairs (ty + 16 i, tx + 16 j), i, j < 4.
#pragma once

#define SQD_T 64         // tile: x rows = y rows
#define SQD_KC 32        // columns per LDS stage
#define SQD_LD 33        // staging row stride in doubles (odd: the column walks spread over the banks)

// acc[i][j] += sum over kk < kn of (xs[ty + 16 i][kk] - ys[tx + 16 j][kk])^2, kk ascending; ld: row stride in doubles
__device__ __forceinline__ void sqd_accumulate(const double* xs, const double* ys, int ld, int kn, int ty, int tx,
                                               double (&acc)[4][4]) {
  for (int kk = 0; kk < kn; ++kk) {
    double x[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = xs[(ty + 16 * i) * ld + kk];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = ys[(tx + 16 * j) * ld + kk];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double df = x[i] - y[j];
        acc[i][j] = fma(df, df, acc[i][j]);
      }
  }
}

// the same stage gathered through row lists: row r of xs is row xrow[r] of L, row r of ys row yrow[r] (64 entries each,
// in LDS; a negative entry is a row that does not exist and is written as 0, like the columns from d on)
__device__ __forceinline__ void sqd_stage_rows(double* xs, double* ys, const double* __restrict__ L,
                                               const int64_t* xrow, const int64_t* yrow, int d, int k0, int t) {
  const int sc = t & 31, sr = t >> 5;
  const int k = k0 + sc;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = sr + 8 * j;
    const int64_t gx = xrow[r], gy = yrow[r];
    xs[r * SQD_LD + sc] = (k < d && gx >= 0) ? L[(size_t)gx * d + k] : 0.0;
    ys[r * SQD_LD + sc] = (k < d && gy >= 0) ? L[(size_t)gy * d + k] : 0.0;
  }
}

// one 64 x 32 stage of both operands as fp64: columns [k0, k0 + 32) of rows [q0, q0 + 64) of Q into xs and of rows
// [r0, r0 + 64) of R into ys (row stride SQD_LD); thread t writes rows (t >> 5) + 8 j of column t & 31.  Rows from
// qe / re on and columns from d on are written as 0.
template <typename TQ, typename TR>
__device__ __forceinline__ void sqd_stage(double* xs, double* ys, const TQ* __restrict__ Q, int q0, int qe,
                                          const TR* __restrict__ R, int r0, int re, int d, int k0, int t) {
  const int sc = t & 31, sr = t >> 5;
  const int k = k0 + sc;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = sr + 8 * j;
    xs[r * SQD_LD + sc] = (k < d && q0 + r < qe) ? (double)Q[(size_t)(q0 + r) * d + k] : 0.0;
    ys[r * SQD_LD + sc] = (k < d && r0 + r < re) ? (double)R[(size_t)(r0 + r) * d + k] : 0.0;
  }
}
