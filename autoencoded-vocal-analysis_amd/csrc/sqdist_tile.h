// The 64 x 64 fp64 squared-distance tile: direct differences sum_k (x_k - y_k)^2, no |x|^2 + |y|^2 - 2xy expansion
// (which cancels for near pairs).  Device-only inline code; every kernel keeps its own epilogue.
//   sqd_tile        the complete tile, staged from row-major operands: nn_eucl_kernel (neighbors.hip), pj_knn_kernel
//                   (projection.hip), ts_sqdist_kernel (tsne.hip); sil_sums_kernel (silhouette.hip) keeps the same
//                   loop written out, for the speed of its stage addressing (the comment there)
//   sqd_pair_tile   the tile of one matrix of rows against itself, or the entries of a precomputed matrix: db_count_kernel,
//                   db_union_kernel, db_border_kernel (dbscan.hip), hd_rowmin_kernel (hdbscan.hip)
//   sqd_stage, sqd_stage_rows, sqd_accumulate      the halves of a stage, for the kernels that stage whole rows at a
//                   stride of their own or through row lists: mmd_tile_sum of mmd_matrix_pair_kernel (mmd.hip),
//                   mmd_perm_stat_kernel (mmd_perm.hip)
//
// Order contract: every pair's sum starts at 0 and takes one fma(x_k - y_k, x_k - y_k, sum) per k, k ascending from 0
// to d - 1, whatever tile, stage or kernel the pair falls in.  So all these kernels give the same bits for the same
// pair of rows (and the bits of the scalar loops of pair_sqdist_kernel and hd_core_kernel), d2(i, j) and d2(j, i) have
// the same bits, and no result depends on the tiling.  mmd_perm_stat_kernel forms its tiles of exp(A d^2) from the same
// pieces, so its kernel values have the bits of mmd_tile_sum's; what it adds to the contract -- a column of K0 S
// depends on the latent rows, sigma and its membership vector only -- is stated in the header of mmd_perm.hip.
//
// Barrier contract of sqd_tile (and of sqd_pair_tile<T, false>): every stage is "barrier, write xs / ys, barrier,
// read xs / ys", and every thread of the workgroup must make the call.  So with d >= 1
//   - whatever the caller wrote to LDS before the call is visible to every thread after it;
//   - xs / ys may still be read by a thread that was slower when a faster one returns: every thread is past its last
//     WRITE of the buffers, not past the last READ.  A caller that writes them afterwards puts a barrier of its own
//     first; the next call needs none, it opens with one.
// sqd_pair_tile<T, true> touches no LDS and has no barrier.
//
// 256 threads; thread (ty, tx) = (t >> 4, t & 15) owns the pairs (ty + 16 i, tx + 16 j), i, j < 4.
#pragma once
#include <math.h>

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

// acc[i][j] = the squared distance of row q0 + ty + 16 i of Q (rows from qe on count as zero rows) and row
// r0 + tx + 16 j of R (from re on likewise); xs, ys: SQD_T * SQD_LD doubles of LDS each.  Barriers: the contract above.
template <typename TQ, typename TR>
__device__ __forceinline__ void sqd_tile(double* xs, double* ys, const TQ* __restrict__ Q, int q0, int qe,
                                         const TR* __restrict__ R, int r0, int re, int d, int t, double (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int k0 = 0; k0 < d; k0 += SQD_KC) {
    __syncthreads();                                                 // the stage before is consumed
    sqd_stage(xs, ys, Q, q0, qe, R, r0, re, d, k0, t);
    __syncthreads();
    sqd_accumulate(xs, ys, SQD_LD, d - k0 < SQD_KC ? d - k0 : SQD_KC, t >> 4, t & 15, acc);
  }
}

// acc[i][j] = the pair measure of the rows (q0 + ty + 16 i, r0 + tx + 16 j) of the n rows of X: their squared distance,
// or with PRE the entry of the n x n matrix X, INFINITY outside it.  Rows and columns from n on are not to be used by
// the caller.
template <typename T, bool PRE>
__device__ __forceinline__ void sqd_pair_tile(const T* __restrict__ X, int n, int d, int q0, int r0, double* xs,
                                              double* ys, int t, double (&acc)[4][4]) {
  if (PRE) {
    const int ty = t >> 4, tx = t & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = q0 + ty + 16 * i, c = r0 + tx + 16 * j;
        acc[i][j] = (r < n && c < n) ? (double)X[(size_t)r * n + c] : INFINITY;
      }
  } else {
    sqd_tile(xs, ys, X, q0, n, X, r0, n, d, t, acc);
  }
}
