// The fp64 correlation tile of nn_corr_kernel (neighbors.hip) and pj_knn_corr_kernel (projection.hip): the row
// statistics, the centred staging and the v_mfma_f64_16x16x4_f64 stage of the centred dot products.  scipy's
// correlation distance centres both operands and takes the cosine distance of the centred rows; the dot products here
// are of the centred values, never sum(uv) - d u v, which cancels for the near-constant rows real spectrograms have.
// Device-only inline pieces; the kernels keep their own barriers, tile shapes and epilogues.
//
// Order contract:
//   statistics  stats[2 r] is the fp64 mean of row r, stats[2 r + 1] its centred sum of squares sum_k (x_k - mean)^2,
//               each a fixed-order two-stage sum: thread t of 256 takes k = t, t + 256, ... ascending (the squares
//               by fma), a wave butterfly (wave_sum_d), then (w0 + w1) + (w2 + w3)
//   centring    an operand is converted to fp64 and its row's mean subtracted as it is written into LDS; rows and
//               columns of padding are exactly 0
//   dot         every pair's sum starts at 0 and takes its k in one ascending walk of 4-wide MFMA steps from k = 0
//               (stage after stage, step after step), whatever tile, stage or kernel the pair falls in
// So both kernels give the same bits for the same pair of rows, and no result depends on the tiling.
// mmd_perm_stat_kernel (mmd_perm.hip) uses corr_mfma_stage alone, for K0 S (kernel values times 0 / 1 membership
// columns): the dot line above is what makes a column's value independent of its place in a tile and of the other
// columns (the contract in the header of mmd_perm.hip).
//
// 256 threads.  A stage holds CORR_KC columns of ROWS rows (ROWS a multiple of 16) of each operand, row stride CORR_LD;
// element t + 256 j of a stage is row (t >> 4) + 16 j, column t & 15.
#pragma once

#define CORR_KC 16       // k per LDS stage
#define CORR_LD 17       // LDS row stride in doubles (odd: the staging writes and fragment reads spread over the banks)

typedef double corr_d4 __attribute__((ext_vector_type(4)));

// mean and centred sum of squares of one row of d values, by one workgroup of 256 threads; red: 4 doubles of LDS.
// Thread 0 writes out[0] = mean, out[1] = sum of squares.
template <typename T>
__device__ __forceinline__ void corr_row_stats(const T* __restrict__ row, int d, int t, double* red,
                                               double* __restrict__ out) {
  double s = 0.0;
  for (int k = t; k < d; k += 256) s += (double)row[k];
  s = wave_sum_d(s);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  const double mean = ((red[0] + red[1]) + (red[2] + red[3])) / (double)d;
  __syncthreads();
  double q = 0.0;
  for (int k = t; k < d; k += 256) {
    const double c = (double)row[k] - mean;
    q = fma(c, c, q);
  }
  q = wave_sum_d(q);
  if ((t & 63) == 0) red[t >> 6] = q;
  __syncthreads();
  if (t == 0) {
    out[0] = mean;
    out[1] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// this thread's ROWS / 16 values of the stage at column k0 of rows [x0, x0 + ROWS) of X (rows from xe on and columns
// from d on read as 0), kept in registers so that the loads are in flight during the MFMAs of the stage before
template <int ROWS, typename T>
__device__ __forceinline__ void corr_fetch(T (&v)[ROWS / 16], const T* __restrict__ X, int x0, int xe, int d, int k0,
                                           int t) {
  const int k = k0 + (t & 15), sr = t >> 4;
#pragma unroll
  for (int j = 0; j < ROWS / 16; ++j) {
    const int g = x0 + sr + 16 * j;
    v[j] = (k < d && g < xe) ? X[(size_t)g * d + k] : (T)0;
  }
}

// the fetched values into LDS, centred on the fp64 conversion with the rows' means xm[ROWS]; padding stays exactly 0
template <int ROWS, typename T>
__device__ __forceinline__ void corr_store(double* xs, const T (&v)[ROWS / 16], const double* xm, int x0, int xe, int d,
                                           int k0, int t) {
  const int sc = t & 15, sr = t >> 4;
  const bool kin = k0 + sc < d;
#pragma unroll
  for (int j = 0; j < ROWS / 16; ++j) {
    const int r = sr + 16 * j;
    xs[r * CORR_LD + sc] = (kin && x0 + r < xe) ? (double)v[j] - xm[r] : 0.0;
  }
}

// one stage of a wave's NA x NB blocks of 16 x 16 pairs: acc[a][b] += qs rows [qrow + 16 a, +16) . rs rows
// [rrow + 16 b, +16) over the stage's CORR_KC columns, in CORR_KC / 4 MFMA steps of ascending k.
// A: lane holds A[row lane & 15][k lane >> 4]; B: B[k lane >> 4][col lane & 15];
// C/D: col = lane & 15, row = (lane >> 4) + 4 reg.
template <int NA, int NB>
__device__ __forceinline__ void corr_mfma_stage(const double* qs, const double* rs, int qrow, int rrow, int lane,
                                                corr_d4 (&acc)[NA][NB]) {
#pragma unroll
  for (int kk = 0; kk < CORR_KC / 4; ++kk) {
    double fa[NA], fb[NB];
#pragma unroll
    for (int a = 0; a < NA; ++a) fa[a] = qs[(qrow + a * 16 + (lane & 15)) * CORR_LD + kk * 4 + (lane >> 4)];
#pragma unroll
    for (int b = 0; b < NB; ++b) fb[b] = rs[(rrow + b * 16 + (lane & 15)) * CORR_LD + kk * 4 + (lane >> 4)];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
  }
}
