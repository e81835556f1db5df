// Silhouette coefficients and the sums behind the Calinski-Harabasz and Davies-Bouldin scores of labelled latent rows
// (SURVEY.md section 8, row f21): the device side of scikit-learn 1.7's sklearn/metrics/cluster/_unsupervised.py.
// X is [N][d] float32 or float64 and is converted on load; everything else is fp64; nothing uses atomics; the same
// inputs give the same bits on every run, whatever the grid or the number of CUs.
//
// The host encodes the labels as 0 .. K - 1, takes the stable argsort `order` of the encoded labels and the table
// off [K + 1] of the clusters' first sorted rows.  "Sorted row r" is the caller's row order[r]; cluster k owns the
// sorted rows [off[k], off[k + 1]).
//   sil_gather_kernel        the rows into cluster order, once (workspace), so that a tile's rows are contiguous
//   sil_sums_kernel          workgroup (64-row tile, cluster k): S[r][k] = sum over the cluster's columns j of
//                            sqrt(sum_c (x_rc - x_jc)^2), the squared distance from sqd_stage / sqd_accumulate
//                            (sqdist_tile.h: direct differences, c ascending), then one fp64 sqrt
//   sil_sums_pre_kernel      the same S from an N x N matrix of distances, gathered through `order`
//   sil_finish_kernel        per row: a = S[r][l] / (n_l - 1), b = min_{k != l} S[r][k] / n_k, s = (b - a) / max(a, b),
//                            s = 0 where that is NaN (a cluster of one row; a = b = 0), written at the caller's row
//   sil_chunk_sum_kernel, sil_total_kernel      the mean of s
//   sil_centroid_kernel, sil_centroid_total_kernel      per cluster sum ||x - c_l|| and sum ||x - c_l||^2
//
// Order contract (every sum is one of these; none depends on the grid, on N or on where the row tile lies):
//   pair           sqdist_tile.h: from 0, one fma(x_c - y_c, x_c - y_c, sum) per c, c ascending; then sqrt
//   S[r][k]        the columns of cluster k are cut into chunks of SIL_CHUNK = 2048 counted from the cluster's first
//                  column.  Column p of a chunk (p < 2048) belongs to lane p & 15 and is that lane's term number p >> 4;
//                  a lane adds its terms ascending from 0, then the 16 lanes are added by the xor butterfly 8, 4, 2, 1
//                  (every lane ends with the same bits: each step adds the same two values in either order).  Columns
//                  beyond the cluster's end are exact zeros.  The chunk sums are added ascending from chunk 0.
//                  sil_sums_pre_kernel takes the same terms in the same order.
//   mean of s      chunks of 2048 rows in the caller's order; thread t of 256 adds rows t + 256 m, m ascending; the 256
//                  sums are added by the butterfly 32 .. 1 within a wave, then waves 0 .. 3 ascending; chunk sums
//                  ascending from chunk 0, then / N
//   centroid sums  chunks of 2048 rows in the caller's order; ||x - c||^2 by fma, features ascending; a cluster's sums
//                  take its rows of the chunk ascending; chunk sums ascending from chunk 0
#include <math.h>

#include "common.h"
#include "sqdist_tile.h"

#define SIL_MAX_K 1024           // grid.y of the sums kernels; the finish kernel walks K per row
#define SIL_CHUNK 2048           // columns (rows) of a chunk: a constant, never derived from the grid
#define SIL_CENT_MAX_D 128       // the centroid sums follow the means of mixture.hip (ava_gm_max_d, ava_gm_max_k)
#define SIL_CENT_MAX_K 64

// ---- rows into cluster order -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void sil_gather_kernel(const T* __restrict__ X, int n, int d,
                                                         const int64_t* __restrict__ order, T* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * d) return;
  const int64_t r = e / d;
  const int c = (int)(e - r * d);
  const int64_t g = order[r];
  out[e] = (g >= 0 && g < n) ? X[(size_t)g * d + c] : (T)0;
}

// the cluster's column range, clamped to the rows that exist
__device__ __forceinline__ void sil_range(const int64_t* __restrict__ off, int k, int n, int& c0, int& ce) {
  const int64_t a = off[k], b = off[k + 1];
  c0 = (int)(a < 0 ? 0 : (a > n ? n : a));
  ce = (int)(b < c0 ? c0 : (b > n ? n : b));
}

// the 16 lanes of a row (t & 15) into every one of them
__device__ __forceinline__ double sil_sum16(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- S, euclidean ------------------------------------------------------------------------------------------------------
// grid (ceil(n / 64), K), 256 threads; thread (ty, tx) = (t >> 4, t & 15) owns the pairs (ty + 16 i, tx + 16 j) of a tile
template <typename T>
__global__ __launch_bounds__(256) void sil_sums_kernel(const T* __restrict__ X, int n, int d, int K,
                                                       const int64_t* __restrict__ off, double* __restrict__ S) {
  __shared__ double xs[SQD_T * SQD_LD];
  __shared__ double ys[SQD_T * SQD_LD];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int k = blockIdx.y;
  const int q0 = blockIdx.x * SQD_T;
  int c0, ce;
  sil_range(off, k, n, c0, ce);
  double total[4] = {0.0, 0.0, 0.0, 0.0};
  for (int h0 = c0; h0 < ce; h0 += SIL_CHUNK) {                     // chunks from the cluster's first column
    const int he = h0 + SIL_CHUNK < ce ? h0 + SIL_CHUNK : ce;
    double part[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r0 = h0; r0 < he; r0 += SQD_T) {
      // sqd_tile's loop, written out: called through sqd_tile this kernel's stage addressing compiles to a 64-bit
      // multiply with sign fix-ups and the pass measured 0.17 % slower at N = 1e5 (profiles/NOTES.md (61))
      double acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
      for (int k0 = 0; k0 < d; k0 += SQD_KC) {
        __syncthreads();                                             // the stage before is consumed
        sqd_stage(xs, ys, X, q0, n, X, r0, he, d, k0, t);
        __syncthreads();
        sqd_accumulate(xs, ys, SQD_LD, d - k0 < SQD_KC ? d - k0 : SQD_KC, ty, tx, acc);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = r0 + tx + 16 * j < he;
#pragma unroll
        for (int i = 0; i < 4; ++i) part[i] += in ? sqrt(acc[i][j]) : 0.0;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) total[i] += sil_sum16(part[i]);
  }
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = q0 + ty + 16 * i;
      if (r < n) S[(size_t)r * K + k] = total[i];
    }
  }
}

// ---- S, precomputed distances ------------------------------------------------------------------------------------------
// the same grid, threads and order; D [n][n] in the caller's order, read through `order`
template <typename T>
__global__ __launch_bounds__(256) void sil_sums_pre_kernel(const T* __restrict__ D, int n, int K,
                                                           const int64_t* __restrict__ order,
                                                           const int64_t* __restrict__ off, double* __restrict__ S) {
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int k = blockIdx.y;
  const int q0 = blockIdx.x * SQD_T;
  int c0, ce;
  sil_range(off, k, n, c0, ce);
  int64_t grow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = q0 + ty + 16 * i;
    const int64_t g = r < n ? order[r] : -1;
    grow[i] = (g >= 0 && g < n) ? g : -1;
  }
  double total[4] = {0.0, 0.0, 0.0, 0.0};
  for (int h0 = c0; h0 < ce; h0 += SIL_CHUNK) {
    const int he = h0 + SIL_CHUNK < ce ? h0 + SIL_CHUNK : ce;
    double part[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r0 = h0; r0 < he; r0 += SQD_T) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = r0 + tx + 16 * j;
        int64_t gc = c < he ? order[c] : -1;
        if (gc >= n) gc = -1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          part[i] += (gc >= 0 && grow[i] >= 0) ? (double)D[(size_t)grow[i] * n + gc] : 0.0;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) total[i] += sil_sum16(part[i]);
  }
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = q0 + ty + 16 * i;
      if (r < n) S[(size_t)r * K + k] = total[i];
    }
  }
}

// ---- per row: a, b, s --------------------------------------------------------------------------------------------------
// thread per sorted row; the results go to the caller's row order[r]
__global__ __launch_bounds__(256) void sil_finish_kernel(const double* __restrict__ S, int n, int K,
                                                         const int64_t* __restrict__ order,
                                                         const int64_t* __restrict__ off, double* __restrict__ s_out,
                                                         double* __restrict__ a_out, double* __restrict__ b_out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int64_t g = order[r];
  if (g < 0 || g >= n) return;
  const double* row = S + (size_t)r * K;
  double a = 0.0, b = INFINITY;
  for (int k = 0; k < K; ++k) {
    const int64_t lo = off[k], hi = off[k + 1];
    const double nk = (double)(hi - lo);
    if (r >= lo && r < hi)
      a = row[k] / (nk - 1.0);                                       // 0 / 0 = NaN for a cluster of one row
    else
      b = fmin(b, row[k] / nk);
  }
  double s = (b - a) / fmax(a, b);
  if (s != s) s = 0.0;                                               // sklearn's nan_to_num
  s_out[g] = s;
  a_out[g] = a;
  b_out[g] = b;
}

// grid chunks, 256 threads: part[c] = the sum of rows [c SIL_CHUNK, (c + 1) SIL_CHUNK) of v in the header's order
__global__ __launch_bounds__(256) void sil_chunk_sum_kernel(const double* __restrict__ v, int n,
                                                            double* __restrict__ part) {
  __shared__ double ws[4];
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * SIL_CHUNK;
  double s = 0.0;
  for (int m = 0; m < SIL_CHUNK / 256; ++m) {
    const int64_t r = c0 + t + 256 * m;
    s += r < n ? v[r] : 0.0;
  }
  s = wave_sum_d(s);
  if ((t & 63) == 0) ws[t >> 6] = s;
  __syncthreads();
  if (t == 0) part[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

__global__ void sil_total_kernel(const double* __restrict__ part, int chunks, int n, double* __restrict__ score) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[c];
  score[0] = s / (double)n;
}

// ---- centroid sums -----------------------------------------------------------------------------------------------------
// grid chunks, 256 threads: part[c][k][0] = sum ||x - means[k]||, part[c][k][1] = sum ||x - means[k]||^2 over the rows of
// chunk c with labels[r] == k.  A label outside 0 .. K - 1 owns no sum.
template <typename T>
__global__ __launch_bounds__(256) void sil_centroid_kernel(const T* __restrict__ X, int n, int d, int K,
                                                           const int64_t* __restrict__ labels,
                                                           const double* __restrict__ means,
                                                           double* __restrict__ part) {
  __shared__ double d2[SIL_CHUNK];
  __shared__ double d1[SIL_CHUNK];
  __shared__ int lab[SIL_CHUNK];
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * SIL_CHUNK;
  for (int m = 0; m < SIL_CHUNK / 256; ++m) {
    const int p = t + 256 * m;
    const int64_t r = c0 + p;
    int l = -1;
    double s = 0.0;
    if (r < n) {
      const int64_t lr = labels[r];
      if (lr >= 0 && lr < K) {
        l = (int)lr;
        const T* x = X + (size_t)r * d;
        const double* mu = means + (size_t)l * d;
        for (int c = 0; c < d; ++c) {
          const double df = (double)x[c] - mu[c];
          s = fma(df, df, s);
        }
      }
    }
    lab[p] = l;
    d2[p] = s;
    d1[p] = sqrt(s);
  }
  __syncthreads();
  const int rows = n - c0 < SIL_CHUNK ? (int)(n - c0) : SIL_CHUNK;
  for (int k = t; k < K; k += 256) {
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < rows; ++p)
      if (lab[p] == k) {
        s1 += d1[p];
        s2 += d2[p];
      }
    part[((size_t)blockIdx.x * K + k) * 2] = s1;
    part[((size_t)blockIdx.x * K + k) * 2 + 1] = s2;
  }
}

__global__ __launch_bounds__(256) void sil_centroid_total_kernel(const double* __restrict__ part, int chunks, int K,
                                                                 double* __restrict__ sum_dist,
                                                                 double* __restrict__ sum_sq) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double s1 = 0.0, s2 = 0.0;
  for (int c = 0; c < chunks; ++c) {
    s1 += part[((size_t)c * K + k) * 2];
    s2 += part[((size_t)c * K + k) * 2 + 1];
  }
  sum_dist[k] = s1;
  sum_sq[k] = s2;
}

// ---- host --------------------------------------------------------------------------------------------------------------
static inline bool sil_shape_ok(int n, int d, int K) {
  return d >= 1 && K >= 2 && K <= SIL_MAX_K && n > K && n <= (1 << 30) && (int64_t)n * d < ((int64_t)1 << 38);
}

struct sil_ws {
  void* rows;
  double *mean_part, *cent_part;
};
static size_t sil_ws_layout(int n, int d, int K, void* base, sil_ws* out) {
  const size_t chunks = ceil_div(n, SIL_CHUNK);
  ava_ws_cursor c(base);
  void* rows = c.take<double>((size_t)n * d);                         // float32 rows use the first half
  double* mean_part = c.take<double>(chunks);
  double* cent_part = c.take<double>(chunks * K * 2);
  if (out) *out = sil_ws{rows, mean_part, cent_part};
  return c.bytes();
}

extern "C" int ava_sil_max_k(void) { return SIL_MAX_K; }
extern "C" int ava_sil_chunk_cols(void) { return SIL_CHUNK; }

extern "C" size_t ava_sil_workspace_bytes(int n, int d, int k) {
  if (!sil_shape_ok(n, d, k)) return 0;
  return sil_ws_layout(n, d, k, nullptr, nullptr);
}

template <typename T>
static int sil_launch_sums(const T* X, int n, int d, int K, const int64_t* order, const int64_t* off, double* S,
                           const sil_ws& w, hipStream_t st) {
  T* rows = static_cast<T*>(w.rows);
  hipLaunchKernelGGL(sil_gather_kernel<T>, dim3((unsigned)ceil_div64((int64_t)n * d, 256)), dim3(256), 0, st, X, n, d,
                     order, rows);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sil_sums_kernel<T>, dim3(ceil_div(n, SQD_T), K), dim3(256), 0, st, rows, n, d, K, off, S);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_sil_cluster_sums(const void* x, int dtype, int n, int d, int k, const int64_t* order,
                                    const int64_t* off, double* sums, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !sil_shape_ok(n, d, k) || !order || !off || !sums || !ws) return AVA_EINVAL;
  if (ws_bytes < ava_sil_workspace_bytes(n, d, k)) return AVA_EWORKSPACE;
  sil_ws w;
  sil_ws_layout(n, d, k, ws, &w);
  return dtype == 0 ? sil_launch_sums(static_cast<const float*>(x), n, d, k, order, off, sums, w, to_stream(s))
                    : sil_launch_sums(static_cast<const double*>(x), n, d, k, order, off, sums, w, to_stream(s));
}

extern "C" int ava_sil_cluster_sums_pre(const void* dist, int dtype, int n, int k, const int64_t* order,
                                        const int64_t* off, double* sums, ava_stream_t s) {
  if (!dist || (dtype != 0 && dtype != 1) || !sil_shape_ok(n, 1, k) || !order || !off || !sums) return AVA_EINVAL;
  const dim3 grid(ceil_div(n, SQD_T), k);
  if (dtype == 0)
    hipLaunchKernelGGL(sil_sums_pre_kernel<float>, grid, dim3(256), 0, to_stream(s), static_cast<const float*>(dist), n,
                       k, order, off, sums);
  else
    hipLaunchKernelGGL(sil_sums_pre_kernel<double>, grid, dim3(256), 0, to_stream(s), static_cast<const double*>(dist),
                       n, k, order, off, sums);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_sil_finish(const double* sums, int n, int k, const int64_t* order, const int64_t* off, double* sil,
                              double* a, double* b, double* score, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!sums || !sil_shape_ok(n, 1, k) || !order || !off || !sil || !a || !b || !score || !ws) return AVA_EINVAL;
  if (ws_bytes < ava_sil_workspace_bytes(n, 1, k)) return AVA_EWORKSPACE;
  sil_ws w;
  sil_ws_layout(n, 1, k, ws, &w);
  const int chunks = ceil_div(n, SIL_CHUNK);
  hipStream_t st = to_stream(s);
  hipLaunchKernelGGL(sil_finish_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, sums, n, k, order, off, sil, a, b);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sil_chunk_sum_kernel, dim3(chunks), dim3(256), 0, st, sil, n, w.mean_part);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sil_total_kernel, dim3(1), dim3(64), 0, st, w.mean_part, chunks, n, score);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_sil_centroid_stats(const void* x, int dtype, int n, int d, int k, const int64_t* labels,
                                      const double* means, double* sum_dist, double* sum_sq, void* ws, size_t ws_bytes,
                                      ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !sil_shape_ok(n, d, k) || d > SIL_CENT_MAX_D || k > SIL_CENT_MAX_K ||
      !labels || !means || !sum_dist || !sum_sq || !ws)
    return AVA_EINVAL;
  if (ws_bytes < ava_sil_workspace_bytes(n, d, k)) return AVA_EWORKSPACE;
  sil_ws w;
  sil_ws_layout(n, d, k, ws, &w);
  const int chunks = ceil_div(n, SIL_CHUNK);
  hipStream_t st = to_stream(s);
  if (dtype == 0)
    hipLaunchKernelGGL(sil_centroid_kernel<float>, dim3(chunks), dim3(256), 0, st, static_cast<const float*>(x), n, d, k,
                       labels, means, w.cent_part);
  else
    hipLaunchKernelGGL(sil_centroid_kernel<double>, dim3(chunks), dim3(256), 0, st, static_cast<const double*>(x), n, d,
                       k, labels, means, w.cent_part);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sil_centroid_total_kernel, dim3(ceil_div(k, 256)), dim3(256), 0, st, w.cent_part, chunks, k,
                     sum_dist, sum_sq);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
