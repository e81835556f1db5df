// UMAP and PCA projections of latent means (DataContainer's 'latent_mean_umap' / 'latent_mean_pca' fields,
// ava/data/data_container.py:514-551).  All arithmetic is fp64; no kernel uses atomics and every reduction runs in one
// fixed order, so every result is bit-reproducible and independent of the launch shape.
//
// kNN       exact euclidean k-nearest neighbours of every row among all rows.  A workgroup owns 64 query rows and walks
//           the references in 64-row tiles (the fp64 direct-difference tile of sqdist_tile.h, which states the order
//           of every sum); each query keeps a running top-(k-1) list in LDS ordered by (distance, index), the query
//           itself excluded.  Column 0 of the output is the row itself at distance 0.
// kNN corr  the same table under umap-learn's correlation distance (TransformableUMAP(metric='correlation')): the
//           centred dot products of corr_tile.h on the fp64 matrix cores, the row statistics from a kernel of their
//           own; the lists, the fold and both modes are the euclidean kernel's.  Every distance is finite.
// smooth    umap's smooth_knn_dist + compute_membership_strengths, one row per thread.
// layout    one synchronous, gather-only SGD epoch per launch over the symmetric CSR graph (rows = heads): a thread
//           per vertex sums, in CSR order, the attractive moves of its active edges and their negative samples, all
//           read from the previous epoch's positions, and advances the edges' sample counters.
// query     the out-of-sample half (umap's transform): the k nearest reference rows of every query row (the kNN kernel
//           with a query pointer and no excluded row), the bipartite memberships (the smooth kernel without the zeroed
//           own column), the l1-normalised weights with the weighted-mean start positions, and a layout in which only
//           the new points move: a thread per query row runs every epoch in one launch and applies its moves edge by
//           edge, the per-slot sample counters in LDS.
// PCA       column sums and X^T X as the Gram matrix of [X, 1] (chunks of rows, chunks summed in order), and the
//           projection X V^T - mu V^T.
#include "common.h"
#include "corr_tile.h"
#include "knn_list.h"
#include "sqdist_tile.h"

#define PJ_MAX_NEG 16
#define PJ_GT 32         // Gram tile
#define PJ_GR 64         // rows per Gram LDS stage
#define PJ_MAX_PCA_DIM 512

// rows [q0, q0 + nq) of the kNN table of the query rows Q among the n reference rows X; dynamic LDS holds the running
// lists: slot s of local query t at [s * 64 + t].  With exclude_self (Q == X) reference q is skipped for query q and
// column 0 is the row itself at 0; without, all k columns come from the list.
template <typename T>
__global__ __launch_bounds__(256) void pj_knn_kernel(const T* __restrict__ Q, const T* __restrict__ X, int n, int d,
                                                     int k, int q0, int nq, int exclude_self,
                                                     int64_t* __restrict__ out_idx, double* __restrict__ out_dist) {
  __shared__ double stage[2 * SQD_T * SQD_LD];      // xs | ys while staging, then the 64 x 64 distance tile
  extern __shared__ double lists[];                 // m x 64 distances, then m x 64 int indices
  double* xs = stage;
  double* ys = stage + SQD_T * SQD_LD;
  double* dt = stage;
  const int m = k - exclude_self;
  double* ld = lists;
  int* li = reinterpret_cast<int*>(lists + (size_t)m * SQD_T);
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int qb = q0 + blockIdx.x * SQD_T;            // first query row of this workgroup
  const int qe = q0 + nq;
  for (int s = t; s < m * SQD_T; s += 256) {
    ld[s] = 0.0;
    li[s] = -1;
  }
  for (int r0 = 0; r0 < n; r0 += SQD_T) {
    double acc[4][4];
    sqd_tile(xs, ys, Q, qb, qe, X, r0, n, d, t, acc);  // opens with a barrier: the distance tile before is folded
    __syncthreads();                                 // staging reads done: the tile reuses the buffer
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dt[(ty + 16 * i) * PJ_DLD + tx + 16 * j] = sqrt(acc[i][j]);
    __syncthreads();
    if (t < SQD_T && qb + t < qe && m > 0)
      pj_fold_tile(dt + t * PJ_DLD, r0, n - r0 < SQD_T ? n - r0 : SQD_T, qb + t, exclude_self, m, ld, li, t);
  }
  __syncthreads();
  if (t < SQD_T && qb + t < qe)
    pj_write_list((size_t)(qb + t - q0), qb + t, k, exclude_self, ld, li, t, out_idx, out_dist);
}

// stats[2 r] = mean of row r, stats[2 r + 1] = sum_k (x_rk - mean)^2 (corr_tile.h): one workgroup per row
template <typename T>
__global__ __launch_bounds__(256) void pj_row_stats_kernel(const T* __restrict__ x, int d, double* __restrict__ stats) {
  __shared__ double red[4];
  corr_row_stats(x + (size_t)blockIdx.x * d, d, threadIdx.x, red, stats + 2 * (size_t)blockIdx.x);
}

// umap-learn's correlation distance of two rows from their centred dot product and centred sums of squares:
// 1 - dot / sqrt(ss_q ss_r) with the cosine clipped to [-1, 1]; 0 when both rows have no variance, 1 when exactly one
// has none.  Always finite: a quotient that is no number (a product of sums of squares that left the fp64 range)
// counts as cosine 0.
__device__ __forceinline__ double pj_corr_dist(double dot, double ssq, double ssr) {
  if (ssq == 0.0 || ssr == 0.0) return (ssq == 0.0 && ssr == 0.0) ? 0.0 : 1.0;
  double c = dot / sqrt(ssq * ssr);
  if (!(fabs(c) <= 1.0)) c = isnan(c) ? 0.0 : copysign(1.0, c);
  return 1.0 - c;
}

// The correlation counterpart of pj_knn_kernel: same modes, same lists, same fold, same output.  A workgroup owns 64
// query rows and walks the references in 64-row tiles; each of its four waves owns a 32 x 32 quarter of the tile,
// 2 x 2 blocks of v_mfma_f64_16x16x4_f64 over the centred operands (the stages and the order of corr_tile.h: 16
// columns per stage, 4 per MFMA step).  The accumulators go through pj_corr_dist into the 64 x 64 distance tile in
// LDS (C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg), which one thread per query folds into its list.
// LDS: 33 280 B static for the distance tile (64 x 65 doubles; its first 17 408 B are the two 64 x 17 staging buffers
// while the MFMAs run), 2 048 B for the means and sums of squares of the 64 + 64 rows, and 768 (k - exclude_self) B of
// dynamic lists: 84 480 B at k = 64 in query mode, of the 160 KiB a workgroup may use.
template <typename T>
__global__ __launch_bounds__(256) void pj_knn_corr_kernel(const T* __restrict__ Q, const T* __restrict__ X,
                                                          const double* __restrict__ qstat,
                                                          const double* __restrict__ xstat, int n, int d, int k, int q0,
                                                          int nq, int exclude_self, int64_t* __restrict__ out_idx,
                                                          double* __restrict__ out_dist) {
  __shared__ double stage[SQD_T * PJ_DLD];          // qs | rs while staging, then the 64 x 64 distance tile
  __shared__ double qm[SQD_T], qss[SQD_T], rm[SQD_T], rss[SQD_T];
  extern __shared__ double lists[];                 // m x 64 distances, then m x 64 int indices
  double* qs = stage;
  double* rs = stage + SQD_T * CORR_LD;
  double* dt = stage;
  const int m = k - exclude_self;
  double* ld = lists;
  int* li = reinterpret_cast<int*>(lists + (size_t)m * SQD_T);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wq = w & 1, wr = w >> 1;                 // this wave's 32 x 32 quarter of the tile
  const int qb = q0 + blockIdx.x * SQD_T;            // first query row of this workgroup
  const int qe = q0 + nq;
  for (int s = t; s < m * SQD_T; s += 256) {
    ld[s] = 0.0;
    li[s] = -1;
  }
  if (t < SQD_T) {
    const bool in = qb + t < qe;
    qm[t] = in ? qstat[2 * (size_t)(qb + t)] : 0.0;
    qss[t] = in ? qstat[2 * (size_t)(qb + t) + 1] : 1.0;
  }
  T vq[SQD_T / 16], vr[SQD_T / 16];
  for (int r0 = 0; r0 < n; r0 += SQD_T) {
    __syncthreads();                                 // previous tile folded: the buffer and rm / rss are free
    if (t < SQD_T) {
      const bool in = r0 + t < n;
      rm[t] = in ? xstat[2 * (size_t)(r0 + t)] : 0.0;
      rss[t] = in ? xstat[2 * (size_t)(r0 + t) + 1] : 1.0;
    }
    corr_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = corr_d4{0.0, 0.0, 0.0, 0.0};
    corr_fetch<SQD_T>(vq, Q, qb, qe, d, 0, t);
    corr_fetch<SQD_T>(vr, X, r0, n, d, 0, t);
    __syncthreads();                                 // qm / rm
    for (int k0 = 0; k0 < d; k0 += CORR_KC) {
      corr_store<SQD_T>(qs, vq, qm, qb, qe, d, k0, t);
      corr_store<SQD_T>(rs, vr, rm, r0, n, d, k0, t);
      __syncthreads();
      if (k0 + CORR_KC < d) {                        // next stage's loads in flight during the MFMAs
        corr_fetch<SQD_T>(vq, Q, qb, qe, d, k0 + CORR_KC, t);
        corr_fetch<SQD_T>(vr, X, r0, n, d, k0 + CORR_KC, t);
      }
      corr_mfma_stage<2, 2>(qs, rs, wq * 32, wr * 32, lane, acc);
      __syncthreads();                               // staging reads done: the next stage / the tile reuses the buffer
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int lr = wq * 32 + a * 16 + (lane >> 4) + 4 * reg;
          const int lc = wr * 32 + b * 16 + (lane & 15);
          dt[lr * PJ_DLD + lc] = pj_corr_dist(acc[a][b][reg], qss[lr], rss[lc]);
        }
    __syncthreads();
    if (t < SQD_T && qb + t < qe && m > 0)
      pj_fold_tile(dt + t * PJ_DLD, r0, n - r0 < SQD_T ? n - r0 : SQD_T, qb + t, exclude_self, m, ld, li, t);
  }
  __syncthreads();
  if (t < SQD_T && qb + t < qe)
    pj_write_list((size_t)(qb + t - q0), qb + t, k, exclude_self, ld, li, t, out_idx, out_dist);
}

// mean of the whole [n][k] distance table: thread t sums rows t, t + 256, ... (each row left to right), then a fixed tree
__global__ __launch_bounds__(256) void pj_mean_kernel(const double* __restrict__ dist, int n, int k,
                                                      double* __restrict__ mean) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int r = t; r < n; r += 256) {
    double rs = 0.0;
    for (int j = 0; j < k; ++j) rs += dist[(size_t)r * k + j];
    s += rs;
  }
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) mean[0] = red[0] / ((double)n * (double)k);
}

// smooth_knn_dist (n_iter 64, bandwidth 1) and compute_membership_strengths of one row per thread; bipartite (the
// columns index another set than the rows) keeps the weight of column idx == row
__global__ __launch_bounds__(256) void pj_smooth_kernel(const double* __restrict__ dist, const int64_t* __restrict__ idx,
                                                        int n, int k, double local_connectivity, int bipartite,
                                                        const double* __restrict__ mean_all,
                                                        double* __restrict__ sigma, double* __restrict__ rho,
                                                        double* __restrict__ w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* row = dist + (size_t)i * k;
  const double target = log2((double)k);
  // rho: the local_connectivity-th nonzero distance (interpolated), else the largest nonzero one
  int nz = 0;
  double maxnz = 0.0, rowsum = 0.0;
  for (int j = 0; j < k; ++j) {
    rowsum += row[j];
    if (row[j] > 0.0) {
      ++nz;
      maxnz = fmax(maxnz, row[j]);
    }
  }
  double r = 0.0;
  if ((double)nz >= local_connectivity) {
    const int index = (int)floor(local_connectivity);
    const double interp = local_connectivity - index;
    double prev = 0.0, at = 0.0;                     // nonzero distances index - 1 and index
    int seen = 0;
    for (int j = 0; j < k; ++j) {
      if (row[j] > 0.0) {
        if (seen == index - 1) prev = row[j];
        if (seen == index) at = row[j];
        ++seen;
      }
    }
    if (index > 0) {
      r = prev;
      if (interp > 1e-5) r += interp * (at - prev);
    } else {
      double first = 0.0;
      for (int j = k - 1; j >= 0; --j)
        if (row[j] > 0.0) first = row[j];
      r = interp * first;
    }
  } else if (nz > 0) {
    r = maxnz;
  }
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int it = 0; it < 64; ++it) {
    double psum = 0.0;
    for (int j = 1; j < k; ++j) {
      const double dd = row[j] - r;
      psum += dd > 0.0 ? exp(-(dd / mid)) : 1.0;
    }
    if (fabs(psum - target) < 1e-5) break;
    if (psum > target) {
      hi = mid;
      mid = (lo + hi) / 2.0;
    } else {
      lo = mid;
      mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
    }
  }
  const double floor_scale = 1e-3 * (r > 0.0 ? rowsum / (double)k : mean_all[0]);
  if (mid < floor_scale) mid = floor_scale;
  sigma[i] = mid;
  rho[i] = r;
  for (int j = 0; j < k; ++j) {
    double v;
    if (!bipartite && idx[(size_t)i * k + j] == i) v = 0.0;
    else if (row[j] - r <= 0.0 || mid == 0.0) v = 1.0;
    else v = exp(-((row[j] - r) / mid));
    w[(size_t)i * k + j] = v;
  }
}

__device__ __forceinline__ double pj_clip(double v) { return v > 4.0 ? 4.0 : (v < -4.0 ? -4.0 : v); }

// one layout epoch: y_out[v] = y_in[v] + the moves of v's active edges and their negative samples
__global__ __launch_bounds__(64) void pj_layout_kernel(const double* __restrict__ y_in, double* __restrict__ y_out,
                                                        const int64_t* __restrict__ indptr,
                                                        const int* __restrict__ col, const double* __restrict__ eps,
                                                        const double* __restrict__ epn, double* __restrict__ next_s,
                                                        double* __restrict__ next_n, int n, int64_t nnz, int epoch,
                                                        double alpha, double a, double b, double gamma, uint64_t salt,
                                                        int* __restrict__ flag) {
  // every product and sum rounded on its own (no fused multiply-add): the layout is chaotic where negative samples
  // meet close pairs, and contraction alone would part it from an unfused restatement within a few epochs
#pragma clang fp contract(off)
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n) return;
  const double y0 = y_in[2 * (size_t)v], y1 = y_in[2 * (size_t)v + 1];
  double m0 = 0.0, m1 = 0.0;
  const double ep = (double)epoch;
  for (int64_t e = indptr[v]; e < indptr[v + 1]; ++e) {
    if (!(next_s[e] <= ep)) continue;
    const int j = col[e];
    double d0 = y0 - y_in[2 * (size_t)j], d1 = y1 - y_in[2 * (size_t)j + 1];
    double d2 = d0 * d0 + d1 * d1;
    double g = 0.0;
    if (d2 > 0.0) g = -2.0 * a * b * pow(d2, b - 1.0) / (a * pow(d2, b) + 1.0);
    m0 += 2.0 * alpha * pj_clip(g * d0);
    m1 += 2.0 * alpha * pj_clip(g * d1);
    next_s[e] += eps[e];
    int nneg = (int)((ep - next_n[e]) / epn[e]);
    if (nneg > PJ_MAX_NEG) {
      flag[0] = 1;
      nneg = PJ_MAX_NEG;
    }
    for (int p = 0; p < nneg; ++p) {
      const uint64_t ctr = ((uint64_t)epoch * (uint64_t)nnz + (uint64_t)e) * PJ_MAX_NEG + (uint64_t)p;
      int64_t kk = (int64_t)floor(ava_u01_hash(ctr, salt) * (double)n);
      if (kk > n - 1) kk = n - 1;
      if (kk == v) continue;
      d0 = y0 - y_in[2 * (size_t)kk];
      d1 = y1 - y_in[2 * (size_t)kk + 1];
      d2 = d0 * d0 + d1 * d1;
      if (d2 > 0.0) {
        const double c = 2.0 * gamma * b / ((0.001 + d2) * (a * pow(d2, b) + 1.0));
        if (c > 0.0) {
          m0 += alpha * pj_clip(c * d0);
          m1 += alpha * pj_clip(c * d1);
        }
      }
    }
    next_n[e] += nneg * epn[e];
  }
  y_out[2 * (size_t)v] = y0 + m0;
  y_out[2 * (size_t)v + 1] = y1 + m1;
}

// transform: l1-normalised weights (summed left to right; a row of sum 0 stays 0) and the start position of every new
// point, the weighted mean of the training positions of its neighbours in slot order (umap's init_transform)
__global__ __launch_bounds__(256) void pj_transform_init_kernel(const double* __restrict__ w,
                                                                const int64_t* __restrict__ idx,
                                                                const double* __restrict__ emb, int m, int k,
                                                                double* __restrict__ wn, double* __restrict__ y0) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double sum = 0.0;
  for (int s = 0; s < k; ++s) sum += w[(size_t)i * k + s];
  double a0 = 0.0, a1 = 0.0;
  for (int s = 0; s < k; ++s) {
    const double v = sum > 0.0 ? w[(size_t)i * k + s] / sum : 0.0;
    const int64_t j = idx[(size_t)i * k + s];
    wn[(size_t)i * k + s] = v;
    a0 += v * emb[2 * (size_t)j];
    a1 += v * emb[2 * (size_t)j + 1];
  }
  y0[2 * (size_t)i] = a0;
  y0[2 * (size_t)i + 1] = a1;
}

// transform layout: epochs [0, epochs) of n_epochs for every new point in one launch.  The training positions emb are
// read-only and the rows do not depend on each other, so a thread owns a row and applies its moves edge by edge as
// umap-learn does: slot s, when due, pulls y towards emb[idx[i][s]] (once: there is no tail move to stand in for) and
// then pushes it from that slot's negative samples, each from the position the moves before it left.  eps / epn are
// slot-major [k][m] (eps <= 0: a pruned slot); the counters of slot s of local row t live in LDS at [s * 64 + t] and
// [(k + s) * 64 + t].
__global__ __launch_bounds__(64) void pj_transform_layout_kernel(double* __restrict__ y, const double* __restrict__ emb,
                                                                  const int64_t* __restrict__ idx,
                                                                  const double* __restrict__ eps,
                                                                  const double* __restrict__ epn, int m, int k,
                                                                  int n_train, int epochs, int n_epochs, double alpha0,
                                                                  double a, double b, double gamma, uint64_t salt,
                                                                  int* __restrict__ flag) {
  // unfused for the reason given in pj_layout_kernel
#pragma clang fp contract(off)
  extern __shared__ double counters[];
  const int t = threadIdx.x;
  const int i = blockIdx.x * 64 + t;
  if (i >= m) return;
  double* next_s = counters;
  double* next_n = counters + (size_t)k * 64;
  for (int s = 0; s < k; ++s) {
    const double e = eps[(size_t)s * m + i];
    next_s[s * 64 + t] = e > 0.0 ? e : INFINITY;
    next_n[s * 64 + t] = epn[(size_t)s * m + i];
  }
  double y0 = y[2 * (size_t)i], y1 = y[2 * (size_t)i + 1];
  for (int epoch = 0; epoch < epochs; ++epoch) {
    const double ep = (double)epoch;
    const double alpha = epoch == 0 ? alpha0 : alpha0 * (1.0 - (double)(epoch - 1) / (double)n_epochs);
    for (int s = 0; s < k; ++s) {
      if (!(next_s[s * 64 + t] <= ep)) continue;
      const int64_t j = idx[(size_t)i * k + s];
      const double es = eps[(size_t)s * m + i], en = epn[(size_t)s * m + i];
      double d0 = y0 - emb[2 * (size_t)j], d1 = y1 - emb[2 * (size_t)j + 1];
      double d2 = d0 * d0 + d1 * d1;
      double g = 0.0;
      if (d2 > 0.0) g = -2.0 * a * b * pow(d2, b - 1.0) / (a * pow(d2, b) + 1.0);
      y0 += alpha * pj_clip(g * d0);
      y1 += alpha * pj_clip(g * d1);
      next_s[s * 64 + t] += es;
      int nneg = (int)((ep - next_n[s * 64 + t]) / en);
      if (nneg > PJ_MAX_NEG) {
        flag[0] = 1;
        nneg = PJ_MAX_NEG;
      }
      for (int p = 0; p < nneg; ++p) {
        const uint64_t ctr = (((uint64_t)epoch * (uint64_t)m + (uint64_t)i) * (uint64_t)k + (uint64_t)s) * PJ_MAX_NEG +
                             (uint64_t)p;
        int64_t kk = (int64_t)floor(ava_u01_hash(ctr, salt) * (double)n_train);
        if (kk > n_train - 1) kk = n_train - 1;
        d0 = y0 - emb[2 * (size_t)kk];
        d1 = y1 - emb[2 * (size_t)kk + 1];
        d2 = d0 * d0 + d1 * d1;
        if (d2 > 0.0) {
          const double c = 2.0 * gamma * b / ((0.001 + d2) * (a * pow(d2, b) + 1.0));
          if (c > 0.0) {
            y0 += alpha * pj_clip(c * d0);
            y1 += alpha * pj_clip(c * d1);
          }
        }
      }
      next_n[s * 64 + t] += nneg * en;
    }
  }
  y[2 * (size_t)i] = y0;
  y[2 * (size_t)i + 1] = y1;
}

// partial Gram matrices of [X, 1] (D = d + 1 columns): part[chunk][i][j] = sum over the chunk's rows, in row order
template <typename T>
__global__ __launch_bounds__(256) void pj_gram_kernel(const T* __restrict__ X, int n, int d, int rows_per_chunk,
                                                      int tiles, double* __restrict__ part) {
  __shared__ double xi[PJ_GR][PJ_GT + 1];
  __shared__ double xj[PJ_GR][PJ_GT + 1];
  const int D = d + 1;
  const int t = threadIdx.x;
  const int i0 = (blockIdx.x / tiles) * PJ_GT, j0 = (blockIdx.x % tiles) * PJ_GT;
  const int rb = blockIdx.y * rows_per_chunk;
  const int re = rb + rows_per_chunk < n ? rb + rows_per_chunk : n;
  const int ti = (t >> 4) * 2, tj = (t & 15) * 2;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int r0 = rb; r0 < re; r0 += PJ_GR) {
    __syncthreads();
    for (int e = t; e < PJ_GR * PJ_GT; e += 256) {
      const int r = e / PJ_GT, c = e % PJ_GT, gr = r0 + r;
      const int ci = i0 + c, cj = j0 + c;
      double vi = 0.0, vj = 0.0;
      if (gr < re) {
        vi = ci < d ? (double)X[(size_t)gr * d + ci] : (ci == d ? 1.0 : 0.0);
        vj = cj < d ? (double)X[(size_t)gr * d + cj] : (cj == d ? 1.0 : 0.0);
      }
      xi[r][c] = vi;
      xj[r][c] = vj;
    }
    __syncthreads();
    for (int r = 0; r < PJ_GR; ++r) {
      const double a0 = xi[r][ti], a1 = xi[r][ti + 1], b0 = xj[r][tj], b1 = xj[r][tj + 1];
      acc[0][0] = fma(a0, b0, acc[0][0]);
      acc[0][1] = fma(a0, b1, acc[0][1]);
      acc[1][0] = fma(a1, b0, acc[1][0]);
      acc[1][1] = fma(a1, b1, acc[1][1]);
    }
  }
  double* out = part + (size_t)blockIdx.y * D * D;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + ti + a, j = j0 + tj + b;
      if (i < D && j < D) out[(size_t)i * D + j] = acc[a][b];
    }
}

__global__ __launch_bounds__(256) void pj_gram_reduce_kernel(const double* __restrict__ part, int chunks, int DD,
                                                             double* __restrict__ gram) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= DD) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(size_t)c * DD + e];
  gram[e] = s;
}

// out[r][c] = sum_j X[r][j] V[c][j] - muv[c]
template <typename T>
__global__ __launch_bounds__(256) void pj_project_kernel(const T* __restrict__ X, int n, int d,
                                                         const double* __restrict__ V, const double* __restrict__ muv,
                                                         int nc, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * nc) return;
  const int64_t r = e / nc;
  const int c = (int)(e % nc);
  const T* row = X + (size_t)r * d;
  const double* vc = V + (size_t)c * d;
  double s = 0.0;
  for (int j = 0; j < d; ++j) s = fma((double)row[j], vc[j], s);
  out[e] = s - muv[c];
}

static bool pj_knn_ok(int n, int d, int k, int q0, int nq) {
  return n >= 1 && d >= 1 && d <= 65536 && k >= 1 && k <= PJ_MAX_K && k <= n && q0 >= 0 && nq >= 1 &&
         (int64_t)q0 + nq <= n;
}

template <typename T>
static int pj_knn_launch(const void* q, const void* x, int n, int d, int k, int q0, int nq, int exclude_self,
                         int64_t* idx, double* dist, hipStream_t st) {
  const size_t lds = (size_t)(k - exclude_self) * SQD_T * (sizeof(double) + sizeof(int));
  hipLaunchKernelGGL(pj_knn_kernel<T>, dim3(ceil_div(nq, SQD_T)), dim3(256), lds, st, reinterpret_cast<const T*>(q),
                     reinterpret_cast<const T*>(x), n, d, k, q0, nq, exclude_self, idx, dist);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_pj_knn(const void* x, int dtype, int n, int d, int k, int q0, int nq, int64_t* out_idx,
                          double* out_dist, ava_stream_t s) {
  if (x == nullptr || out_idx == nullptr || out_dist == nullptr || (dtype != 0 && dtype != 1) ||
      !pj_knn_ok(n, d, k, q0, nq))
    return AVA_EINVAL;
  if (dtype == 0) return pj_knn_launch<float>(x, x, n, d, k, q0, nq, 1, out_idx, out_dist, to_stream(s));
  return pj_knn_launch<double>(x, x, n, d, k, q0, nq, 1, out_idx, out_dist, to_stream(s));
}

extern "C" int ava_pj_knn_query(const void* q, const void* x, int dtype, int m, int n, int d, int k, int q0, int nq,
                                int64_t* out_idx, double* out_dist, ava_stream_t s) {
  if (q == nullptr || x == nullptr || out_idx == nullptr || out_dist == nullptr || (dtype != 0 && dtype != 1) ||
      n < 1 || m < 1 || d < 1 || d > 65536 || k < 1 || k > PJ_MAX_K || k > n || q0 < 0 || nq < 1 ||
      (int64_t)q0 + nq > m)
    return AVA_EINVAL;
  if (dtype == 0) return pj_knn_launch<float>(q, x, n, d, k, q0, nq, 0, out_idx, out_dist, to_stream(s));
  return pj_knn_launch<double>(q, x, n, d, k, q0, nq, 0, out_idx, out_dist, to_stream(s));
}

template <typename T>
static int pj_knn_corr_launch(const void* q, const void* x, const double* qstat, const double* xstat, int n, int d,
                              int k, int q0, int nq, int exclude_self, int64_t* idx, double* dist, hipStream_t st) {
  const size_t lds = (size_t)(k - exclude_self) * SQD_T * (sizeof(double) + sizeof(int));
  hipLaunchKernelGGL(pj_knn_corr_kernel<T>, dim3(ceil_div(nq, SQD_T)), dim3(256), lds, st,
                     reinterpret_cast<const T*>(q), reinterpret_cast<const T*>(x), qstat, xstat, n, d, k, q0, nq,
                     exclude_self, idx, dist);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_pj_row_stats(const void* x, int dtype, int n, int d, double* stats, ava_stream_t s) {
  if (x == nullptr || stats == nullptr || (dtype != 0 && dtype != 1) || n < 1 || d < 1 || d > 65536)
    return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  if (dtype == 0)
    hipLaunchKernelGGL(pj_row_stats_kernel<float>, dim3(n), dim3(256), 0, st, reinterpret_cast<const float*>(x), d,
                       stats);
  else
    hipLaunchKernelGGL(pj_row_stats_kernel<double>, dim3(n), dim3(256), 0, st, reinterpret_cast<const double*>(x), d,
                       stats);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_pj_knn_corr(const void* x, int dtype, const double* xstat, int n, int d, int k, int q0, int nq,
                               int64_t* out_idx, double* out_dist, ava_stream_t s) {
  if (x == nullptr || xstat == nullptr || out_idx == nullptr || out_dist == nullptr || (dtype != 0 && dtype != 1) ||
      !pj_knn_ok(n, d, k, q0, nq))
    return AVA_EINVAL;
  if (dtype == 0)
    return pj_knn_corr_launch<float>(x, x, xstat, xstat, n, d, k, q0, nq, 1, out_idx, out_dist, to_stream(s));
  return pj_knn_corr_launch<double>(x, x, xstat, xstat, n, d, k, q0, nq, 1, out_idx, out_dist, to_stream(s));
}

extern "C" int ava_pj_knn_corr_query(const void* q, const void* x, int dtype, const double* qstat, const double* xstat,
                                     int m, int n, int d, int k, int q0, int nq, int64_t* out_idx, double* out_dist,
                                     ava_stream_t s) {
  if (q == nullptr || x == nullptr || qstat == nullptr || xstat == nullptr || out_idx == nullptr ||
      out_dist == nullptr || (dtype != 0 && dtype != 1) || n < 1 || m < 1 || d < 1 || d > 65536 || k < 1 ||
      k > PJ_MAX_K || k > n || q0 < 0 || nq < 1 || (int64_t)q0 + nq > m)
    return AVA_EINVAL;
  if (dtype == 0)
    return pj_knn_corr_launch<float>(q, x, qstat, xstat, n, d, k, q0, nq, 0, out_idx, out_dist, to_stream(s));
  return pj_knn_corr_launch<double>(q, x, qstat, xstat, n, d, k, q0, nq, 0, out_idx, out_dist, to_stream(s));
}

static int pj_smooth_launch(const double* dist, const int64_t* idx, int n, int k, double local_connectivity,
                            int bipartite, double* mean_all, double* sigma, double* rho, double* w, ava_stream_t s) {
  if (dist == nullptr || idx == nullptr || mean_all == nullptr || sigma == nullptr || rho == nullptr ||
      w == nullptr || n < 1 || k < 1 || k > PJ_MAX_K || !(local_connectivity >= 0.0))
    return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  hipLaunchKernelGGL(pj_mean_kernel, dim3(1), dim3(256), 0, st, dist, n, k, mean_all);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(pj_smooth_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, dist, idx, n, k, local_connectivity,
                     bipartite, mean_all, sigma, rho, w);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_pj_smooth(const double* dist, const int64_t* idx, int n, int k, double local_connectivity,
                             double* mean_all, double* sigma, double* rho, double* w, ava_stream_t s) {
  return pj_smooth_launch(dist, idx, n, k, local_connectivity, 0, mean_all, sigma, rho, w, s);
}

extern "C" int ava_pj_smooth_bipartite(const double* dist, const int64_t* idx, int n, int k,
                                       double local_connectivity, double* mean_all, double* sigma, double* rho,
                                       double* w, ava_stream_t s) {
  return pj_smooth_launch(dist, idx, n, k, local_connectivity, 1, mean_all, sigma, rho, w, s);
}

extern "C" int ava_pj_layout(double* y, double* y_tmp, const int64_t* indptr, const int* col, const double* eps,
                             const double* epn, double* next_s, double* next_n, int n, int64_t nnz, int e0, int e1,
                             int n_epochs, double learning_rate, double a, double b, double gamma, uint64_t salt,
                             int* flag, ava_stream_t s) {
  if (y == nullptr || y_tmp == nullptr || indptr == nullptr || flag == nullptr || n < 1 || nnz < 0 || e0 < 0 ||
      e1 < e0 || e1 > n_epochs || (nnz > 0 && (col == nullptr || eps == nullptr || epn == nullptr ||
                                               next_s == nullptr || next_n == nullptr)))
    return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  double* cur = y;
  double* nxt = y_tmp;
  for (int ep = e0; ep < e1; ++ep) {
    const double alpha = ep == 0 ? learning_rate : learning_rate * (1.0 - (double)(ep - 1) / (double)n_epochs);
    // one-wave workgroups: the thread per vertex is latency-bound on its gathers, so spread the vertices over all CUs
    hipLaunchKernelGGL(pj_layout_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, st, cur, nxt, indptr, col, eps, epn,
                       next_s, next_n, n, nnz, ep, alpha, a, b, gamma, salt, flag);
    AVA_CHECK_LAUNCH();
    double* tmp = cur;
    cur = nxt;
    nxt = tmp;
  }
  if (cur != y && hipMemcpyAsync(y, cur, 2 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return AVA_ELAUNCH;
  return AVA_OK;
}

extern "C" int ava_pj_transform_init(const double* w, const int64_t* idx, const double* emb, int m, int k,
                                     double* wn, double* y0, ava_stream_t s) {
  if (w == nullptr || idx == nullptr || emb == nullptr || wn == nullptr || y0 == nullptr || m < 1 || k < 1 ||
      k > PJ_MAX_K)
    return AVA_EINVAL;
  hipLaunchKernelGGL(pj_transform_init_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, to_stream(s), w, idx, emb, m, k,
                     wn, y0);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_pj_transform_layout(double* y, const double* emb, const int64_t* idx, const double* eps,
                                       const double* epn, int m, int k, int n_train, int epochs, int n_epochs,
                                       double learning_rate, double a, double b, double gamma, uint64_t salt,
                                       int* flag, ava_stream_t s) {
  if (y == nullptr || emb == nullptr || idx == nullptr || eps == nullptr || epn == nullptr || flag == nullptr ||
      m < 1 || k < 1 || k > PJ_MAX_K || n_train < 1 || epochs < 0 || n_epochs < 1 || epochs > n_epochs)
    return AVA_EINVAL;
  if (epochs == 0) return AVA_OK;
  // one-wave workgroups, as the fit layout: a row is a chain of dependent gathers, so the rows go to as many CUs as
  // there are; the two counters of every slot take k KiB of LDS per workgroup
  const size_t lds = (size_t)k * 64 * 2 * sizeof(double);
  hipLaunchKernelGGL(pj_transform_layout_kernel, dim3(ceil_div(m, 64)), dim3(64), lds, to_stream(s), y, emb, idx, eps,
                     epn, m, k, n_train, epochs, n_epochs, learning_rate / 4.0, a, b, gamma, salt, flag);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

static int pj_gram_rows(int n) {
  const int r = ceil_div(n, 256);
  return r < 2048 ? 2048 : ceil_div(r, PJ_GR) * PJ_GR;
}

extern "C" size_t ava_pj_gram_workspace_bytes(int n, int d) {
  if (n < 1 || d < 1 || d > PJ_MAX_PCA_DIM) return 0;
  const size_t D = (size_t)d + 1;
  return (size_t)ceil_div(n, pj_gram_rows(n)) * D * D * sizeof(double);
}

template <typename T>
static void pj_gram_launch(const void* x, int n, int d, double* part, hipStream_t st) {
  const int tiles = ceil_div(d + 1, PJ_GT), rows = pj_gram_rows(n);
  hipLaunchKernelGGL(pj_gram_kernel<T>, dim3(tiles * tiles, ceil_div(n, rows)), dim3(256), 0, st,
                     reinterpret_cast<const T*>(x), n, d, rows, tiles, part);
}

extern "C" int ava_pj_gram(const void* x, int dtype, int n, int d, double* gram, void* ws, size_t ws_bytes,
                           ava_stream_t s) {
  if (x == nullptr || gram == nullptr || ws == nullptr || (dtype != 0 && dtype != 1) || n < 1 || d < 1 ||
      d > PJ_MAX_PCA_DIM)
    return AVA_EINVAL;
  if (ws_bytes < ava_pj_gram_workspace_bytes(n, d)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  double* part = reinterpret_cast<double*>(ws);
  if (dtype == 0) pj_gram_launch<float>(x, n, d, part, st);
  else pj_gram_launch<double>(x, n, d, part, st);
  AVA_CHECK_LAUNCH();
  const int DD = (d + 1) * (d + 1);
  hipLaunchKernelGGL(pj_gram_reduce_kernel, dim3(ceil_div(DD, 256)), dim3(256), 0, st, part,
                     ceil_div(n, pj_gram_rows(n)), DD, gram);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_pj_project(const void* x, int dtype, int n, int d, const double* V, const double* muv, int nc,
                              double* out, ava_stream_t s) {
  if (x == nullptr || V == nullptr || muv == nullptr || out == nullptr || (dtype != 0 && dtype != 1) || n < 1 ||
      d < 1 || nc < 1 || nc > d)
    return AVA_EINVAL;
  const int64_t total = (int64_t)n * nc;
  const int64_t blocks = ceil_div64(total, 256);
  if (blocks > 0x7fffffff) return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  if (dtype == 0)
    hipLaunchKernelGGL(pj_project_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st,
                       reinterpret_cast<const float*>(x), n, d, V, muv, nc, out);
  else
    hipLaunchKernelGGL(pj_project_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st,
                       reinterpret_cast<const double*>(x), n, d, V, muv, nc, out);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
