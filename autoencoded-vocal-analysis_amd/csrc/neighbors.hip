// Exact 1-nearest-neighbour search.
//
// Replaces the two searches of the reference's shotgun_movie_DC (ava/plotting/shotgun_movie.py:126-133, 148-158):
// sklearn's NearestNeighbors(n_neighbors=1, metric='correlation') over whole spectrograms (brute force through
// scipy's fp64 cdist) and the Python loop np.argmin([euclidean(latent[i], j) for j in original_latent]).  All
// arithmetic is fp64, like scipy's.
//
// Correlation: scipy centres both operands (x - mean(x)) and takes the cosine distance of the centred rows.  Here the
// row statistics kernel computes every row's fp64 mean and centred sum of squares, and the tile kernel subtracts the
// mean while it converts the operands to fp64 into LDS; the statistics, the staging and the MFMA stage are the shared
// pieces of corr_tile.h, which states the order of every sum.  A
// workgroup owns 128 queries x 128 references; each of its four waves a 64 x 64 quarter, i.e. 4 x 4 blocks of
// v_mfma_f64_16x16x4_f64 (16 accumulators of 4 doubles per lane).  The epilogue forms 1 - dot / sqrt(ss_q ss_r)
// (clipped to [0, 2] as scipy clips the cosine) and writes one (dist, idx) partial per (query, reference tile).
//
// Euclidean: the fp64 direct-difference tile of sqdist_tile.h (64 x 64 pairs, a 4 x 4 block per thread), then sqrt
// (the reference compares the square roots).
//
// A fixed-order reduce kernel combines the partials of each query.  The candidates are ordered by nn_better, a total
// order, so every tile, every reduce step and the host's merge of reference chunks pick the same winner: the result
// is bit-reproducible and independent of the tiling and of the chunking (the euclidean sums: the order contract of
// sqdist_tile.h; the correlation dot products: that of corr_tile.h).
//   ties        equal distances resolve to the lowest reference index
//   correlation a zero-variance row gives NaN (0 / 0, as scipy); NaN loses to any number; a query whose distances are
//               all NaN gets index 0 and distance NaN
//   euclidean   NaN wins and the first NaN is taken, as np.argmin does
#include "common.h"
#include "corr_tile.h"
#include "sqdist_tile.h"

#define NN_CORR 0
#define NN_EUCL 1

#define NC_BQ 128        // correlation tile: queries
#define NC_BR 128        //                   references

// true when candidate (d1, i1) beats (d2, i2); an empty candidate (index < 0) loses to everything
__device__ __forceinline__ bool nn_better(double d1, int64_t i1, double d2, int64_t i2, int nan_wins) {
  if (i2 < 0) return i1 >= 0;
  if (i1 < 0) return false;
  const bool n1 = isnan(d1), n2 = isnan(d2);
  if (n1 != n2) return nan_wins ? n1 : n2;
  if (!n1 && d1 != d2) return d1 < d2;
  return i1 < i2;
}

// best of the 16 lanes that share lane >> 4 (xor butterfly: every lane ends with the same winner)
__device__ __forceinline__ void nn_best16(double& d, int64_t& i, int nan_wins) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const double od = __shfl_xor(d, o, 64);
    const int64_t oi = __shfl_xor(i, o, 64);
    if (nn_better(od, oi, d, i, nan_wins)) { d = od; i = oi; }
  }
}

// stats[2 r] = mean of row r, stats[2 r + 1] = sum_k (x_rk - mean)^2: one workgroup per row, fixed order
template <typename T>
__global__ __launch_bounds__(256) void nn_row_stats_kernel(const T* __restrict__ x, int d, double* __restrict__ stats) {
  __shared__ double red[4];
  corr_row_stats(x + (size_t)blockIdx.x * d, d, threadIdx.x, red, stats + 2 * (size_t)blockIdx.x);
}

// one (dist, idx) partial per (query, 128-reference tile): partial[q * rtiles + tile]
template <typename TQ, typename TR>
__global__ __launch_bounds__(256) void nn_corr_kernel(const TQ* __restrict__ Q, int nq, const TR* __restrict__ R, int nr,
                                                      int d, const double* __restrict__ qstat,
                                                      const double* __restrict__ rstat, int rtiles,
                                                      double* __restrict__ pdist, int64_t* __restrict__ pidx) {
  __shared__ double qs[NC_BQ * CORR_LD];
  __shared__ double rs[NC_BR * CORR_LD];
  __shared__ double qm[NC_BQ], rm[NC_BR];
  __shared__ double bd[2][NC_BQ];
  __shared__ int64_t bi[2][NC_BQ];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wq = w & 1, wr = w >> 1;                 // this wave's 64 x 64 quarter of the tile
  const int rt = blockIdx.x;
  const int q0 = blockIdx.y * NC_BQ, r0 = rt * NC_BR;
  if (t < NC_BQ) {
    qm[t] = q0 + t < nq ? qstat[2 * (size_t)(q0 + t)] : 0.0;
  } else {
    rm[t - NC_BQ] = r0 + t - NC_BQ < nr ? rstat[2 * (size_t)(r0 + t - NC_BQ)] : 0.0;
  }
  TQ vq[NC_BQ / 16];
  TR vr[NC_BR / 16];
  corr_d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = corr_d4{0.0, 0.0, 0.0, 0.0};
  corr_fetch<NC_BQ>(vq, Q, q0, nq, d, 0, t);
  corr_fetch<NC_BR>(vr, R, r0, nr, d, 0, t);
  __syncthreads();                                   // qm / rm
  for (int k0 = 0; k0 < d; k0 += CORR_KC) {
    corr_store<NC_BQ>(qs, vq, qm, q0, nq, d, k0, t);
    corr_store<NC_BR>(rs, vr, rm, r0, nr, d, k0, t);
    __syncthreads();
    if (k0 + CORR_KC < d) {                          // next stage's loads in flight during the MFMAs
      corr_fetch<NC_BQ>(vq, Q, q0, nq, d, k0 + CORR_KC, t);
      corr_fetch<NC_BR>(vr, R, r0, nr, d, k0 + CORR_KC, t);
    }
    corr_mfma_stage<4, 4>(qs, rs, wq * 64, wr * 64, lane, acc);
    __syncthreads();
  }
  // epilogue: f64 C/D layout col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int lr = wq * 64 + a * 16 + (lane >> 4) + 4 * reg;
      const int gq = q0 + lr;
      const double ssq = gq < nq ? qstat[2 * (size_t)gq + 1] : 1.0;
      double best = 0.0;
      int64_t besti = -1;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int gr = r0 + wr * 64 + b * 16 + (lane & 15);
        if (gr < nr) {
          double c = acc[a][b][reg] / sqrt(ssq * rstat[2 * (size_t)gr + 1]);
          if (fabs(c) > 1.0) c = copysign(1.0, c);
          const double dist = 1.0 - c;
          if (nn_better(dist, gr, best, besti, 0)) { best = dist; besti = gr; }
        }
      }
      nn_best16(best, besti, 0);
      if ((lane & 15) == 0) { bd[wr][lr] = best; bi[wr][lr] = besti; }
    }
  }
  __syncthreads();
  if (t < NC_BQ && q0 + t < nq) {
    double best = bd[0][t];
    int64_t besti = bi[0][t];
    if (nn_better(bd[1][t], bi[1][t], best, besti, 0)) { best = bd[1][t]; besti = bi[1][t]; }
    pdist[(size_t)(q0 + t) * rtiles + rt] = best;
    pidx[(size_t)(q0 + t) * rtiles + rt] = besti;
  }
}

// one (dist, idx) partial per (query, 64-reference tile); thread (ty, tx) owns queries ty + 16 i, references tx + 16 j
template <typename TQ, typename TR>
__global__ __launch_bounds__(256) void nn_eucl_kernel(const TQ* __restrict__ Q, int nq, const TR* __restrict__ R, int nr,
                                                      int d, int rtiles, double* __restrict__ pdist,
                                                      int64_t* __restrict__ pidx) {
  __shared__ double xs[SQD_T * SQD_LD];
  __shared__ double ys[SQD_T * SQD_LD];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int rt = blockIdx.x;
  const int q0 = blockIdx.y * SQD_T, r0 = rt * SQD_T;
  double acc[4][4];
  sqd_tile(xs, ys, Q, q0, nq, R, r0, nr, d, t, acc);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double best = 0.0;
    int64_t besti = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gr = r0 + tx + 16 * j;
      if (gr < nr) {
        const double dist = sqrt(acc[i][j]);
        if (nn_better(dist, gr, best, besti, 1)) { best = dist; besti = gr; }
      }
    }
    nn_best16(best, besti, 1);
    const int gq = q0 + ty + 16 * i;
    if (tx == 0 && gq < nq) {
      pdist[(size_t)gq * rtiles + rt] = best;
      pidx[(size_t)gq * rtiles + rt] = besti;
    }
  }
}

// one wave per query: lane l folds partials l, l + 64, ... in order, then a fixed butterfly
__global__ __launch_bounds__(256) void nn_reduce_kernel(const double* __restrict__ pdist,
                                                        const int64_t* __restrict__ pidx, int nq, int rtiles,
                                                        int nan_wins, int64_t* __restrict__ out_idx,
                                                        double* __restrict__ out_dist) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= nq) return;                               // uniform per wave
  double best = 0.0;
  int64_t besti = -1;
  for (int j = lane; j < rtiles; j += 64) {
    const double dd = pdist[(size_t)q * rtiles + j];
    const int64_t ii = pidx[(size_t)q * rtiles + j];
    if (nn_better(dd, ii, best, besti, nan_wins)) { best = dd; besti = ii; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(best, o, 64);
    const int64_t oi = __shfl_xor(besti, o, 64);
    if (nn_better(od, oi, best, besti, nan_wins)) { best = od; besti = oi; }
  }
  if (lane == 0) {
    out_idx[q] = besti;
    out_dist[q] = best;
  }
}

__global__ __launch_bounds__(256) void nn_merge_kernel(int64_t* __restrict__ best_idx, double* __restrict__ best_dist,
                                                       const int64_t* __restrict__ idx,
                                                       const double* __restrict__ dist, int nq, int64_t offset,
                                                       int nan_wins) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int64_t i = idx[q] + offset;
  const double dd = dist[q];
  if (nn_better(dd, i, best_dist[q], best_idx[q], nan_wins)) {
    best_idx[q] = i;
    best_dist[q] = dd;
  }
}

static inline int nn_tile(int metric) { return metric == NN_CORR ? NC_BR : SQD_T; }

static bool nn_shape_ok(int nq, int nr, int d, int metric) {
  if (nq < 1 || nr < 1 || d < 1 || d > 65536 || (metric != NN_CORR && metric != NN_EUCL)) return false;
  const int qt = metric == NN_CORR ? NC_BQ : SQD_T;
  return ceil_div(nq, qt) <= 65535;                  // grid.y
}

extern "C" size_t ava_nn_workspace_bytes(int nq, int nr, int d, int metric) {
  if (!nn_shape_ok(nq, nr, d, metric)) return 0;
  const size_t rtiles = ceil_div(nr, nn_tile(metric));
  const size_t stats = metric == NN_CORR ? 2 * ((size_t)nq + nr) : 0;
  return (stats + 2 * (size_t)nq * rtiles) * sizeof(double);
}

template <typename TQ, typename TR>
static int nn_launch(const void* queries, int nq, const void* refs, int nr, int d, int metric, double* stats,
                     double* pdist, int64_t* pidx, int rtiles, hipStream_t st) {
  const TQ* Q = reinterpret_cast<const TQ*>(queries);
  const TR* R = reinterpret_cast<const TR*>(refs);
  if (metric == NN_CORR) {
    double* qstat = stats;
    double* rstat = stats + 2 * (size_t)nq;
    hipLaunchKernelGGL(nn_row_stats_kernel<TQ>, dim3(nq), dim3(256), 0, st, Q, d, qstat);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_row_stats_kernel<TR>, dim3(nr), dim3(256), 0, st, R, d, rstat);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL((nn_corr_kernel<TQ, TR>), dim3(rtiles, ceil_div(nq, NC_BQ)), dim3(256), 0, st, Q, nq, R, nr, d,
                       qstat, rstat, rtiles, pdist, pidx);
  } else {
    hipLaunchKernelGGL((nn_eucl_kernel<TQ, TR>), dim3(rtiles, ceil_div(nq, SQD_T)), dim3(256), 0, st, Q, nq, R, nr, d,
                       rtiles, pdist, pidx);
  }
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_nn_argmin(const void* queries, int q_dtype, int nq, const void* refs, int r_dtype, int nr, int d,
                             int metric, int64_t* out_idx, double* out_dist, void* ws, size_t ws_bytes,
                             ava_stream_t s) {
  if (queries == nullptr || refs == nullptr || out_idx == nullptr || out_dist == nullptr || ws == nullptr ||
      (q_dtype != 0 && q_dtype != 1) || (r_dtype != 0 && r_dtype != 1) || !nn_shape_ok(nq, nr, d, metric))
    return AVA_EINVAL;
  if (ws_bytes < ava_nn_workspace_bytes(nq, nr, d, metric)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  const int rtiles = ceil_div(nr, nn_tile(metric));
  double* stats = reinterpret_cast<double*>(ws);
  double* pdist = stats + (metric == NN_CORR ? 2 * ((size_t)nq + nr) : 0);
  int64_t* pidx = reinterpret_cast<int64_t*>(pdist + (size_t)nq * rtiles);
  int rc;
  if (q_dtype == 0 && r_dtype == 0)
    rc = nn_launch<float, float>(queries, nq, refs, nr, d, metric, stats, pdist, pidx, rtiles, st);
  else if (q_dtype == 0)
    rc = nn_launch<float, double>(queries, nq, refs, nr, d, metric, stats, pdist, pidx, rtiles, st);
  else if (r_dtype == 0)
    rc = nn_launch<double, float>(queries, nq, refs, nr, d, metric, stats, pdist, pidx, rtiles, st);
  else
    rc = nn_launch<double, double>(queries, nq, refs, nr, d, metric, stats, pdist, pidx, rtiles, st);
  if (rc != AVA_OK) return rc;
  hipLaunchKernelGGL(nn_reduce_kernel, dim3(ceil_div(nq, 4)), dim3(256), 0, st, pdist, pidx, nq, rtiles,
                     metric == NN_EUCL ? 1 : 0, out_idx, out_dist);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_nn_merge(int64_t* best_idx, double* best_dist, const int64_t* idx, const double* dist, int nq,
                            int64_t offset, int metric, ava_stream_t s) {
  if (best_idx == nullptr || best_dist == nullptr || idx == nullptr || dist == nullptr || nq < 1 || offset < 0 ||
      (metric != NN_CORR && metric != NN_EUCL))
    return AVA_EINVAL;
  hipLaunchKernelGGL(nn_merge_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, to_stream(s), best_idx, best_dist, idx,
                     dist, nq, offset, metric == NN_EUCL ? 1 : 0);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
