// Lloyd k-means with k-means++ seeding of latent means: the device counterpart of
// scikit-learn 1.7's KMeans(algorithm='lloyd') (sklearn/cluster/_kmeans.py: _kmeans_plusplus, _init_centroids,
// _tolerance, _kmeans_single_lloyd; _k_means_common.pyx: _relocate_empty_clusters_dense, _inertia_dense).  X is [N][d]
// float32 or float64 and is converted on load; the C ABI is the ava_km_ block of include/ava_hip.h.
//
// The model (ava_amd/kmeans.py states the same; tests/kmeans_cases.py restates it in numpy):
//   arithmetic   all fp64, also for float32 rows.  Every distance is the tile of sqdist_tile.h or a scalar loop in its
//                order (direct differences, fma, features ascending from 0): a (row, centre) or (row, row) pair has the
//                bits ava_pair_sqdist gives it.  Rows are not centred: sklearn subtracts the column means only to tame its
//                |x|^2 - 2 x.c + |c|^2 expansion, which is not used here.
//   assignment   each row takes its nearest centre, the lowest index on a tie (np.argmin)
//   sums         no floating-point atomics.  Every sum over rows (per-cluster sum of x, counts, inertia, the k-means++
//                potentials and scan, the column means and variances) is taken inside chunks of KM_CHUNK = 2048 rows in
//                ascending row order from 0, and the chunk partials are added in ascending chunk order from 0.  So a fit
//                gives the same bits on every run, for float32 and float64 copies of the same values, and however its
//                iterations are split over calls of ava_km_fit.
//   k-means++    the host makes sklearn's draws.  The device keeps closest [N], forms its inclusive scan (sequential
//                inside the chunks, scan[r] = offset[chunk] + local, the offsets the ascending sums of the chunk totals;
//                its last entry is the potential), finds the L candidates as searchsorted(scan, r * potential) clipped
//                to N - 1, forms min(closest, d2(candidate, .)) and the L potentials, takes the candidate of least
//                potential (the first on a tie) and commits its minimum as the new closest.  The chosen rows are written
//                to a device array: the host reads nothing between centres.
//   iteration    sklearn's loop: assign; new centres = sum / count (empty clusters below); shift = sum_k |c_new - c_old|^2
//                (features ascending by fma inside a centre, centres ascending); stop when no label changed (strict), else
//                when shift <= tol * mean(var(X, axis=0)).  After the loop one more assignment at the final centres gives
//                the labels, each row's d2 and the inertia sum d2; after a strict stop the final centres have the bits of
//                the ones before them, so that assignment repeats the labels.
//   empty        the empty clusters, in ascending id, take the rows with the largest d2 to their own centre of this
//                iteration, the lowest row on a tie; each such row leaves its old cluster's sum and count (its label
//                stays, as in sklearn).  A cluster left without rows by that keeps its sum as its centre, as sklearn's
//                _average_centers does.  sklearn's argpartition leaves the order among several such rows unspecified.
//
// One iteration is four launches:
//   1. km_assign_kernel   a workgroup per 64 rows; the centres pass in tiles of 64 through sqd_tile; a running (d2, index)
//                         per row; writes labels, d2 and the tile's count of changed labels; no [N][K] array
//   2. km_sums_kernel     per (chunk, slab of KM_SLAB = 16 features): sum of x and counts per cluster, in registers for
//      km_sums_lds_kernel K <= 64 and in LDS above.  The rows are staged 64 at a time in LDS; thread (g, col) owns column
//                         col of the clusters k with k % 16 == g and walks the staged rows in ascending order, so every
//                         cluster's sum takes its rows ascending.  Also the chunk's sum of d2.
//   3. km_reduce_kernel   a workgroup per cluster: the chunk partials in ascending order
//   4. km_finish_kernel   one workgroup: relocation, means, shift, the changed count, the stopping rule
// Iterations without the host (the design of ava_gm_fit): ctl[0] = 1 after a strict stop, ctl[1] the number of iterations
// that ran, ctl[2 + it] whether the loop had stopped BEFORE iteration it.  Every launch of iteration it begins with a
// uniform read of ctl[2 + it] and returns at once if it is set; km_finish_kernel writes ctl[1] = it + 1 and
// ctl[2 + it + 1].
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "sqdist_tile.h"

#define KM_MAX_D 128
#define KM_MAX_K 256
#define KM_CHUNK 2048            // rows of a chunk of the partial sums: a constant, never derived from the grid
#define KM_SLAB 16               // features of a workgroup of km_sums_kernel
#define KM_GROUPS 16             // cluster groups of km_sums_kernel: 256 threads = KM_GROUPS x KM_SLAB
#define KM_ST 64                 // rows of a stage of km_sums_kernel
#define KM_REG_K 64              // km_sums_kernel keeps the sums in registers up to this K, km_sums_lds_kernel in LDS above
#define KM_MAX_TRIALS 8          // 2 + int(log 256) = 7 candidates at most
#define KM_MAX_N (INT_MAX - 63)  // the last tile's row indices stay in an int

static inline int km_chunks(int n) { return (int)(((int64_t)n + KM_CHUNK - 1) / KM_CHUNK); }
static inline int km_tiles(int n) { return (int)(((int64_t)n + SQD_T - 1) / SQD_T); }
static inline bool km_rows_ok(int n, int d) { return n >= 1 && n <= KM_MAX_N && d >= 1 && d <= KM_MAX_D; }
// k <= n is a rule of a fit (ava_km_fit); rows are assigned to, or moved between, more centres than there are rows
static inline bool km_shape_ok(int n, int d, int k) { return km_rows_ok(n, d) && k >= 1 && k <= KM_MAX_K; }

__device__ __forceinline__ bool km_stopped(const int* __restrict__ ctl, int it) { return ctl != nullptr && ctl[2 + it] != 0; }

struct km_ws {
  double* vpart;   // [chunks][d]   column sums of a chunk (ava_km_variance)
  double* vmean;   // [d]
  double* ctot;    // [chunks]      chunk totals of closest
  double* coff;    // [chunks + 1]  their exclusive ascending sums; the last is the potential
  double* ppart;   // [chunks][KM_MAX_TRIALS]  chunk potentials of the candidates
  int* cand;       // [KM_MAX_TRIALS]
  double* psum;    // [chunks][k][d]
  int* pcnt;       // [chunks][k]
  double* pin;     // [chunks]      chunk sums of d2
  double* csum;    // [k][d]
  int* cnt;        // [k]
  int* tchg;       // [tiles]       changed labels per assign tile
};

static size_t km_ws_layout(int n, int d, int k, void* base, km_ws* w) {
  const size_t chunks = (size_t)km_chunks(n);
  ava_ws_cursor c(base);
  w->vpart = c.take<double>(chunks * d);
  w->vmean = c.take<double>(d);
  w->ctot = c.take<double>(chunks);
  w->coff = c.take<double>(chunks + 1);
  w->ppart = c.take<double>(chunks * KM_MAX_TRIALS);
  w->cand = c.take<int>(KM_MAX_TRIALS);
  w->psum = c.take<double>(chunks * k * d);
  w->pcnt = c.take<int>(chunks * k);
  w->pin = c.take<double>(chunks);
  w->csum = c.take<double>((size_t)k * d);
  w->cnt = c.take<int>(k);
  w->tchg = c.take<int>((size_t)km_tiles(n));
  return c.bytes();
}

// ---- assignment -------------------------------------------------------------------------------------------------------
// (v, idx) precedes (bv, bi): nearer, or as near with the lower index
__device__ __forceinline__ bool km_nearer(double v, int idx, double bv, int bi) { return v < bv || (v == bv && idx < bi); }

template <typename T>
__global__ __launch_bounds__(256) void km_assign_kernel(const T* __restrict__ X, int n, int d, int K,
                                                        const double* __restrict__ C, int* __restrict__ labels,
                                                        double* __restrict__ d2out, int* __restrict__ tchg,
                                                        const int* __restrict__ ctl, int it) {
  if (km_stopped(ctl, it)) return;
  __shared__ double xs[SQD_T * SQD_LD], ys[SQD_T * SQD_LD];
  __shared__ int chg[SQD_T];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int q0 = blockIdx.x * SQD_T;
  double best[4];
  int bi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) best[i] = INFINITY, bi[i] = INT_MAX;
  for (int c0 = 0; c0 < K; c0 += SQD_T) {
    double acc[4][4];
    sqd_tile(xs, ys, X, q0, n, C, c0, K, d, t, acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = c0 + tx + 16 * j;
      if (idx < K) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (km_nearer(acc[i][j], idx, best[i], bi[i])) best[i] = acc[i][j], bi[i] = idx;
      }
    }
  }
  // the 16 lanes of a row are consecutive lanes of one wave
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const double ov = __shfl_xor(best[i], o, 64);
      const int oi = __shfl_xor(bi[i], o, 64);
      if (km_nearer(ov, oi, best[i], bi[i])) best[i] = ov, bi[i] = oi;
    }
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = ty + 16 * i;
      int changed = 0;
      if (q0 + lr < n) {
        const size_t r = (size_t)q0 + lr;
        const int lab = bi[i] == INT_MAX ? 0 : bi[i];          // no distance compared: NaN rows, refused by the host
        changed = labels[r] != lab;
        labels[r] = lab;
        d2out[r] = best[i];
      }
      chg[lr] = changed;
    }
  }
  if (tchg != nullptr) {
    __syncthreads();
    if (t == 0) {
      int s = 0;
      for (int i = 0; i < SQD_T; ++i) s += chg[i];
      tchg[blockIdx.x] = s;
    }
  }
}

// ---- per-cluster sums of a chunk ---------------------------------------------------------------------------------------
// NS = ceil(K / KM_GROUPS) accumulators per thread, in registers: thread (g, col) owns column col of the clusters
// g + KM_GROUPS s, s < NS.  Every staged row is offered to every accumulator and taken by the one it belongs to (a
// select, not an addition of zero), so the loop has no store and no dependence but each accumulator's own chain, and a
// cluster's sum still takes its rows in ascending order.
template <typename T, int NS>
__global__ __launch_bounds__(256) void km_sums_kernel(const T* __restrict__ X, int n, int d, int K,
                                                      const int* __restrict__ labels, const double* __restrict__ d2,
                                                      double* __restrict__ psum, int* __restrict__ pcnt,
                                                      double* __restrict__ pin, const int* __restrict__ ctl, int it) {
  if (km_stopped(ctl, it)) return;
  __shared__ double xt[KM_ST * KM_SLAB];
  __shared__ double dt[KM_ST];
  __shared__ int lt[KM_ST];
  const int t = threadIdx.x, col = t & (KM_SLAB - 1), g = t / KM_SLAB;
  const int chunk = blockIdx.x, j0 = blockIdx.y * KM_SLAB;
  double acc[NS];
  int cnt[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0, cnt[s] = 0;
  const int64_t r0 = (int64_t)chunk * KM_CHUNK;
  const int rows = (int)((int64_t)n - r0 < KM_CHUNK ? (int64_t)n - r0 : KM_CHUNK);
  double inert = 0.0;
  for (int s0 = 0; s0 < rows; s0 += KM_ST) {
    __syncthreads();                                           // the stage before is consumed
    const int ns = rows - s0 < KM_ST ? rows - s0 : KM_ST;
#pragma unroll
    for (int q = 0; q < KM_ST * KM_SLAB / 256; ++q) {
      const int e = t + 256 * q, rr = e / KM_SLAB, cc = e % KM_SLAB;
      xt[e] = (rr < ns && j0 + cc < d) ? (double)X[(size_t)(r0 + s0 + rr) * d + j0 + cc] : 0.0;
    }
    if (t < KM_ST) {
      const int lab = t < ns ? labels[r0 + s0 + t] : -1;
      lt[t] = (lab >= 0 && lab < K) ? lab : -1;                // a label outside [0, K) is in no cluster
      dt[t] = (d2 != nullptr && t < ns) ? d2[r0 + s0 + t] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int rr = 0; rr < ns; ++rr) {
      const int lab = lt[rr];
      const double x = xt[rr * KM_SLAB + col];
      const int slot = (lab & (KM_GROUPS - 1)) == g ? lab / KM_GROUPS : -1;      // lab = -1: -1 & 15 = 15, -1 / 16 = 0
      const int mine = lab >= 0 ? slot : -1;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const double sum = acc[s] + x;
        acc[s] = mine == s ? sum : acc[s];
        cnt[s] += mine == s ? 1 : 0;
      }
    }
    if (t == 0 && blockIdx.y == 0)
      for (int rr = 0; rr < ns; ++rr) inert += dt[rr];
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int k = g + KM_GROUPS * s;
    if (k < K) {
      if (j0 + col < d) psum[((size_t)chunk * K + k) * d + j0 + col] = acc[s];
      if (col == 0 && blockIdx.y == 0) pcnt[(size_t)chunk * K + k] = cnt[s];
    }
  }
  if (t == 0 && blockIdx.y == 0) pin[chunk] = inert;
}

// The same sums for K > KM_REG_K, where a thread would own more than 4 clusters and offering every row to every
// accumulator costs more than it saves (measured: profiles/NOTES.md): the sums and counts are in LDS, K x KM_SLAB x 8 B =
// 32 KiB at K = 256, and thread (g, col) adds a staged row to the one entry it belongs to.  Same owner, same order.
template <typename T>
__global__ __launch_bounds__(256) void km_sums_lds_kernel(const T* __restrict__ X, int n, int d, int K,
                                                          const int* __restrict__ labels, const double* __restrict__ d2,
                                                          double* __restrict__ psum, int* __restrict__ pcnt,
                                                          double* __restrict__ pin, const int* __restrict__ ctl, int it) {
  if (km_stopped(ctl, it)) return;
  __shared__ double sums[KM_MAX_K * KM_SLAB];
  __shared__ int cnts[KM_MAX_K];
  __shared__ double xt[KM_ST * KM_SLAB];
  __shared__ double dt[KM_ST];
  __shared__ int lt[KM_ST];
  const int t = threadIdx.x, col = t & (KM_SLAB - 1), g = t / KM_SLAB;
  const int chunk = blockIdx.x, j0 = blockIdx.y * KM_SLAB;
  for (int i = t; i < K * KM_SLAB; i += 256) sums[i] = 0.0;
  for (int i = t; i < K; i += 256) cnts[i] = 0;
  const int64_t r0 = (int64_t)chunk * KM_CHUNK;
  const int rows = (int)((int64_t)n - r0 < KM_CHUNK ? (int64_t)n - r0 : KM_CHUNK);
  double inert = 0.0;
  for (int s0 = 0; s0 < rows; s0 += KM_ST) {
    __syncthreads();                                           // the stage before is consumed (and the zeroing done)
    const int ns = rows - s0 < KM_ST ? rows - s0 : KM_ST;
#pragma unroll
    for (int q = 0; q < KM_ST * KM_SLAB / 256; ++q) {
      const int e = t + 256 * q, rr = e / KM_SLAB, cc = e % KM_SLAB;
      xt[e] = (rr < ns && j0 + cc < d) ? (double)X[(size_t)(r0 + s0 + rr) * d + j0 + cc] : 0.0;
    }
    if (t < KM_ST) {
      lt[t] = t < ns ? labels[r0 + s0 + t] : -1;
      dt[t] = (d2 != nullptr && t < ns) ? d2[r0 + s0 + t] : 0.0;
    }
    __syncthreads();
    for (int rr = 0; rr < ns; ++rr) {
      const int lab = lt[rr];
      if (lab >= 0 && lab < K && (lab & (KM_GROUPS - 1)) == g) {
        sums[lab * KM_SLAB + col] += xt[rr * KM_SLAB + col];
        if (col == 0) cnts[lab] += 1;
      }
    }
    if (t == 0 && blockIdx.y == 0)
      for (int rr = 0; rr < ns; ++rr) inert += dt[rr];
  }
  __syncthreads();
  for (int i = t; i < K * KM_SLAB; i += 256) {
    const int k = i / KM_SLAB, c = i % KM_SLAB;
    if (j0 + c < d) psum[((size_t)chunk * K + k) * d + j0 + c] = sums[i];
  }
  if (blockIdx.y == 0) {
    for (int i = t; i < K; i += 256) pcnt[(size_t)chunk * K + i] = cnts[i];
    if (t == 0) pin[chunk] = inert;
  }
}

// a workgroup per cluster, 128 threads: the chunk partials in ascending order; workgroup 0 also the sum of d2
__global__ __launch_bounds__(128) void km_reduce_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt,
                                                        const double* __restrict__ pin, int chunks, int d, int K,
                                                        double* __restrict__ csum, int* __restrict__ cnt,
                                                        double* __restrict__ inertia, const int* __restrict__ ctl, int it) {
  if (km_stopped(ctl, it)) return;
  const int k = blockIdx.x, j = threadIdx.x;
  if (j < d) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += psum[((size_t)c * K + k) * d + j];
    csum[(size_t)k * d + j] = s;
  }
  if (j == 0) {
    int m = 0;
    for (int c = 0; c < chunks; ++c) m += pcnt[(size_t)c * K + k];
    cnt[k] = m;
    if (k == 0 && inertia != nullptr) {
      double s = 0.0;
      for (int c = 0; c < chunks; ++c) s += pin[c];
      *inertia = s;
    }
  }
}

// chunk sums of d2 alone (the inertia of ava_km_assign): a thread per chunk
__global__ __launch_bounds__(64) void km_chunk_total_kernel(const double* __restrict__ v, int n, int chunks,
                                                            double* __restrict__ tot) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= chunks) return;
  const int64_t r0 = (int64_t)c * KM_CHUNK;
  const int64_t re = r0 + KM_CHUNK < n ? r0 + KM_CHUNK : n;
  double s = 0.0;
  for (int64_t r = r0; r < re; ++r) s += v[r];
  tot[c] = s;
}

__global__ void km_total_kernel(const double* __restrict__ tot, int chunks, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += tot[c];
  *out = s;
}

__device__ __forceinline__ double km_x(const void* X, int dtype, size_t i) {
  return dtype == 0 ? (double)static_cast<const float*>(X)[i] : static_cast<const double*>(X)[i];
}

// The end of iteration it, one workgroup of 256 threads.  csum / cnt hold the sums of the labels of this iteration.
__global__ __launch_bounds__(256) void km_finish_kernel(const void* __restrict__ X, int dtype, int n, int d, int K,
                                                        const int* __restrict__ labels, const double* __restrict__ d2,
                                                        double* __restrict__ csum, int* __restrict__ cnt,
                                                        const int* __restrict__ tchg, int tiles,
                                                        double* __restrict__ C, double tol,
                                                        const double* __restrict__ mean_var, double* __restrict__ shift_out,
                                                        int* __restrict__ ctl, int it) {
  const int t = threadIdx.x;
  if (km_stopped(ctl, it)) {
    if (t == 0) ctl[2 + it + 1] = 1;                           // the loop stays stopped
    return;
  }
  __shared__ int empty[KM_MAX_K];
  __shared__ int n_empty;
  __shared__ double rv[256];
  __shared__ int64_t ri[256];
  __shared__ int red[256];
  __shared__ double sk[KM_MAX_K];
  if (t == 0) {
    int m = 0;
    for (int k = 0; k < K; ++k)
      if (cnt[k] == 0) empty[m++] = k;
    n_empty = m;
  }
  __syncthreads();
  // relocation: pick e is the row after pick e - 1 in the order (d2 descending, row ascending)
  double pv = INFINITY;
  int64_t pi = -1;
  for (int e = 0; e < n_empty; ++e) {
    double bv = -1.0;
    int64_t bidx = -1;
    for (int64_t r = t; r < n; r += 256) {
      const double v = d2[r];
      const bool after = v < pv || (v == pv && r > pi);
      if (after && (v > bv || bidx < 0)) bv = v, bidx = r;     // ascending r: the first of equal values stays
    }
    rv[t] = bv, ri[t] = bidx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) {
        const double ov = rv[t + o];
        const int64_t oi = ri[t + o];
        if (oi >= 0 && (ri[t] < 0 || ov > rv[t] || (ov == rv[t] && oi < ri[t]))) rv[t] = ov, ri[t] = oi;
      }
      __syncthreads();
    }
    pv = rv[0], pi = ri[0];
    __syncthreads();                                           // rv / ri are read before the next pick writes them
    if (pi < 0) break;                                         // fewer rows than empty clusters: K <= n rules it out
    const int to = empty[e], from = labels[pi];
    if (t < d) {
      const double x = km_x(X, dtype, (size_t)pi * d + t);
      if (from >= 0 && from < K) csum[(size_t)from * d + t] -= x;
      csum[(size_t)to * d + t] = x;
    }
    if (t == 0) {
      cnt[to] = 1;
      if (from >= 0 && from < K) cnt[from] -= 1;
    }
    __syncthreads();
  }
  // means, in place of the sums
  for (int i = t; i < K * d; i += 256) {
    const int c = cnt[i / d];
    if (c > 0) csum[i] = csum[i] / (double)c;
  }
  __syncthreads();
  if (t < K) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) {
      const double v = csum[(size_t)t * d + j];
      const double df = v - C[(size_t)t * d + j];
      s = fma(df, df, s);
      C[(size_t)t * d + j] = v;
    }
    sk[t] = s;
  }
  int ch = 0;
  for (int i = t; i < tiles; i += 256) ch += tchg[i];
  red[t] = ch;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];                           // integers: no order to keep
    __syncthreads();
  }
  if (t == 0) {
    double shift = 0.0;
    for (int k = 0; k < K; ++k) shift += sk[k];
    if (shift_out != nullptr) *shift_out = shift;
    const bool strict = red[0] == 0;
    ctl[1] = it + 1;
    if (strict) ctl[0] = 1;
    ctl[2 + it + 1] = (strict || shift <= tol * mean_var[0]) ? 1 : 0;
  }
}

// centres = sums / counts (an empty cluster: zeros) and the counts as int64: ava_km_update
__global__ void km_means_kernel(const double* __restrict__ csum, const int* __restrict__ cnt, int d, int K,
                                double* __restrict__ C, int64_t* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K * d) return;
  const int c = cnt[i / d];
  C[i] = c > 0 ? csum[i] / (double)c : 0.0;
  if (i % d == 0) counts[i / d] = c;
}

// ---- k-means++ ---------------------------------------------------------------------------------------------------------
// closest[r] = d2(x_r, x_c), or its minimum with the closest before; c = *cptr if given, else cidx
template <typename T>
__global__ __launch_bounds__(256) void km_pp_apply_kernel(const T* __restrict__ X, int n, int d,
                                                          const int* __restrict__ cptr, int cidx, int init,
                                                          double* __restrict__ closest) {
  __shared__ double cr[KM_MAX_D];
  const int t = threadIdx.x;
  int c = cptr != nullptr ? *cptr : cidx;
  c = c < 0 ? 0 : (c >= n ? n - 1 : c);
  if (t < d) cr[t] = (double)X[(size_t)c * d + t];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + t;
  if (r >= n) return;
  double s = 0.0;
  for (int k = 0; k < d; ++k) {
    const double df = (double)X[(size_t)r * d + k] - cr[k];
    s = fma(df, df, s);
  }
  closest[r] = init ? s : fmin(closest[r], s);
}

// one workgroup: the chunk offsets, then thread l < L finds candidate l = searchsorted(scan, rand[l] * potential)
__global__ __launch_bounds__(64) void km_pp_pick_kernel(const double* __restrict__ closest, int n, int chunks,
                                                        const double* __restrict__ ctot, double* __restrict__ coff,
                                                        const double* __restrict__ rand, int L, int* __restrict__ cand) {
  const int t = threadIdx.x;
  if (t == 0) {
    double s = 0.0;
    coff[0] = 0.0;
    for (int c = 0; c < chunks; ++c) s += ctot[c], coff[c + 1] = s;
  }
  __syncthreads();
  if (t >= L) return;
  const double v = rand[t] * coff[chunks];
  int lo = 0, hi = chunks;                                     // the first chunk whose last scan entry is >= v
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (coff[mid + 1] < v) lo = mid + 1; else hi = mid;
  }
  if (lo >= chunks) {                                          // v is past the scan: the clip to N - 1
    cand[t] = n - 1;
    return;
  }
  const int64_t r0 = (int64_t)lo * KM_CHUNK;
  const int64_t re = r0 + KM_CHUNK < n ? r0 + KM_CHUNK : n;
  const double off = coff[lo];
  double local = 0.0;
  int64_t r = r0;
  for (; r < re - 1; ++r) {
    local += closest[r];
    if (off + local >= v) break;
  }
  cand[t] = (int)r;
}

// per chunk: min(closest, d2(candidate l, .)) of its rows and their ascending sum per candidate
template <typename T>
__global__ __launch_bounds__(256) void km_pp_update_kernel(const T* __restrict__ X, int n, int d, int L,
                                                           const int* __restrict__ cand,
                                                           const double* __restrict__ closest,
                                                           double* __restrict__ ppart) {
  __shared__ double cr[KM_MAX_TRIALS * KM_MAX_D];
  __shared__ double m[KM_MAX_TRIALS * 256];
  const int t = threadIdx.x, chunk = blockIdx.x;
  for (int i = t; i < KM_MAX_TRIALS * d; i += 256) {
    const int l = i / d, k = i % d;
    int c = l < L ? cand[l] : 0;
    c = c < 0 ? 0 : (c >= n ? n - 1 : c);
    cr[l * KM_MAX_D + k] = (double)X[(size_t)c * d + k];
  }
  const int64_t r0 = (int64_t)chunk * KM_CHUNK;
  const int rows = (int)((int64_t)n - r0 < KM_CHUNK ? (int64_t)n - r0 : KM_CHUNK);
  double part = 0.0;
  for (int s0 = 0; s0 < rows; s0 += 256) {
    __syncthreads();                                           // m of the stage before is consumed (and cr written)
    double sl[KM_MAX_TRIALS];
#pragma unroll
    for (int l = 0; l < KM_MAX_TRIALS; ++l) sl[l] = 0.0;
    double cl = 0.0;
    if (s0 + t < rows) {
      const size_t r = (size_t)(r0 + s0 + t);
      cl = closest[r];
      for (int k = 0; k < d; ++k) {
        const double x = (double)X[r * d + k];
#pragma unroll
        for (int l = 0; l < KM_MAX_TRIALS; ++l)
          if (l < L) {
            const double df = x - cr[l * KM_MAX_D + k];
            sl[l] = fma(df, df, sl[l]);
          }
      }
    }
#pragma unroll
    for (int l = 0; l < KM_MAX_TRIALS; ++l) m[l * 256 + t] = s0 + t < rows ? fmin(cl, sl[l]) : 0.0;
    __syncthreads();
    if (t < L) {
      const int ns = rows - s0 < 256 ? rows - s0 : 256;
      for (int i = 0; i < ns; ++i) part += m[t * 256 + i];
    }
  }
  if (t < L) ppart[(size_t)chunk * KM_MAX_TRIALS + t] = part;
}

// one workgroup: the L potentials in chunk order, the candidate of least potential (the first on a tie)
__global__ __launch_bounds__(64) void km_pp_commit_kernel(const double* __restrict__ ppart, int chunks, int L,
                                                          const int* __restrict__ cand, int* __restrict__ out_idx,
                                                          double* __restrict__ out_pot) {
  __shared__ double pots[KM_MAX_TRIALS];
  const int t = threadIdx.x;
  if (t < L) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += ppart[(size_t)c * KM_MAX_TRIALS + t];
    pots[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    int b = 0;
    for (int l = 1; l < L; ++l)
      if (pots[l] < pots[b]) b = l;
    *out_idx = cand[b];
    *out_pot = pots[b];
  }
}

// ---- column variances --------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(128) void km_var_part_kernel(const T* __restrict__ X, int n, int d,
                                                          const double* __restrict__ mean, double* __restrict__ vpart) {
  const int j = threadIdx.x, chunk = blockIdx.x;
  if (j >= d) return;
  const int64_t r0 = (int64_t)chunk * KM_CHUNK;
  const int64_t re = r0 + KM_CHUNK < n ? r0 + KM_CHUNK : n;
  double s = 0.0;
  if (mean == nullptr) {
    for (int64_t r = r0; r < re; ++r) s += (double)X[(size_t)r * d + j];
  } else {
    const double mj = mean[j];
    for (int64_t r = r0; r < re; ++r) {
      const double df = (double)X[(size_t)r * d + j] - mj;
      s = fma(df, df, s);
    }
  }
  vpart[(size_t)chunk * d + j] = s;
}

// pass 0: vmean = column sums / n; pass 1: out[1 + j] = sums / n, out[0] = their ascending sum / d
__global__ __launch_bounds__(128) void km_var_fin_kernel(const double* __restrict__ vpart, int chunks, int d, int n, int pass,
                                                         double* __restrict__ vmean, double* __restrict__ out) {
  __shared__ double v[KM_MAX_D];
  const int j = threadIdx.x;
  if (j < d) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += vpart[(size_t)c * d + j];
    s /= (double)n;
    if (pass == 0) vmean[j] = s; else v[j] = out[1 + j] = s;
  }
  if (pass == 0) return;
  __syncthreads();
  if (j == 0) {
    double s = 0.0;
    for (int i = 0; i < d; ++i) s += v[i];
    out[0] = s / (double)d;
  }
}

// ---- distances to the centres ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void km_transform_kernel(const T* __restrict__ X, int n, int d, int K,
                                                           const double* __restrict__ C, double* __restrict__ out) {
  __shared__ double xs[SQD_T * SQD_LD], ys[SQD_T * SQD_LD];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int q0 = blockIdx.x * SQD_T, c0 = blockIdx.y * SQD_T;
  double acc[4][4];
  sqd_tile(xs, ys, X, q0, n, C, c0, K, d, t, acc);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int lr = ty + 16 * i, c = c0 + tx + 16 * j;
      if (q0 + lr < n && c < K) out[((size_t)q0 + lr) * K + c] = sqrt(acc[i][j]);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
template <typename T>
static int km_launch_assign(const T* X, int n, int d, int K, const double* C, int* labels, double* d2, int* tchg,
                            const int* ctl, int it, hipStream_t st) {
  hipLaunchKernelGGL(km_assign_kernel<T>, dim3(km_tiles(n)), dim3(256), 0, st, X, n, d, K, C, labels, d2, tchg, ctl, it);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename T>
static int km_launch_sums(const T* X, int n, int d, int K, const int* labels, const double* d2, const km_ws& w,
                          double* inertia, const int* ctl, int it, hipStream_t st) {
  const int chunks = km_chunks(n);
  const dim3 grid(chunks, ceil_div(d, KM_SLAB));
#define KM_SUMS(NS_)                                                                                              \
  hipLaunchKernelGGL((km_sums_kernel<T, NS_>), grid, dim3(256), 0, st, X, n, d, K, labels, d2, w.psum, w.pcnt, w.pin, ctl, it)
  switch (K <= KM_REG_K ? ceil_div(K, KM_GROUPS) : 0) {        // the accumulators a thread needs; no result depends on it
    case 1: KM_SUMS(1); break;
    case 2: KM_SUMS(2); break;
    case 3: case 4: KM_SUMS(4); break;
    default:
      hipLaunchKernelGGL(km_sums_lds_kernel<T>, grid, dim3(256), 0, st, X, n, d, K, labels, d2, w.psum, w.pcnt, w.pin, ctl,
                         it);
      break;
  }
#undef KM_SUMS
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_reduce_kernel, dim3(K), dim3(128), 0, st, w.psum, w.pcnt, w.pin, chunks, d, K, w.csum, w.cnt,
                     inertia, ctl, it);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename T>
static int km_fit(const T* X, int dtype, int n, int d, int K, double* C, int* labels, double* d2, double tol,
                  const double* mean_var, int it0, int n_iters, int* ctl, double* shift, const km_ws& w, hipStream_t st) {
  for (int it = it0; it < it0 + n_iters; ++it) {
    int rc = km_launch_assign(X, n, d, K, C, labels, d2, w.tchg, ctl, it, st);
    if (rc != AVA_OK) return rc;
    rc = km_launch_sums(X, n, d, K, labels, d2, w, nullptr, ctl, it, st);
    if (rc != AVA_OK) return rc;
    hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(256), 0, st, static_cast<const void*>(X), dtype, n, d, K, labels,
                       d2, w.csum, w.cnt, w.tchg, km_tiles(n), C, tol, mean_var, shift, ctl, it);
    AVA_CHECK_LAUNCH();
  }
  return AVA_OK;
}

template <typename T>
static int km_pp_step(const T* X, int n, int d, int L, const double* rand, double* closest, int* out_idx, double* out_pot,
                      const km_ws& w, hipStream_t st) {
  const int chunks = km_chunks(n);
  hipLaunchKernelGGL(km_chunk_total_kernel, dim3(ceil_div(chunks, 64)), dim3(64), 0, st, closest, n, chunks, w.ctot);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_pp_pick_kernel, dim3(1), dim3(64), 0, st, closest, n, chunks, w.ctot, w.coff, rand, L, w.cand);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_pp_update_kernel<T>, dim3(chunks), dim3(256), 0, st, X, n, d, L, w.cand, closest, w.ppart);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_pp_commit_kernel, dim3(1), dim3(64), 0, st, w.ppart, chunks, L, w.cand, out_idx, out_pot);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_pp_apply_kernel<T>, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, X, n, d, out_idx, 0, 0,
                     closest);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename T>
static int km_variance(const T* X, int n, int d, double* out, const km_ws& w, hipStream_t st) {
  const int chunks = km_chunks(n);
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(km_var_part_kernel<T>, dim3(chunks), dim3(128), 0, st, X, n, d,
                       pass == 0 ? static_cast<const double*>(nullptr) : w.vmean, w.vpart);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_var_fin_kernel, dim3(1), dim3(128), 0, st, w.vpart, chunks, d, n, pass, w.vmean, out);
    AVA_CHECK_LAUNCH();
  }
  return AVA_OK;
}

#define KM_DISPATCH(FN, ...)                                                    \
  (dtype == 0 ? FN(static_cast<const float*>(x), __VA_ARGS__) : FN(static_cast<const double*>(x), __VA_ARGS__))

extern "C" int ava_km_max_d(void) { return KM_MAX_D; }
extern "C" int ava_km_max_k(void) { return KM_MAX_K; }
extern "C" int ava_km_chunk_rows(void) { return KM_CHUNK; }

extern "C" size_t ava_km_workspace_bytes(int n, int d, int k) {
  if (!km_shape_ok(n, d, k)) return 0;
  km_ws w;
  return km_ws_layout(n, d, k, nullptr, &w);
}

extern "C" int ava_km_assign(const void* x, int dtype, int n, int d, int k, const double* centres, int* labels, double* d2,
                             double* inertia, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !km_shape_ok(n, d, k) || !centres || !labels || !d2 || !ws) return AVA_EINVAL;
  if (ws_bytes < ava_km_workspace_bytes(n, d, k)) return AVA_EWORKSPACE;
  km_ws w;
  km_ws_layout(n, d, k, ws, &w);
  hipStream_t st = to_stream(s);
  const int rc = KM_DISPATCH(km_launch_assign, n, d, k, centres, labels, d2, nullptr, nullptr, 0, st);
  if (rc != AVA_OK || !inertia) return rc;
  const int chunks = km_chunks(n);
  hipLaunchKernelGGL(km_chunk_total_kernel, dim3(ceil_div(chunks, 64)), dim3(64), 0, st, d2, n, chunks, w.pin);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_total_kernel, dim3(1), dim3(64), 0, st, w.pin, chunks, inertia);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_km_update(const void* x, int dtype, int n, int d, int k, const int* labels, double* centres,
                             int64_t* counts, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !km_shape_ok(n, d, k) || !labels || !centres || !counts || !ws)
    return AVA_EINVAL;
  if (ws_bytes < ava_km_workspace_bytes(n, d, k)) return AVA_EWORKSPACE;
  km_ws w;
  km_ws_layout(n, d, k, ws, &w);
  hipStream_t st = to_stream(s);
  const int rc = KM_DISPATCH(km_launch_sums, n, d, k, labels, nullptr, w, nullptr, nullptr, 0, st);
  if (rc != AVA_OK) return rc;
  hipLaunchKernelGGL(km_means_kernel, dim3(ceil_div(k * d, 256)), dim3(256), 0, st, w.csum, w.cnt, d, k, centres, counts);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_km_fit(const void* x, int dtype, int n, int d, int k, double* centres, int* labels, double* d2,
                          double tol, const double* mean_var, int it0, int n_iters, int* ctl, double* shift, void* ws,
                          size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !km_shape_ok(n, d, k) || k > n || !centres || !labels || !d2 || !(tol >= 0.0) ||
      !mean_var || it0 < 0 || n_iters < 1 || n_iters > (1 << 20) || it0 > (1 << 20) || !ctl || !ws)
    return AVA_EINVAL;
  if (ws_bytes < ava_km_workspace_bytes(n, d, k)) return AVA_EWORKSPACE;
  km_ws w;
  km_ws_layout(n, d, k, ws, &w);
  return KM_DISPATCH(km_fit, dtype, n, d, k, centres, labels, d2, tol, mean_var, it0, n_iters, ctl, shift, w, to_stream(s));
}

extern "C" int ava_km_pp_start(const void* x, int dtype, int n, int d, int first, double* closest, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !km_rows_ok(n, d) || first < 0 || first >= n || !closest) return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  const dim3 grid((unsigned)ceil_div64(n, 256));
  if (dtype == 0)
    hipLaunchKernelGGL(km_pp_apply_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), n, d,
                       static_cast<const int*>(nullptr), first, 1, closest);
  else
    hipLaunchKernelGGL(km_pp_apply_kernel<double>, grid, dim3(256), 0, st, static_cast<const double*>(x), n, d,
                       static_cast<const int*>(nullptr), first, 1, closest);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_km_pp_step(const void* x, int dtype, int n, int d, int n_trials, const double* rand, double* closest,
                              int* out_idx, double* out_pot, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !km_rows_ok(n, d) || n_trials < 1 || n_trials > KM_MAX_TRIALS || !rand ||
      !closest || !out_idx || !out_pot || !ws)
    return AVA_EINVAL;
  if (ws_bytes < ava_km_workspace_bytes(n, d, 1)) return AVA_EWORKSPACE;
  km_ws w;
  km_ws_layout(n, d, 1, ws, &w);
  return KM_DISPATCH(km_pp_step, n, d, n_trials, rand, closest, out_idx, out_pot, w, to_stream(s));
}

extern "C" int ava_km_variance(const void* x, int dtype, int n, int d, double* out, void* ws, size_t ws_bytes,
                               ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !km_rows_ok(n, d) || !out || !ws) return AVA_EINVAL;
  if (ws_bytes < ava_km_workspace_bytes(n, d, 1)) return AVA_EWORKSPACE;
  km_ws w;
  km_ws_layout(n, d, 1, ws, &w);
  return KM_DISPATCH(km_variance, n, d, out, w, to_stream(s));
}

extern "C" int ava_km_transform(const void* x, int dtype, int n, int d, int k, const double* centres, double* out,
                                ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !km_rows_ok(n, d) || k < 1 || k > KM_MAX_K || !centres || !out)
    return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  const dim3 grid(km_tiles(n), ceil_div(k, SQD_T));
  if (dtype == 0)
    hipLaunchKernelGGL(km_transform_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), n, d, k, centres,
                       out);
  else
    hipLaunchKernelGGL(km_transform_kernel<double>, grid, dim3(256), 0, st, static_cast<const double*>(x), n, d, k,
                       centres, out);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
