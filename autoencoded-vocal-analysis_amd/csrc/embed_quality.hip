// Trustworthiness, continuity and preserved neighbours of an embedding (the specification
// of the first is scikit-learn 1.7's manifold/_t_sne.py::trustworthiness, the definitions are in
// include/ava_embed_quality.h).  Every result is an integer: a count of pairs under the strict (distance, index) order
// pj_before of knn_list.h, or a sum of such counts.  Integer sums are exact in any order, so no result depends on the
// launch shape; no kernel uses a floating-point atomic.
//
// rank      rank[i][s] = 1 + #{ l != i : (d2(i, l), l) before (d2(i, tgt[i][s]), tgt[i][s]) }.  One workgroup owns 64
//           query rows and a range of reference tiles.  It forms the target distances with the scalar loop of the order
//           contract of sqdist_tile.h (the bits of pair_sqdist_kernel), so a target compares equal to its own tile entry
//           and counts under nothing, and duplicated rows tie exactly.  It sorts every row's targets by the order and
//           sweeps its reference tiles with sqd_tile: a pair at or beyond the row's last sorted target is rejected by one
//           compare, every other pair finds the first sorted target it comes before by bisection and bumps one
//           counter there.  The pairs before sorted target p are the prefix sum of the counters up to p.
// penalty   pen[i][a] = sum over s < ks[a] of max(0, rank[i][s] - ks[a]), int64.
// overlap   ov[i][a] = #{ (s, t) : A[i][s] == B[i][t], max(s, t) < ks[a] }: one wavefront per row, a histogram over
//           max(s, t) and a prefix sum.
// total     the column sums of either table, one workgroup per column, int64.
#include <limits.h>

#include "common.h"
#include "knn_list.h"
#include "sqdist_tile.h"

#define EQ_MAX_M (PJ_MAX_K - 1)      // targets per row: a kNN list without its self column
#define EQ_MAX_SWEEP 16
#define EQ_MAX_DIM 65536             // projection.MAX_DIM
#define EQ_FILL_WGS 512              // workgroups col_splits = 0 aims at: two for each of the 256 CUs

struct eq_sweep {
  int n_k;
  int k[EQ_MAX_SWEEP];
};

// flag[0] |= 1 when a target lies outside [0, n) or equals its row
__global__ __launch_bounds__(256) void eq_check_kernel(const int64_t* __restrict__ tgt, int n, int m,
                                                       int* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * m) return;
  const int64_t j = tgt[e];
  if (j < 0 || j >= n || j == e / m) atomicOr(flag, 1);
}

// rank [n][m] += this workgroup's counts (the workgroups of split 0 add the 1 of the definition): the table is zeroed
// before the launch.  Grid (query tiles, col_splits); workgroup (x, y) sweeps the reference tiles
// [y rt / col_splits, (y + 1) rt / col_splits) of the rt = ceil(n / 64) tiles.
// LDS: 33 792 B static for the staging buffers and 64 m 17 B dynamic: the sorted target distances (double), their
// indices (int), the counters (int) and every slot's sorted position (a byte); 102 336 B at m = 63, of the 160 KiB a
// workgroup may use.
template <typename T>
__global__ __launch_bounds__(256) void eq_rank_kernel(const T* __restrict__ X, const int64_t* __restrict__ tgt, int n,
                                                      int d, int m, int* __restrict__ rank) {
  __shared__ double stage[2 * SQD_T * SQD_LD];      // xs | ys of sqd_tile; before the sweep the sort's copy buffer
  extern __shared__ double eq_lds[];
  const int tm = SQD_T * m;
  double* sd = eq_lds;                                          // [64][m] target distances, sorted per row
  int* si = reinterpret_cast<int*>(sd + tm);                    // [64][m] their indices
  int* hist = si + tm;                                          // [64][m] pairs whose first later target is this one
  unsigned char* spos = reinterpret_cast<unsigned char*>(hist + tm);   // [64][m] sorted position of slot s
  double* xs = stage;
  double* ys = stage + SQD_T * SQD_LD;
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int qb = blockIdx.x * SQD_T;

  // the target distances in slot order: one fma per feature, features ascending (the order contract)
  for (int e = t; e < tm; e += 256) {
    const int q = qb + e / m;
    double s = 0.0;
    int j = 0;
    if (q < n) {
      j = (int)tgt[(size_t)q * m + e % m];
      const T* x = X + (size_t)q * d;
      const T* y = X + (size_t)j * d;
      for (int k = 0; k < d; ++k) {
        const double df = (double)x[k] - (double)y[k];
        s = fma(df, df, s);
      }
    }
    sd[e] = s;
    si[e] = j;
    hist[e] = 0;
  }
  __syncthreads();
  // every slot's position in its row's order; equal targets (a repeated index) keep their slot order
  for (int e = t; e < tm; e += 256) {
    const int r0 = (e / m) * m, s = e - r0;
    const double ds = sd[e];
    const int is = si[e];
    int p = 0;
    for (int u = 0; u < m; ++u) {
      const double du = sd[r0 + u];
      const int iu = si[r0 + u];
      p += (du < ds || (du == ds && (iu < is || (iu == is && u < s)))) ? 1 : 0;
    }
    spos[e] = (unsigned char)p;
  }
  __syncthreads();
  // the permutation, through the staging buffer: distances, then indices
  for (int e = t; e < tm; e += 256) stage[e] = sd[e];
  __syncthreads();
  for (int e = t; e < tm; e += 256) sd[(e / m) * m + spos[e]] = stage[e];
  __syncthreads();
  int* stage_i = reinterpret_cast<int*>(stage);
  for (int e = t; e < tm; e += 256) stage_i[e] = si[e];
  __syncthreads();
  for (int e = t; e < tm; e += 256) si[(e / m) * m + spos[e]] = stage_i[e];
  __syncthreads();                                   // sqd_tile opens with a barrier of its own before it writes stage

  // the row's last sorted target: a pair that is not before it counts under no target.  A row that does not exist
  // gets a bound nothing is before.
  double wd[4];
  int wi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty + 16 * i;
    const bool live = qb + r < n;
    wd[i] = live ? sd[r * m + m - 1] : -1.0;
    wi[i] = live ? si[r * m + m - 1] : 0;
  }

  int top = 1;                                       // the largest power of two <= m
  while (2 * top <= m) top *= 2;
  const int rt = (n + SQD_T - 1) / SQD_T;
  const int t0 = (int)((int64_t)blockIdx.y * rt / gridDim.y), t1 = (int)((int64_t)(blockIdx.y + 1) * rt / gridDim.y);
  for (int tile = t0; tile < t1; ++tile) {
    const int r0 = tile * SQD_T;
    double acc[4][4];
    sqd_tile(xs, ys, X, qb, n, X, r0, n, d, t, acc);
    // which of the thread's 16 pairs lie before their row's last sorted target
    unsigned pass = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = ty + 16 * i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int l = r0 + tx + 16 * j;
        const double dd = acc[i][j];
        if (l < n && l != qb + r && (dd < wd[i] || (dd == wd[i] && l < wi[i]))) pass |= 1u << (4 * i + j);
      }
    }
    if (pass != 0) {
      // pos = the number of sorted targets that are not after the pair, for all 16 pairs at once and without branches, so
      // that their LDS reads overlap: a bisection by descending powers of two (top: the largest one <= m)
      int pos[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) pos[i][j] = 0;
      for (int step = top; step > 0; step >>= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = ty + 16 * i;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = pos[i][j] + step;
            const int e = r * m + (c <= m ? c : m) - 1;
            const bool before = pj_before(acc[i][j], r0 + tx + 16 * j, sd[e], si[e]);
            pos[i][j] = (c <= m && !before) ? c : pos[i][j];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((pass >> (4 * i + j)) & 1) atomicAdd(&hist[(ty + 16 * i) * m + pos[i][j]], 1);
    }
  }
  __syncthreads();
  const int one = blockIdx.y == 0 ? 1 : 0;
  for (int e = t; e < tm; e += 256) {
    const int r = e / m, q = qb + r;
    if (q >= n) break;                               // e ascends with r
    const int p = spos[e];
    int c = one;
    for (int u = 0; u <= p; ++u) c += hist[r * m + u];
    atomicAdd(&rank[(size_t)q * m + (e - r * m)], c);
  }
}

// pen [n][n_k]: one thread per row
__global__ __launch_bounds__(256) void eq_penalty_kernel(const int* __restrict__ rank, int n, int m, eq_sweep sw,
                                                         int64_t* __restrict__ pen) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const int* r = rank + (size_t)row * m;
  for (int a = 0; a < sw.n_k; ++a) {
    const int k = sw.k[a];
    int64_t p = 0;
    for (int s = 0; s < k; ++s) {
      const int64_t over = (int64_t)r[s] - k;
      p += over > 0 ? over : 0;
    }
    pen[(size_t)row * sw.n_k + a] = p;
  }
}

// ov [n][n_k]: wavefront w of a workgroup owns row 4 blockIdx.x + w; lane s holds slot s of both lists.  An entry
// below 0 matches nothing.
__global__ __launch_bounds__(256) void eq_overlap_kernel(const int64_t* __restrict__ A, const int64_t* __restrict__ B,
                                                         int n, int m, eq_sweep sw, int* __restrict__ ov) {
  __shared__ int hist[4][AVA_WAVE];                  // matches by max(s, t)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  const bool live = row < n && lane < m;
  const int64_t a = live ? A[(size_t)row * m + lane] : -1;
  const int64_t bv = live ? B[(size_t)row * m + lane] : -1;
  hist[w][lane] = 0;
  __syncthreads();
  for (int s = 0; s < m; ++s) {
    const int64_t b = __shfl(bv, s, 64);             // by every lane
    if (a >= 0 && a == b) atomicAdd(&hist[w][lane > s ? lane : s], 1);
  }
  __syncthreads();
  if (row < n && lane < sw.n_k) {
    int c = 0;
    for (int u = 0; u < sw.k[lane]; ++u) c += hist[w][u];
    ov[(size_t)row * sw.n_k + lane] = c;
  }
}

// tot [c] = the sum over the rows of column blockIdx.x of the table [n][c]
template <typename T>
__global__ __launch_bounds__(256) void eq_total_kernel(const T* __restrict__ table, int n, int c,
                                                       int64_t* __restrict__ tot) {
  __shared__ int64_t part[256];
  const int t = threadIdx.x;
  int64_t s = 0;
  for (int64_t r = t; r < n; r += 256) s += (int64_t)table[(size_t)r * c + blockIdx.x];
  part[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) part[t] += part[t + o];
    __syncthreads();
  }
  if (t == 0) tot[blockIdx.x] = part[0];
}

extern "C" int ava_eq_max_targets(void) { return EQ_MAX_M; }
extern "C" int ava_eq_max_sweep(void) { return EQ_MAX_SWEEP; }

static bool eq_shape_ok(int n, int m) { return n >= 2 && n <= INT_MAX - SQD_T && m >= 1 && m <= EQ_MAX_M; }

extern "C" size_t ava_eq_workspace_bytes(int n, int m) {
  if (!eq_shape_ok(n, m)) return 0;
  ava_ws_cursor c(nullptr);
  c.take<int>(1);                                    // the target check's flag
  return c.bytes();
}

// false unless 1 <= ks[a] <= m for every a < n_k <= EQ_MAX_SWEEP
static bool eq_sweep_of(const int* ks, int n_k, int m, eq_sweep* sw) {
  if (ks == nullptr || n_k < 1 || n_k > EQ_MAX_SWEEP) return false;
  sw->n_k = n_k;
  for (int a = 0; a < EQ_MAX_SWEEP; ++a) {
    sw->k[a] = a < n_k ? ks[a] : 0;
    if (a < n_k && (ks[a] < 1 || ks[a] > m)) return false;
  }
  return true;
}

extern "C" int ava_eq_ranks(const void* x, int dtype, int n, int d, const int64_t* tgt, int m, int col_splits,
                            int* rank, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (x == nullptr || tgt == nullptr || rank == nullptr || ws == nullptr || (dtype != 0 && dtype != 1) ||
      !eq_shape_ok(n, m) || d < 1 || d > EQ_MAX_DIM || col_splits < 0)
    return AVA_EINVAL;
  if (ws_bytes < ava_eq_workspace_bytes(n, m)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  ava_ws_cursor c(ws);
  int* flag = c.take<int>(1);
  // the targets are read as row numbers: they are checked, on the device, before anything follows them
  if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) return AVA_ELAUNCH;
  hipLaunchKernelGGL(eq_check_kernel, dim3((unsigned)ceil_div64((int64_t)n * m, 256)), dim3(256), 0, st, tgt, n, m, flag);
  AVA_CHECK_LAUNCH();
  int bad = 0;
  if (hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return AVA_ELAUNCH;
  if (bad != 0) return AVA_EINVAL;

  const int tiles = ceil_div(n, SQD_T);
  int splits = col_splits > 0 ? col_splits : ceil_div(EQ_FILL_WGS, tiles);
  if (splits > tiles) splits = tiles;
  if (splits > 65535) splits = 65535;
  if (hipMemsetAsync(rank, 0, (size_t)n * m * sizeof(int), st) != hipSuccess) return AVA_ELAUNCH;
  const size_t lds = (size_t)SQD_T * m * (sizeof(double) + 2 * sizeof(int) + 1);
  if (dtype == 0)
    hipLaunchKernelGGL(eq_rank_kernel<float>, dim3(tiles, splits), dim3(256), lds, st,
                       reinterpret_cast<const float*>(x), tgt, n, d, m, rank);
  else
    hipLaunchKernelGGL(eq_rank_kernel<double>, dim3(tiles, splits), dim3(256), lds, st,
                       reinterpret_cast<const double*>(x), tgt, n, d, m, rank);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_eq_penalties(const int* rank, int n, int m, const int* ks, int n_k, int64_t* pen, int64_t* totals,
                                ava_stream_t s) {
  eq_sweep sw;
  if (rank == nullptr || pen == nullptr || totals == nullptr || n < 1 || m < 1 || m > EQ_MAX_M ||
      !eq_sweep_of(ks, n_k, m, &sw))
    return AVA_EINVAL;
  hipLaunchKernelGGL(eq_penalty_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, to_stream(s), rank, n, m, sw, pen);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(eq_total_kernel<int64_t>, dim3(n_k), dim3(256), 0, to_stream(s), pen, n, n_k, totals);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_eq_overlap(const int64_t* a, const int64_t* b, int n, int m, const int* ks, int n_k, int* overlap,
                              int64_t* totals, ava_stream_t s) {
  eq_sweep sw;
  if (a == nullptr || b == nullptr || overlap == nullptr || totals == nullptr || n < 1 || m < 1 || m > EQ_MAX_M ||
      !eq_sweep_of(ks, n_k, m, &sw))
    return AVA_EINVAL;
  hipLaunchKernelGGL(eq_overlap_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, to_stream(s), a, b, n, m, sw, overlap);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(eq_total_kernel<int>, dim3(n_k), dim3(256), 0, to_stream(s), overlap, n, n_k, totals);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
