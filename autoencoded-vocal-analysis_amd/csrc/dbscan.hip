// DBSCAN of latent rows: the device side of scikit-learn 1.7's sklearn/cluster/_dbscan.py
// and _dbscan_inner.pyx.  X is [N][d] float32 or float64 and is converted on load; everything else is fp64 or integer.
// The result is a function of the data alone: integer atomics only (adds, minima, compare-and-swap), whose outcome does
// not depend on their order, so the same inputs give the same labels on every run, whatever the grid or the interleaving.
//
// Every pass takes n_eps <= DB_MAX_EPS = 8 radii, forms each pair's distance once and compares it n_eps times; per-radius
// state is laid out [n_eps][N].  The three distance passes walk the 64 x 64 tiles on or above the diagonal, one workgroup
// per tile, tile p of the row-major list of the pairs (bi, bj), bi <= bj.  In a tile above the diagonal every pair has
// row < column and serves both rows; the diagonal tile is formed in full (both orders of a pair, and the row against
// itself) and serves its rows only, so no pair is counted twice and every row meets itself once.
//   db_count_kernel      counts[e][i] = #{j : within(i, j, e)}, the row itself included: per tile the row and column sums
//                        in LDS, then one global atomicAdd per row with a non-zero sum
//   db_union_kernel      parent[e][i] (initialised to i): for every pair i < j within eps whose rows are both core
//                        (counts >= min_samples), unite the two trees.  Lock-free: find the two roots by relaxed
//                        agent-scope atomic loads (the workgroups sit on different XCDs; a plain load may be served stale
//                        from L1), then atomicCAS the LARGER root, from itself, to the smaller.  Only roots are ever
//                        rewritten, parent[i] <= i always holds and only decreases, so there are no cycles, and a
//                        component's smallest row can never be hooked: it is the final root whatever the interleaving.
//                        A thread whose CAS fails finds the roots again and retries its own edge; nobody waits for
//                        anybody, and the end of the launch is the only barrier.
//   db_flatten_kernel    root[e][i] = find(i) for core rows, -1 for the others (a launch of its own)
//   db_border_kernel     cand[e][i] (initialised to INT_MAX) = min root[e][j] over the core rows j within eps of the
//                        non-core row i: minima per tile in LDS, then one global atomicMin.  It is the minimum ROOT, taken
//                        after the flatten: roots are numbered in ascending order below, so it is the smallest cluster
//                        number, which is what dbscan_inner's expansion in label order leaves.
//   db_flagsum_kernel, db_chunkscan_kernel, db_scan_kernel, db_relabel_kernel
//                        flag[i] = core && root[i] == i; its exclusive scan over constant chunks of DB_CHUNK = 2048 rows
//                        is the cluster number of root i (clusters in ascending order of their smallest row);
//                        labels = scan[root[i]] (core), scan[cand[i]] (border), -1 (noise); n_clusters[e] = the total
// A tile none of whose pairs can matter (no core row among its rows or its columns; for the border pass no non-core row
// facing a core row) returns before it forms a distance.
//
// Pair predicate.  Euclidean: d2 <= eps2, d2 the sum of sqdist_tile.h (direct differences, one fma per feature, features
// ascending, so d2(i, j) and d2(j, i) have the same bits), eps2 = eps * eps rounded once on the host in fp64; no square
// root.  Precomputed: (double)D[i][j] <= eps with i <= j the pair's smaller row; D must be symmetric (the caller checks).
#include <limits.h>
#include <math.h>

#include "common.h"
#include "sqdist_tile.h"

#define DB_MAX_EPS 8
#define DB_CHUNK 2048            // rows of a scan chunk: a constant, never derived from the grid
#define DB_MAX_N (1 << 21)       // 32768 row tiles: the tile list of the upper triangle stays below 2^31
#define DB_MAX_D 65536

struct db_thr {
  double v[DB_MAX_EPS];          // eps2 (euclidean) or eps (precomputed) per radius
};

// ---- the tile walk -------------------------------------------------------------------------------------------------------
// tile p of the row-major list of the pairs (bi, bj), bi <= bj < tiles: row bi starts at s(bi) = bi tiles - bi (bi - 1) / 2
__device__ __forceinline__ int64_t db_row_start(int64_t bi, int64_t tiles) { return bi * tiles - bi * (bi - 1) / 2; }

__device__ __forceinline__ void db_decode_tile(int64_t p, int tiles, int& bi, int& bj) {
  const double b = 2.0 * tiles + 1.0;
  int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  if (r < 0) r = 0;
  if (r > tiles - 1) r = tiles - 1;
  while (r + 1 < tiles && db_row_start(r + 1, tiles) <= p) ++r;    // the square root is a first guess only
  while (r > 0 && db_row_start(r, tiles) > p) --r;
  bi = (int)r;
  bj = (int)(r + (p - db_row_start(r, tiles)));
}

// The core bits of the tile's rows (side 0, from q0) and columns (side 1, from r0) into LDS: bit e of bits[side][l] is
// set when counts[e][row] >= min_samples, and any[side] is the OR over the side.  A row from n on has no bit set.  With
// BORDER it has all n_eps bits set instead (a row that does not exist is never a border row), and any[2 + side] is the
// OR of the complements over the rows that exist: the radii at which the side has a non-core row.  Every thread calls;
// opens with a barrier after zeroing `any` (which also publishes what the caller initialised) and ends with one.
template <bool BORDER>
__device__ __forceinline__ void db_stage_core_bits(const int* __restrict__ counts, int n, int n_eps, int min_samples,
                                                   int q0, int r0, int t, unsigned (*bits)[SQD_T], unsigned* any) {
  const unsigned all = (1u << n_eps) - 1u;
  if (t < (BORDER ? 4 : 2)) any[t] = 0;
  __syncthreads();
  if (t < 2 * SQD_T) {
    const int side = t >> 6, l = t & 63;
    const int row = (side ? r0 : q0) + l;
    unsigned m = 0;
    if (row < n)
      for (int e = 0; e < n_eps; ++e) m |= (counts[(size_t)e * n + row] >= min_samples ? 1u : 0u) << e;
    bits[side][l] = (BORDER && row >= n) ? all : m;
    if (m) atomicOr(&any[side], m);
    if (BORDER && row < n && (~m & all)) atomicOr(&any[2 + side], ~m & all);
  }
  __syncthreads();
}

// ---- 1. neighbour counts ------------------------------------------------------------------------------------------------
// grid tiles (tiles + 1) / 2, 256 threads; counts is zero before the launch
template <typename T, bool PRE>
__global__ __launch_bounds__(256) void db_count_kernel(const T* __restrict__ X, int n, int d, int tiles, db_thr thr,
                                                       int n_eps, int* __restrict__ counts) {
  __shared__ double xs[PRE ? 1 : SQD_T * SQD_LD];
  __shared__ double ys[PRE ? 1 : SQD_T * SQD_LD];
  __shared__ int rsum[DB_MAX_EPS][SQD_T];
  __shared__ int csum[DB_MAX_EPS][SQD_T];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  int bi, bj;
  db_decode_tile(blockIdx.x, tiles, bi, bj);
  const int q0 = bi * SQD_T, r0 = bj * SQD_T;
  const bool diag = bi == bj;
  for (int p = t; p < DB_MAX_EPS * SQD_T; p += 256) {
    (&rsum[0][0])[p] = 0;
    (&csum[0][0])[p] = 0;
  }
  double acc[4][4];
  sqd_pair_tile<T, PRE>(X, n, d, q0, r0, xs, ys, t, acc);            // its barriers also publish the zeros (d >= 1)
  if (PRE) __syncthreads();
  for (int e = 0; e < n_eps; ++e) {
    const double lim = thr.v[e];
    int rs[4] = {0, 0, 0, 0}, cs[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = q0 + ty + 16 * i < n && r0 + tx + 16 * j < n && acc[i][j] <= lim;
        rs[i] += in ? 1 : 0;
        cs[j] += in ? 1 : 0;
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (rs[i]) atomicAdd(&rsum[e][ty + 16 * i], rs[i]);
      if (!diag && cs[i]) atomicAdd(&csum[e][tx + 16 * i], cs[i]);
    }
  }
  __syncthreads();
  for (int p = t; p < n_eps * SQD_T; p += 256) {
    const int e = p >> 6, l = p & 63;
    const int a = rsum[e][l], b = csum[e][l];
    if (a && q0 + l < n) atomicAdd(&counts[(size_t)e * n + q0 + l], a);
    if (b && r0 + l < n) atomicAdd(&counts[(size_t)e * n + r0 + l], b);
  }
}

// ---- 3. union ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int db_find(int* parent, int x) {
  for (;;) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= x || p < 0) return x;                                   // p == x: a root (p > x or p < 0 cannot happen)
    x = p;
  }
}

// unite the trees of a and b; terminates: every failed CAS means another thread's hook succeeded on that root
__device__ __forceinline__ void db_unite(int* parent, int a, int b) {
  for (;;) {
    a = db_find(parent, a);
    b = db_find(parent, b);
    if (a == b) return;                                              // the root-equality check before any CAS
    if (a > b) {
      const int s = a;
      a = b;
      b = s;
    }
    if (atomicCAS(parent + b, b, a) == b) return;                    // hook the larger root under the smaller
  }
}

__global__ __launch_bounds__(256) void db_iota_kernel(int* __restrict__ parent, int n, int n_eps) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < (int64_t)n * n_eps) parent[p] = (int)(p % n);
}

template <typename T, bool PRE>
__global__ __launch_bounds__(256) void db_union_kernel(const T* __restrict__ X, int n, int d, int tiles, db_thr thr,
                                                       int n_eps, int min_samples, const int* __restrict__ counts,
                                                       int* parent) {
  __shared__ double xs[PRE ? 1 : SQD_T * SQD_LD];
  __shared__ double ys[PRE ? 1 : SQD_T * SQD_LD];
  __shared__ unsigned bits[2][SQD_T];                                // core bits of the tile's rows and columns
  __shared__ unsigned any[2];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  int bi, bj;
  db_decode_tile(blockIdx.x, tiles, bi, bj);
  const int q0 = bi * SQD_T, r0 = bj * SQD_T;
  const bool diag = bi == bj;
  db_stage_core_bits<false>(counts, n, n_eps, min_samples, q0, r0, t, bits, any);
  const unsigned live = any[0] & any[1];
  if (!live) return;                                                 // uniform: no radius has core rows on both sides
  double acc[4][4];
  sqd_pair_tile<T, PRE>(X, n, d, q0, r0, xs, ys, t, acc);
  unsigned rb[4], cb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rb[i] = bits[0][ty + 16 * i];                                    // 0 for rows from n on
    cb[i] = bits[1][tx + 16 * i];
  }
  for (int e = 0; e < n_eps; ++e) {
    if (!((live >> e) & 1u)) continue;
    const double lim = thr.v[e];
    int* par = parent + (size_t)e * n;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = q0 + ty + 16 * i, c = r0 + tx + 16 * j;
        if (((rb[i] & cb[j]) >> e) & 1u)
          if (acc[i][j] <= lim && (!diag || r < c)) db_unite(par, r, c);
      }
  }
}

// ---- 4. flatten ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void db_flatten_kernel(int* parent, const int* __restrict__ counts, int n, int n_eps,
                                                         int min_samples, int* __restrict__ root,
                                                         int* __restrict__ cand) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)n * n_eps) return;
  const int e = (int)(p / n), i = (int)(p - (int64_t)e * n);
  root[p] = counts[p] >= min_samples ? db_find(parent + (size_t)e * n, i) : -1;
  cand[p] = INT_MAX;
}

// ---- 5. border -----------------------------------------------------------------------------------------------------------
template <typename T, bool PRE>
__global__ __launch_bounds__(256) void db_border_kernel(const T* __restrict__ X, int n, int d, int tiles, db_thr thr,
                                                        int n_eps, int min_samples, const int* __restrict__ counts,
                                                        const int* __restrict__ root, int* __restrict__ cand) {
  __shared__ double xs[PRE ? 1 : SQD_T * SQD_LD];
  __shared__ double ys[PRE ? 1 : SQD_T * SQD_LD];
  __shared__ unsigned bits[2][SQD_T];
  __shared__ unsigned any[4];                                        // core rows, core columns, non-core rows, columns
  __shared__ int rmin[DB_MAX_EPS][SQD_T];
  __shared__ int cmin[DB_MAX_EPS][SQD_T];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  int bi, bj;
  db_decode_tile(blockIdx.x, tiles, bi, bj);
  const int q0 = bi * SQD_T, r0 = bj * SQD_T;
  const bool diag = bi == bj;
  for (int p = t; p < DB_MAX_EPS * SQD_T; p += 256) {
    (&rmin[0][0])[p] = INT_MAX;
    (&cmin[0][0])[p] = INT_MAX;
  }
  db_stage_core_bits<true>(counts, n, n_eps, min_samples, q0, r0, t, bits, any);
  const unsigned live_r = any[2] & any[1];                           // non-core rows facing core columns
  const unsigned live_c = diag ? 0u : any[3] & any[0];
  if (!(live_r | live_c)) return;                                    // uniform
  double acc[4][4];
  sqd_pair_tile<T, PRE>(X, n, d, q0, r0, xs, ys, t, acc);
  unsigned rb[4], cb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rb[i] = bits[0][ty + 16 * i];
    cb[i] = bits[1][tx + 16 * i];
  }
  for (int e = 0; e < n_eps; ++e) {
    if (!(((live_r | live_c) >> e) & 1u)) continue;
    const double lim = thr.v[e];
    const int* rt = root + (size_t)e * n;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = q0 + ty + 16 * i, c = r0 + tx + 16 * j;
        if (r >= n || c >= n || !(acc[i][j] <= lim)) continue;
        const bool rc = (rb[i] >> e) & 1u, cc = (cb[j] >> e) & 1u;
        if (!rc && cc)
          atomicMin(&rmin[e][ty + 16 * i], rt[c]);
        else if (rc && !cc && !diag)
          atomicMin(&cmin[e][tx + 16 * j], rt[r]);
      }
  }
  __syncthreads();
  for (int p = t; p < n_eps * SQD_T; p += 256) {
    const int e = p >> 6, l = p & 63;
    const int a = rmin[e][l], b = cmin[e][l];
    if (a != INT_MAX && q0 + l < n) atomicMin(&cand[(size_t)e * n + q0 + l], a);
    if (b != INT_MAX && r0 + l < n) atomicMin(&cand[(size_t)e * n + r0 + l], b);
  }
}

// ---- 6. relabel ----------------------------------------------------------------------------------------------------------
// grid (chunks, n_eps), 256 threads: csum[e][c] = the number of roots among the rows of chunk c
__global__ __launch_bounds__(256) void db_flagsum_kernel(const int* __restrict__ root, int n, int chunks,
                                                         int* __restrict__ csum) {
  __shared__ int ws[4];
  const int t = threadIdx.x, e = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * DB_CHUNK;
  int s = 0;
  for (int m = 0; m < DB_CHUNK / 256; ++m) {
    const int64_t r = c0 + t + 256 * m;
    s += (r < n && root[(size_t)e * n + r] == (int)r) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((t & 63) == 0) ws[t >> 6] = s;
  __syncthreads();
  if (t == 0) csum[(size_t)e * chunks + blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// grid n_eps, one thread: the chunk sums become the chunks' first cluster numbers; n_clusters[e] = the total
__global__ void db_chunkscan_kernel(int* __restrict__ csum, int chunks, int* __restrict__ n_clusters) {
  if (threadIdx.x != 0) return;
  int* v = csum + (size_t)blockIdx.x * chunks;
  int s = 0;
  for (int c = 0; c < chunks; ++c) {
    const int x = v[c];
    v[c] = s;
    s += x;
  }
  n_clusters[blockIdx.x] = s;
}

// grid (chunks, n_eps), 256 threads, thread t owns the rows 8 t .. 8 t + 7 of the chunk: scan[e][i] = the number of
// roots below row i
__global__ __launch_bounds__(256) void db_scan_kernel(const int* __restrict__ root, int n, int chunks,
                                                      const int* __restrict__ coff, int* __restrict__ scan) {
  __shared__ int part[256];
  const int t = threadIdx.x, e = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * DB_CHUNK + (int64_t)t * (DB_CHUNK / 256);
  int f[DB_CHUNK / 256];
  int s = 0;
#pragma unroll
  for (int m = 0; m < DB_CHUNK / 256; ++m) {
    const int64_t r = c0 + m;
    f[m] = (r < n && root[(size_t)e * n + r] == (int)r) ? 1 : 0;
    s += f[m];
  }
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                                // inclusive scan of the 256 thread sums
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = coff[(size_t)e * chunks + blockIdx.x] + part[t] - s;
#pragma unroll
  for (int m = 0; m < DB_CHUNK / 256; ++m) {
    const int64_t r = c0 + m;
    if (r < n) scan[(size_t)e * n + r] = run;
    run += f[m];
  }
}

__global__ __launch_bounds__(256) void db_relabel_kernel(const int* __restrict__ root, const int* __restrict__ cand,
                                                         const int* __restrict__ scan, int n, int n_eps,
                                                         int64_t* __restrict__ labels,
                                                         unsigned char* __restrict__ core) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)n * n_eps) return;
  const size_t base = (size_t)(p / n) * n;
  const int r = root[p], c = cand[p];
  int64_t l = -1;
  if (r >= 0 && r < n)
    l = scan[base + r];
  else if (r < 0 && c >= 0 && c < n)
    l = scan[base + c];
  labels[p] = l;
  core[p] = r >= 0 ? 1 : 0;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static inline bool db_shape_ok(int n, int d, int n_eps) {
  return n >= 1 && n <= DB_MAX_N && d >= 1 && d <= DB_MAX_D && n_eps >= 1 && n_eps <= DB_MAX_EPS;
}

struct db_ws {
  int *parent, *root, *cand, *scan, *csum;
};
static size_t db_ws_layout(int n, int n_eps, void* base, db_ws* out) {
  const size_t chunks = ceil_div(n, DB_CHUNK), rows = (size_t)n_eps * n;
  ava_ws_cursor c(base);
  int* parent = c.take<int>(rows);
  int* root = c.take<int>(rows);
  int* cand = c.take<int>(rows);
  int* scan = c.take<int>(rows);
  int* csum = c.take<int>((size_t)n_eps * chunks);
  if (out) *out = db_ws{parent, root, cand, scan, csum};
  return c.bytes();
}

// eps2 (or eps) per radius; false for a radius that is not a positive finite number
static bool db_thresholds(const double* eps, int n_eps, bool pre, db_thr* out) {
  for (int e = 0; e < DB_MAX_EPS; ++e) out->v[e] = -1.0;
  for (int e = 0; e < n_eps; ++e) {
    if (!(eps[e] > 0.0) || !isfinite(eps[e])) return false;
    out->v[e] = pre ? eps[e] : eps[e] * eps[e];
    if (!isfinite(out->v[e])) return false;
  }
  return true;
}

static inline unsigned db_tile_pairs(int n) {
  const int64_t tiles = ceil_div(n, SQD_T);
  return (unsigned)(tiles * (tiles + 1) / 2);
}

extern "C" int ava_db_max_eps(void) { return DB_MAX_EPS; }

extern "C" size_t ava_db_workspace_bytes(int n, int d, int n_eps) {
  if (!db_shape_ok(n, d, n_eps)) return 0;
  return db_ws_layout(n, n_eps, nullptr, nullptr);
}

template <typename T, bool PRE>
static int db_launch_counts(const T* X, int n, int d, const db_thr& thr, int n_eps, int* counts, hipStream_t st) {
  if (hipMemsetAsync(counts, 0, (size_t)n_eps * n * sizeof(int), st) != hipSuccess) return AVA_ELAUNCH;
  hipLaunchKernelGGL((db_count_kernel<T, PRE>), dim3(db_tile_pairs(n)), dim3(256), 0, st, X, n, d, ceil_div(n, SQD_T),
                     thr, n_eps, counts);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename T, bool PRE>
static int db_launch_union(const T* X, int n, int d, const db_thr& thr, int n_eps, int min_samples, const int* counts,
                           const db_ws& w, hipStream_t st) {
  const dim3 rows((unsigned)ceil_div64((int64_t)n * n_eps, 256));
  hipLaunchKernelGGL(db_iota_kernel, rows, dim3(256), 0, st, w.parent, n, n_eps);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL((db_union_kernel<T, PRE>), dim3(db_tile_pairs(n)), dim3(256), 0, st, X, n, d, ceil_div(n, SQD_T),
                     thr, n_eps, min_samples, counts, w.parent);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(db_flatten_kernel, rows, dim3(256), 0, st, w.parent, counts, n, n_eps, min_samples, w.root, w.cand);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename T, bool PRE>
static int db_launch_assign(const T* X, int n, int d, const db_thr& thr, int n_eps, int min_samples, const int* counts,
                            unsigned char* core, int64_t* labels, int* n_clusters, const db_ws& w, hipStream_t st) {
  const int chunks = ceil_div(n, DB_CHUNK);
  hipLaunchKernelGGL((db_border_kernel<T, PRE>), dim3(db_tile_pairs(n)), dim3(256), 0, st, X, n, d, ceil_div(n, SQD_T),
                     thr, n_eps, min_samples, counts, w.root, w.cand);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(db_flagsum_kernel, dim3(chunks, n_eps), dim3(256), 0, st, w.root, n, chunks, w.csum);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(db_chunkscan_kernel, dim3(n_eps), dim3(64), 0, st, w.csum, chunks, n_clusters);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(db_scan_kernel, dim3(chunks, n_eps), dim3(256), 0, st, w.root, n, chunks, w.csum, w.scan);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(db_relabel_kernel, dim3((unsigned)ceil_div64((int64_t)n * n_eps, 256)), dim3(256), 0, st, w.root,
                     w.cand, w.scan, n, n_eps, labels, core);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// steps: 1 = counts, 2 = union + flatten, 4 = border + relabel
template <typename T, bool PRE>
static int db_run_typed(const void* x, int n, int d, const db_thr& thr, int n_eps, int min_samples, int* counts,
                        unsigned char* core, int64_t* labels, int* n_clusters, const db_ws& w, int steps,
                        hipStream_t st) {
  const T* X = static_cast<const T*>(x);
  int rc = AVA_OK;
  if (steps & 1) rc = db_launch_counts<T, PRE>(X, n, d, thr, n_eps, counts, st);
  if (rc == AVA_OK && (steps & 2)) rc = db_launch_union<T, PRE>(X, n, d, thr, n_eps, min_samples, counts, w, st);
  if (rc == AVA_OK && (steps & 4))
    rc = db_launch_assign<T, PRE>(X, n, d, thr, n_eps, min_samples, counts, core, labels, n_clusters, w, st);
  return rc;
}

static int db_run(bool pre, const void* x, int dtype, int n, int d, const double* eps, int n_eps, int min_samples,
                  int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws, size_t ws_bytes,
                  int steps, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !db_shape_ok(n, d, n_eps) || !eps || !counts) return AVA_EINVAL;
  if ((steps & 6) && (min_samples < 1 || !ws)) return AVA_EINVAL;
  if ((steps & 4) && (!core || !labels || !n_clusters)) return AVA_EINVAL;
  db_thr thr;
  if (!db_thresholds(eps, n_eps, pre, &thr)) return AVA_EINVAL;
  db_ws w = db_ws{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (steps & 6) {
    if (ws_bytes < ava_db_workspace_bytes(n, d, n_eps)) return AVA_EWORKSPACE;
    db_ws_layout(n, n_eps, ws, &w);
  }
  hipStream_t st = to_stream(s);
  if (pre)
    return dtype == 0 ? db_run_typed<float, true>(x, n, d, thr, n_eps, min_samples, counts, core, labels, n_clusters, w,
                                                  steps, st)
                      : db_run_typed<double, true>(x, n, d, thr, n_eps, min_samples, counts, core, labels, n_clusters,
                                                   w, steps, st);
  return dtype == 0 ? db_run_typed<float, false>(x, n, d, thr, n_eps, min_samples, counts, core, labels, n_clusters, w,
                                                 steps, st)
                    : db_run_typed<double, false>(x, n, d, thr, n_eps, min_samples, counts, core, labels, n_clusters, w,
                                                  steps, st);
}

extern "C" int ava_db_counts(const void* x, int dtype, int n, int d, const double* eps, int n_eps, int* counts,
                             ava_stream_t s) {
  return db_run(false, x, dtype, n, d, eps, n_eps, 1, counts, nullptr, nullptr, nullptr, nullptr, 0, 1, s);
}

extern "C" int ava_db_counts_pre(const void* dist, int dtype, int n, const double* eps, int n_eps, int* counts,
                                 ava_stream_t s) {
  return db_run(true, dist, dtype, n, 1, eps, n_eps, 1, counts, nullptr, nullptr, nullptr, nullptr, 0, 1, s);
}

extern "C" int ava_db_union(const void* x, int dtype, int n, int d, const double* eps, int n_eps, int min_samples,
                            const int* counts, void* ws, size_t ws_bytes, ava_stream_t s) {
  return db_run(false, x, dtype, n, d, eps, n_eps, min_samples, const_cast<int*>(counts), nullptr, nullptr, nullptr, ws,
                ws_bytes, 2, s);
}

extern "C" int ava_db_union_pre(const void* dist, int dtype, int n, const double* eps, int n_eps, int min_samples,
                                const int* counts, void* ws, size_t ws_bytes, ava_stream_t s) {
  return db_run(true, dist, dtype, n, 1, eps, n_eps, min_samples, const_cast<int*>(counts), nullptr, nullptr, nullptr,
                ws, ws_bytes, 2, s);
}

extern "C" int ava_db_assign(const void* x, int dtype, int n, int d, const double* eps, int n_eps, int min_samples,
                             const int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws,
                             size_t ws_bytes, ava_stream_t s) {
  return db_run(false, x, dtype, n, d, eps, n_eps, min_samples, const_cast<int*>(counts), core, labels, n_clusters, ws,
                ws_bytes, 4, s);
}

extern "C" int ava_db_assign_pre(const void* dist, int dtype, int n, const double* eps, int n_eps, int min_samples,
                                 const int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws,
                                 size_t ws_bytes, ava_stream_t s) {
  return db_run(true, dist, dtype, n, 1, eps, n_eps, min_samples, const_cast<int*>(counts), core, labels, n_clusters, ws,
                ws_bytes, 4, s);
}

extern "C" int ava_db_labels(const void* x, int dtype, int n, int d, const double* eps, int n_eps, int min_samples,
                             const int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws,
                             size_t ws_bytes, ava_stream_t s) {
  return db_run(false, x, dtype, n, d, eps, n_eps, min_samples, const_cast<int*>(counts), core, labels, n_clusters, ws,
                ws_bytes, 6, s);
}

extern "C" int ava_db_labels_pre(const void* dist, int dtype, int n, const double* eps, int n_eps, int min_samples,
                                 const int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws,
                                 size_t ws_bytes, ava_stream_t s) {
  return db_run(true, dist, dtype, n, 1, eps, n_eps, min_samples, const_cast<int*>(counts), core, labels, n_clusters, ws,
                ws_bytes, 6, s);
}
