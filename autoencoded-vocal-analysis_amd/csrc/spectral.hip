// Connected components and thick-restart Lanczos over a symmetric sparse graph (the
// definitions and the sum orders are in include/ava_spectral.h).  The operator is M = D^-1/2 A D^-1/2 without the
// diagonal, I - L_sym; the host (ava_amd/spectral.py) holds only the projected matrix of a restart cycle.
//
// components  parent[i] <= i always points into i's component.  A round hooks the parent of every row below the least
//             parent among its neighbours (integer atomicMin) and then compresses every chain to its root; when a round
//             hooks nothing every parent is the smallest row of its component.  Roots are ranked by a chunked scan.
// rows        16 lanes per CSR row: lane l takes the entries l, l + 16, ... ascending, a butterfly adds the 16 sums.
// B^T w       a workgroup per 1024-row chunk and 16 basis vectors, a wavefront per vector: lane rows lane + 64 k
//             ascending, a butterfly over the lanes; partial [chunk][vector], added over the chunks ascending by
//             sp_reduce_kernel.  About 8 n m bytes, as is w -= B h (a thread per row, the vectors ascending).
// norm        the second update squares its rows: a partial per 256-row block, added by one fixed tree in sp_scale_kernel.
// No floating-point atomics; no sum depends on the grid.
#include <limits.h>

#include "common.h"

#define SP_MAX_N (1 << 30)
#define SP_MAX_BASIS 1024
#define SP_CHUNK 1024                // rows per partial sum of B^T w
#define SP_COLS 16                   // basis vectors per workgroup of sp_dot_kernel
#define SP_LANES 16                  // lanes per CSR row
#define SP_ROT_TILE 8                // output vectors per thread of sp_rotate_kernel

// ---- the graph check ---------------------------------------------------------------------------------------------------
// flag[0] |= 1 unless indptr ascends from 0 to nnz and every col is a row number
__global__ __launch_bounds__(256) void sp_check_kernel(const int64_t* __restrict__ indptr, const int* __restrict__ col,
                                                       int n, int64_t nnz, int* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (e < n) {
    const int64_t a = indptr[e], b = indptr[e + 1];
    bad = a < 0 || b < a || b > nnz || (e == 0 && a != 0) || (e == n - 1 && b != nnz);
  }
  if (e < nnz) {
    const int c = col[e];
    bad = bad || c < 0 || c >= n;
  }
  if (bad) atomicOr(flag, 1);
}

__device__ __forceinline__ double sp_lanes_sum(double v) {
#pragma unroll
  for (int o = SP_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, SP_LANES);
  return v;
}

// ---- components --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_iota_kernel(int* __restrict__ parent, int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = (int)i;
}

__global__ __launch_bounds__(256) void sp_cc_hook_kernel(const int64_t* __restrict__ indptr, const int* __restrict__ col,
                                                         const double* __restrict__ val, int n, int* parent,
                                                         int* __restrict__ flag) {
  const int64_t row = (int64_t)blockIdx.x * (256 / SP_LANES) + (threadIdx.x / SP_LANES);
  const int l = threadIdx.x % SP_LANES;
  int mn = INT_MAX;
  if (row < n) {
    const int64_t e1 = indptr[row + 1];
    for (int64_t e = indptr[row] + l; e < e1; e += SP_LANES) {
      const int c = col[e];
      if (c != row && val[e] != 0.0) {
        const int p = __atomic_load_n(&parent[c], __ATOMIC_RELAXED);
        mn = p < mn ? p : mn;
      }
    }
  }
#pragma unroll
  for (int o = SP_LANES / 2; o > 0; o >>= 1) {
    const int other = __shfl_xor(mn, o, SP_LANES);
    mn = other < mn ? other : mn;
  }
  if (row < n && l == 0) {
    const int p = __atomic_load_n(&parent[row], __ATOMIC_RELAXED);
    if (mn < p) {
      atomicMin(&parent[p], mn);
      atomicMin(&parent[row], mn);
      flag[0] = 1;
    }
  }
}

// every chain to its root: a root stays one for the whole launch (only its own thread writes it, and writes itself)
__global__ __launch_bounds__(256) void sp_cc_jump_kernel(int* parent, int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int p = __atomic_load_n(&parent[i], __ATOMIC_RELAXED);
  for (;;) {
    const int q = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
    if (q == p) break;
    p = q;
  }
  __atomic_store_n(&parent[i], p, __ATOMIC_RELAXED);
}

// rank[i] = the roots among the rows of i's chunk before i (roots only); ccount[chunk] = the chunk's roots.  Thread t
// owns the rows 4 t .. 4 t + 3 of the chunk.
__global__ __launch_bounds__(256) void sp_cc_rank_kernel(const int* __restrict__ parent, int n, int* __restrict__ rank,
                                                         int* __restrict__ ccount) {
  __shared__ int scan[256];
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * SP_CHUNK + 4 * t;
  int root[4], mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    root[k] = (r0 + k < n && parent[r0 + k] == r0 + k) ? 1 : 0;
    mine += root[k];
  }
  scan[t] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int add = t >= o ? scan[t - o] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  int before = scan[t] - mine;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (r0 + k < n) rank[r0 + k] = before;
    before += root[k];
  }
  if (t == 255) ccount[blockIdx.x] = scan[255];
}

// coff [nchunks + 1]: the exclusive scan of ccount, one workgroup; thread t scans a run of chunks
__global__ __launch_bounds__(256) void sp_cc_scan_kernel(const int* __restrict__ ccount, int nchunks,
                                                         int* __restrict__ coff) {
  __shared__ int tot[256];
  const int t = threadIdx.x;
  const int per = (nchunks + 255) / 256;
  const int a = t * per < nchunks ? t * per : nchunks, b = a + per < nchunks ? a + per : nchunks;
  int s = 0;
  for (int c = a; c < b; ++c) s += ccount[c];
  tot[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int u = 0; u < 256; ++u) {
      const int v = tot[u];
      tot[u] = run;
      run += v;
    }
    coff[nchunks] = run;
  }
  __syncthreads();
  s = tot[t];
  for (int c = a; c < b; ++c) {
    coff[c] = s;
    s += ccount[c];
  }
}

__global__ __launch_bounds__(256) void sp_cc_label_kernel(const int* __restrict__ parent, const int* __restrict__ rank,
                                                          const int* __restrict__ coff, int n, int* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = parent[i];
  labels[i] = coff[p / SP_CHUNK] + rank[p];
}

// ---- degrees and the operator ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_degree_kernel(const int64_t* __restrict__ indptr, const int* __restrict__ col,
                                                        const double* __restrict__ val, int n, double* __restrict__ deg,
                                                        double* __restrict__ dd) {
  const int64_t row = (int64_t)blockIdx.x * (256 / SP_LANES) + (threadIdx.x / SP_LANES);
  const int l = threadIdx.x % SP_LANES;
  double s = 0.0;
  if (row < n) {
    const int64_t e1 = indptr[row + 1];
    for (int64_t e = indptr[row] + l; e < e1; e += SP_LANES)
      if (col[e] != row) s += val[e];
  }
  s = sp_lanes_sum(s);
  if (row < n && l == 0) {
    deg[row] = s;
    dd[row] = s == 0.0 ? 1.0 : sqrt(s);
  }
}

__global__ __launch_bounds__(256) void sp_dinv_kernel(const double* __restrict__ dd, int n, double* __restrict__ dinv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dinv[i] = 1.0 / dd[i];
}

__global__ __launch_bounds__(256) void sp_op_kernel(const int64_t* __restrict__ indptr, const int* __restrict__ col,
                                                    const double* __restrict__ val, const double* __restrict__ dinv,
                                                    int n, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t row = (int64_t)blockIdx.x * (256 / SP_LANES) + (threadIdx.x / SP_LANES);
  const int l = threadIdx.x % SP_LANES;
  double s = 0.0;
  if (row < n) {
    const int64_t e1 = indptr[row + 1];
    for (int64_t e = indptr[row] + l; e < e1; e += SP_LANES) {
      const int c = col[e];
      if (c != row) s = fma(val[e], x[c] * dinv[c], s);
    }
  }
  s = sp_lanes_sum(s);
  if (row < n && l == 0) y[row] = s * dinv[row];
}

// ---- the tall-skinny products ------------------------------------------------------------------------------------------
// partial [chunk][m]: the chunk's share of B^T w for the vectors 16 blockIdx.y .. + 15, wavefront wv those = wv mod 4
__global__ __launch_bounds__(256) void sp_dot_kernel(const double* __restrict__ B, int n, int m,
                                                     const double* __restrict__ w, double* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * SP_CHUNK + lane;
  double wr[SP_CHUNK / 64];
#pragma unroll
  for (int k = 0; k < SP_CHUNK / 64; ++k) wr[k] = r0 + 64 * k < n ? w[r0 + 64 * k] : 0.0;
  for (int c = blockIdx.y * SP_COLS + wv; c < m && c < (int)(blockIdx.y + 1) * SP_COLS; c += 4) {
    const double* b = B + (size_t)c * n;
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < SP_CHUNK / 64; ++k) p = fma(r0 + 64 * k < n ? b[r0 + 64 * k] : 0.0, wr[k], p);
    p = wave_sum_d(p);
    if (lane == 0) partial[(size_t)blockIdx.x * m + c] = p;
  }
}

// h [m]: the chunks ascending; acc[0] takes (add = 0) or adds (add = 1) the coefficient of vector m - 1
__global__ __launch_bounds__(256) void sp_reduce_kernel(const double* __restrict__ partial, int nchunks, int m,
                                                        double* __restrict__ h, double* __restrict__ acc, int add) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  double s = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) s += partial[(size_t)ch * m + c];
  h[c] = s;
  if (acc != nullptr && c == m - 1) acc[0] = add ? acc[0] + s : s;
}

// w -= B h, the vectors ascending; NORM: normp[block] = the sum of the block's squared rows
template <bool NORM>
__global__ __launch_bounds__(256) void sp_update_kernel(const double* __restrict__ B, int n, int m,
                                                        const double* __restrict__ h, double* __restrict__ w,
                                                        double* __restrict__ normp) {
  __shared__ double hs[SP_MAX_BASIS];
  __shared__ double wsum[4];
  const int t = threadIdx.x;
  for (int c = t; c < m; c += 256) hs[c] = h[c];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + t;
  double s = 0.0;
  if (i < n) {
    s = w[i];
    const double* b = B + i;
#pragma unroll 8
    for (int c = 0; c < m; ++c) s = fma(-b[(size_t)c * n], hs[c], s);
    w[i] = s;
  }
  if (NORM) {
    const double q = wave_sum_d(i < n ? s * s : 0.0);
    if ((t & 63) == 0) wsum[t >> 6] = q;
    __syncthreads();
    if (t == 0) normp[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  }
}

// out = w / |w| with |w|^2 the fixed tree over normp [nblk]; norm[0] = |w|; the zero vector where |w| <= breakdown
__global__ __launch_bounds__(256) void sp_scale_kernel(const double* __restrict__ w, int n,
                                                       const double* __restrict__ normp, int nblk, double breakdown,
                                                       double* __restrict__ norm, double* __restrict__ out) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int b = t; b < nblk; b += 256) s += normp[b];
  part[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) part[t] += part[t + o];
    __syncthreads();
  }
  const double len = sqrt(part[0]);
  const double inv = len > breakdown ? 1.0 / len : 0.0;
  const int64_t i = (int64_t)blockIdx.x * 256 + t;
  if (i < n) out[i] = w[i] * inv;
  if (blockIdx.x == 0 && t == 0) norm[0] = len;
}

__global__ __launch_bounds__(256) void sp_null_kernel(const int* __restrict__ labels, const double* __restrict__ dd,
                                                      int n, double* __restrict__ B) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) B[(size_t)blockIdx.y * n + i] = labels[i] == (int)blockIdx.y ? dd[i] : 0.0;
}

__global__ __launch_bounds__(256) void sp_hash_kernel(int n, uint64_t seed, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) w[i] = ava_u01_hash((uint64_t)i, seed) - 0.5;
}

// out[k] = sum_c B[c] S[c][k], c ascending, for the 8 vectors k of tile blockIdx.y: a thread per row
__global__ __launch_bounds__(256) void sp_rotate_kernel(const double* __restrict__ B, int n, int ncv, int keep,
                                                        const double* __restrict__ S, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int k0 = blockIdx.y * SP_ROT_TILE;
  if (i >= n) return;
  double acc[SP_ROT_TILE];
#pragma unroll
  for (int u = 0; u < SP_ROT_TILE; ++u) acc[u] = 0.0;
  for (int c = 0; c < ncv; ++c) {
    const double v = B[(size_t)c * n + i];
#pragma unroll
    for (int u = 0; u < SP_ROT_TILE; ++u)
      acc[u] = fma(v, k0 + u < keep ? S[(size_t)c * keep + k0 + u] : 0.0, acc[u]);
  }
#pragma unroll
  for (int u = 0; u < SP_ROT_TILE; ++u)
    if (k0 + u < keep) out[(size_t)(k0 + u) * n + i] = acc[u];
}

// ---- host --------------------------------------------------------------------------------------------------------------
extern "C" int ava_sp_max_n(void) { return SP_MAX_N; }
extern "C" int ava_sp_max_basis(void) { return SP_MAX_BASIS; }
extern "C" int ava_sp_chunk_rows(void) { return SP_CHUNK; }
extern "C" int ava_sp_rotate_tile(void) { return SP_ROT_TILE; }

struct sp_ws {
  int* flag;
  int* parent;
  int* rank;
  int* ccount;
  int* coff;
  double* dinv;
  double* w;
  double* partial;
  double* h;
  double* normp;
  double* rot;
  size_t bytes;
};

static inline int sp_chunks(int n) { return ceil_div(n, SP_CHUNK); }
static inline unsigned sp_blocks(int64_t n) { return (unsigned)ceil_div64(n, 256); }
static bool sp_shape_ok(int n, int capacity) {
  return n >= 1 && n <= SP_MAX_N && capacity >= 1 && capacity <= SP_MAX_BASIS;
}

static sp_ws sp_carve(void* base, int n, int capacity) {
  ava_ws_cursor c(base);
  sp_ws w;
  const size_t nc = (size_t)sp_chunks(n);
  w.flag = c.take<int>(1);
  w.parent = c.take<int>((size_t)n);
  w.rank = c.take<int>((size_t)n);
  w.ccount = c.take<int>(nc);
  w.coff = c.take<int>(nc + 1);
  w.dinv = c.take<double>((size_t)n);
  w.w = c.take<double>((size_t)n);
  w.partial = c.take<double>(nc * capacity);
  w.h = c.take<double>((size_t)capacity);
  w.normp = c.take<double>((size_t)sp_blocks(n));
  w.rot = c.take<double>((size_t)n * capacity);
  w.bytes = c.bytes();
  return w;
}

extern "C" size_t ava_sp_workspace_bytes(int n, int capacity) {
  return sp_shape_ok(n, capacity) ? sp_carve(nullptr, n, capacity).bytes : 0;
}

// AVA_OK when the graph may be followed; the call waits for the device's answer
static int sp_check_graph(const int64_t* indptr, const int* col, int n, int64_t nnz, int* flag, hipStream_t st) {
  if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) return AVA_ELAUNCH;
  const int64_t span = nnz > n ? nnz : n;
  if (ceil_div64(span, 256) > INT_MAX) return AVA_EINVAL;
  hipLaunchKernelGGL(sp_check_kernel, dim3(sp_blocks(span)), dim3(256), 0, st, indptr, col, n, nnz, flag);
  AVA_CHECK_LAUNCH();
  int bad = 0;
  if (hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return AVA_ELAUNCH;
  return bad != 0 ? AVA_EINVAL : AVA_OK;
}

static bool sp_graph_args_ok(const int64_t* indptr, const int* col, const double* val, int n, int64_t nnz) {
  return indptr != nullptr && n >= 1 && n <= SP_MAX_N && nnz >= 0 && (nnz == 0 || (col != nullptr && val != nullptr));
}

static inline unsigned sp_row_blocks(int n) { return (unsigned)ceil_div64(n, 256 / SP_LANES); }

extern "C" int ava_sp_components(const int64_t* indptr, const int* col, const double* val, int n, int64_t nnz,
                                 int* labels, int* count, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!sp_graph_args_ok(indptr, col, val, n, nnz) || labels == nullptr || count == nullptr || ws == nullptr)
    return AVA_EINVAL;
  if (ws_bytes < ava_sp_workspace_bytes(n, 1)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  const sp_ws w = sp_carve(ws, n, 1);
  const int rc = sp_check_graph(indptr, col, n, nnz, w.flag, st);
  if (rc != AVA_OK) return rc;
  hipLaunchKernelGGL(sp_iota_kernel, dim3(sp_blocks(n)), dim3(256), 0, st, w.parent, n);
  AVA_CHECK_LAUNCH();
  for (;;) {
    if (hipMemsetAsync(w.flag, 0, sizeof(int), st) != hipSuccess) return AVA_ELAUNCH;
    hipLaunchKernelGGL(sp_cc_hook_kernel, dim3(sp_row_blocks(n)), dim3(256), 0, st, indptr, col, val, n, w.parent,
                       w.flag);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_cc_jump_kernel, dim3(sp_blocks(n)), dim3(256), 0, st, w.parent, n);
    AVA_CHECK_LAUNCH();
    int changed = 0;
    if (hipMemcpyAsync(&changed, w.flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return AVA_ELAUNCH;
    if (changed == 0) break;
  }
  const int nc = sp_chunks(n);
  hipLaunchKernelGGL(sp_cc_rank_kernel, dim3(nc), dim3(256), 0, st, w.parent, n, w.rank, w.ccount);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_cc_scan_kernel, dim3(1), dim3(256), 0, st, w.ccount, nc, w.coff);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_cc_label_kernel, dim3(sp_blocks(n)), dim3(256), 0, st, w.parent, w.rank, w.coff, n, labels);
  AVA_CHECK_LAUNCH();
  if (hipMemcpyAsync(count, w.coff + nc, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return AVA_ELAUNCH;
  return AVA_OK;
}

extern "C" int ava_sp_degrees(const int64_t* indptr, const int* col, const double* val, int n, int64_t nnz, double* deg,
                              double* dd, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!sp_graph_args_ok(indptr, col, val, n, nnz) || deg == nullptr || dd == nullptr || ws == nullptr)
    return AVA_EINVAL;
  if (ws_bytes < ava_sp_workspace_bytes(n, 1)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  const sp_ws w = sp_carve(ws, n, 1);
  const int rc = sp_check_graph(indptr, col, n, nnz, w.flag, st);
  if (rc != AVA_OK) return rc;
  hipLaunchKernelGGL(sp_degree_kernel, dim3(sp_row_blocks(n)), dim3(256), 0, st, indptr, col, val, n, deg, dd);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

static int sp_dinv(const double* dd, int n, double* dinv, hipStream_t st) {
  hipLaunchKernelGGL(sp_dinv_kernel, dim3(sp_blocks(n)), dim3(256), 0, st, dd, n, dinv);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_sp_apply(const int64_t* indptr, const int* col, const double* val, const double* dd, int n,
                            int64_t nnz, const double* x, double* y, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!sp_graph_args_ok(indptr, col, val, n, nnz) || dd == nullptr || x == nullptr || y == nullptr || x == y ||
      ws == nullptr)
    return AVA_EINVAL;
  if (ws_bytes < ava_sp_workspace_bytes(n, 1)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  const sp_ws w = sp_carve(ws, n, 1);
  int rc = sp_check_graph(indptr, col, n, nnz, w.flag, st);
  if (rc != AVA_OK) return rc;
  if ((rc = sp_dinv(dd, n, w.dinv, st)) != AVA_OK) return rc;
  hipLaunchKernelGGL(sp_op_kernel, dim3(sp_row_blocks(n)), dim3(256), 0, st, indptr, col, val, w.dinv, n, x, y);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// h = B^T w over the m vectors of B; acc as in sp_reduce_kernel
static int sp_project(const sp_ws& w, const double* B, int n, int m, double* acc, int add, hipStream_t st) {
  hipLaunchKernelGGL(sp_dot_kernel, dim3(sp_chunks(n), ceil_div(m, SP_COLS)), dim3(256), 0, st, B, n, m, w.w, w.partial);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_reduce_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, w.partial, sp_chunks(n), m, w.h, acc,
                     add);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// w.w, orthogonalised twice against the m vectors of B (m may be 0) and normalised, to out; norm[0] its length before
static int sp_orth_normalise(const sp_ws& w, const double* B, int n, int m, double* acc, double breakdown, double* norm,
                             double* out, hipStream_t st) {
  int rc;
  if (m > 0) {
    if ((rc = sp_project(w, B, n, m, acc, 0, st)) != AVA_OK) return rc;
    hipLaunchKernelGGL(sp_update_kernel<false>, dim3(sp_blocks(n)), dim3(256), 0, st, B, n, m, w.h, w.w, w.normp);
    AVA_CHECK_LAUNCH();
    if ((rc = sp_project(w, B, n, m, acc, 1, st)) != AVA_OK) return rc;
  }
  hipLaunchKernelGGL(sp_update_kernel<true>, dim3(sp_blocks(n)), dim3(256), 0, st, B, n, m, w.h, w.w, w.normp);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_scale_kernel, dim3(sp_blocks(n)), dim3(256), 0, st, w.w, n, w.normp, (int)sp_blocks(n),
                     breakdown, norm, out);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_sp_null_vectors(const int* labels, const double* dd, int n, int k, double* basis, int capacity,
                                   void* ws, size_t ws_bytes, ava_stream_t s) {
  if (labels == nullptr || dd == nullptr || basis == nullptr || ws == nullptr || !sp_shape_ok(n, capacity) || k < 1 ||
      k > capacity)
    return AVA_EINVAL;
  if (ws_bytes < ava_sp_workspace_bytes(n, capacity)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  const sp_ws w = sp_carve(ws, n, capacity);
  hipLaunchKernelGGL(sp_null_kernel, dim3(sp_blocks(n), k), dim3(256), 0, st, labels, dd, n, basis);
  AVA_CHECK_LAUNCH();
  for (int c = 0; c < k; ++c) {
    double* v = basis + (size_t)c * n;
    if (hipMemcpyAsync(w.w, v, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return AVA_ELAUNCH;
    const int rc = sp_orth_normalise(w, basis, n, 0, nullptr, 0.0, w.h, v, st);
    if (rc != AVA_OK) return rc;
  }
  return AVA_OK;
}

extern "C" int ava_sp_start(double* basis, int n, int capacity, int nlock, uint64_t seed, double breakdown,
                            double* norm, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (basis == nullptr || norm == nullptr || ws == nullptr || !sp_shape_ok(n, capacity) || nlock < 0 ||
      nlock + 1 > capacity || !(breakdown >= 0.0))
    return AVA_EINVAL;
  if (ws_bytes < ava_sp_workspace_bytes(n, capacity)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  const sp_ws w = sp_carve(ws, n, capacity);
  hipLaunchKernelGGL(sp_hash_kernel, dim3(sp_blocks(n)), dim3(256), 0, st, n, seed, w.w);
  AVA_CHECK_LAUNCH();
  return sp_orth_normalise(w, basis, n, nlock, nullptr, breakdown, norm, basis + (size_t)nlock * n, st);
}

extern "C" int ava_sp_lanczos(const int64_t* indptr, const int* col, const double* val, const double* dd, int n,
                              int64_t nnz, double* basis, int capacity, int nlock, int j0, int j1, double breakdown,
                              double* alpha, double* beta, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!sp_graph_args_ok(indptr, col, val, n, nnz) || dd == nullptr || basis == nullptr || alpha == nullptr ||
      beta == nullptr || ws == nullptr || !sp_shape_ok(n, capacity) || nlock < 0 || j0 < 0 || j1 < j0 ||
      (int64_t)nlock + j1 + 1 > capacity || !(breakdown >= 0.0))
    return AVA_EINVAL;
  if (ws_bytes < ava_sp_workspace_bytes(n, capacity)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  const sp_ws w = sp_carve(ws, n, capacity);
  int rc = sp_check_graph(indptr, col, n, nnz, w.flag, st);
  if (rc != AVA_OK) return rc;
  if ((rc = sp_dinv(dd, n, w.dinv, st)) != AVA_OK) return rc;
  for (int j = j0; j < j1; ++j) {
    const int m = nlock + j + 1;
    hipLaunchKernelGGL(sp_op_kernel, dim3(sp_row_blocks(n)), dim3(256), 0, st, indptr, col, val, w.dinv, n,
                       basis + (size_t)(m - 1) * n, w.w);
    AVA_CHECK_LAUNCH();
    if ((rc = sp_orth_normalise(w, basis, n, m, alpha + j, breakdown, beta + j, basis + (size_t)m * n, st)) != AVA_OK)
      return rc;
  }
  return AVA_OK;
}

extern "C" int ava_sp_rotate(double* basis, int n, int capacity, int ncv, int keep, const double* S, void* ws,
                             size_t ws_bytes, ava_stream_t s) {
  if (basis == nullptr || S == nullptr || ws == nullptr || !sp_shape_ok(n, capacity) || ncv > capacity || keep < 1 ||
      keep > ncv)
    return AVA_EINVAL;
  if (ws_bytes < ava_sp_workspace_bytes(n, capacity)) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  const sp_ws w = sp_carve(ws, n, capacity);
  hipLaunchKernelGGL(sp_rotate_kernel, dim3(sp_blocks(n), ceil_div(keep, SP_ROT_TILE)), dim3(256), 0, st, basis, n, ncv,
                     keep, S, w.rot);
  AVA_CHECK_LAUNCH();
  if (hipMemcpyAsync(basis, w.rot, (size_t)n * keep * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return AVA_ELAUNCH;
  return AVA_OK;
}
