// HDBSCAN of latent rows: the device side of scikit-learn 1.7's sklearn/cluster/_hdbscan
// (hdbscan.py, _reachability.pyx, _linkage.pyx, _tree.pyx).  X is [N][d] float32 or float64 and is converted on load;
// everything else is fp64 or integer.
//
// Pair measure m(i, j): the d2 of sqdist_tile.h (direct differences, one fma per feature, features ascending, so
// m(i, j) and m(j, i) have the same bits), or (double)D[i][j] of a SYMMETRIC precomputed matrix; no square root anywhere.
// core[i] = the min_samples-th smallest m(i, .), the row itself (0) counted first; w(i, j) = max(core[i], core[j], m).
// Edges are compared by the key (w, m, min(i, j), max(i, j)), lexicographically: a strict total order, so the minimum
// spanning tree of the mutual-reachability graph is unique and Boruvka's rounds cannot close a cycle.
//
// One round = these launches; the end of a launch is the only barrier, no workgroup waits for another, and every step
// is a minimum under the key or an integer atomic, so the outcome does not depend on the grid or the interleaving:
//   hd_round_init_kernel  best[c] = all ones, parent[i] = i
//   hd_rowmin_kernel      grid (strips, segs): a workgroup owns a 64-row strip and the column tiles of one segment and
//                         leaves per row the least (w, m, j) over the columns j with comp[j] != comp[i].  A tile whose
//                         columns and the strip's rows all carry ONE component id (the per-block (min, max) of comp) is
//                         skipped before any distance is formed: late rounds form almost nothing.
//   hd_compmin_kernel<S>  three staged 64-bit atomicMins per candidate onto its component: the order-preserving bits of
//                         w, then of m among the candidates still tied, then the packed (min(i, j) << 32 | max(i, j))
//   hd_hook_kernel        parent[c] = the component of the chosen edge's far end; a mutual pick is the only possible
//                         cycle and its smaller id stays the root.  Every chosen edge is emitted once (by the component
//                         that hooks) through an atomicAdd cursor; the caller sorts the list by key.
//   hd_jump_kernel        pointer jumping, ceil(log2(components)) + 1 launches: a hook tree is no deeper than the
//                         number of components and every launch at least halves the depth
//   hd_relabel_kernel     comp[i] = parent[comp[i]] and the (min, max) of comp per 64-row block
// The host reads one word per round, the edge cursor: components = N - edges.  Every round at least halves the
// components, so ceil(log2 N) rounds suffice; the driver returns AVA_ELAUNCH instead of running one more.
//
// ava_hd_tree is host code and makes no HIP call: sklearn's make_single_linkage, _condense_tree, _compute_stability,
// _get_clusters ('eom' / 'leaf'), _do_labelling and get_probabilities on the N - 1 sorted edges, in O(N alpha(N)).
#include <limits.h>
#include <math.h>

#include <vector>

#include "common.h"
#include "sqdist_tile.h"

#define HD_MAX_N (1 << 21)
#define HD_MAX_D 65536
#define HD_MAX_K 64              // projection.MAX_K
#define HD_MAX_SEG 8             // column segments of a strip: strips * segs is about 4096 workgroups, at most 8 a strip
#define HD_NONE 0xFFFFFFFFFFFFFFFFull

typedef unsigned long long hd_u64;

// fp64 -> 64 bits whose unsigned order is the order of the numbers (-0 < +0; no NaN reaches here), and back
__device__ __forceinline__ hd_u64 hd_ord(double x) {
  const hd_u64 b = (hd_u64)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double hd_unord(hd_u64 k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// ---- core measures -------------------------------------------------------------------------------------------------------
// euclidean: kth[i] is the row of the min_samples-th neighbour (ava_pj_knn); its d2 again in the tile's fma order
template <typename T>
__global__ __launch_bounds__(256) void hd_core_kernel(const T* __restrict__ X, int n, int d,
                                                      const int64_t* __restrict__ kth, double* __restrict__ core) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t j = kth[i];
  if (j < 0 || j >= n) {                                             // not a row: never read
    core[i] = INFINITY;
    return;
  }
  const T* a = X + (size_t)i * d;
  const T* b = X + (size_t)j * d;
  double s = 0.0;
  for (int k = 0; k < d; ++k) {
    const double df = (double)a[k] - (double)b[k];
    s = fma(df, df, s);
  }
  core[i] = s;
}

// precomputed: a workgroup per row takes the next (value, column) of the row k times; the diagonal counts as 0
template <typename T>
__global__ __launch_bounds__(256) void hd_core_pre_kernel(const T* __restrict__ D, int n, int k,
                                                          double* __restrict__ core) {
  __shared__ hd_u64 wv[4];
  __shared__ int wc[4];
  const int t = threadIdx.x, i = blockIdx.x;
  const T* row = D + (size_t)i * n;
  hd_u64 lv = 0;
  int lc = -1;                                                       // the key taken last; lc < 0: none yet
  for (int r = 0; r < k; ++r) {
    hd_u64 bv = HD_NONE;
    int bc = INT_MAX;
    for (int c = t; c < n; c += 256) {
      const hd_u64 v = hd_ord(c == i ? 0.0 : (double)row[c]);
      const bool after = lc < 0 || v > lv || (v == lv && c > lc);
      if (after && (v < bv || (v == bv && c < bc))) {
        bv = v;
        bc = c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const hd_u64 ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (ov < bv || (ov == bv && oc < bc)) {
        bv = ov;
        bc = oc;
      }
    }
    __syncthreads();                                                 // the round before has read wv / wc
    if ((t & 63) == 0) {
      wv[t >> 6] = bv;
      wc[t >> 6] = bc;
    }
    __syncthreads();
    lv = wv[0];
    lc = wc[0];
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (wv[q] < lv || (wv[q] == lv && wc[q] < lc)) {
        lv = wv[q];
        lc = wc[q];
      }
  }
  if (t == 0) core[i] = hd_unord(lv);
}

// ---- Boruvka rounds ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hd_start_kernel(int* __restrict__ comp, int2* __restrict__ brange, int n,
                                                       int* __restrict__ cursor) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *cursor = 0;
  if (i >= n) return;
  comp[i] = i;
  if ((i & (SQD_T - 1)) == 0) brange[i / SQD_T] = make_int2(i, i + SQD_T - 1 < n ? i + SQD_T - 1 : n - 1);
}

__global__ __launch_bounds__(256) void hd_round_init_kernel(hd_u64* __restrict__ bw, hd_u64* __restrict__ bm,
                                                            hd_u64* __restrict__ be, int* __restrict__ parent, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bw[i] = HD_NONE;
  bm[i] = HD_NONE;
  be[i] = HD_NONE;
  parent[i] = i;
}

// grid (tiles, segs), 256 threads; cand_* are [segs][n], cand_j < 0: the row has no candidate in this segment
template <typename T, bool PRE>
__global__ __launch_bounds__(256) void hd_rowmin_kernel(const T* __restrict__ X, int n, int d, int tiles, int per_seg,
                                                        const double* __restrict__ core, const int* __restrict__ comp,
                                                        const int2* __restrict__ brange, double* __restrict__ cand_w,
                                                        double* __restrict__ cand_m, int* __restrict__ cand_j) {
  __shared__ double xs[PRE ? SQD_T * 16 : SQD_T * SQD_LD];            // the stage, then the rows' 16 partial minima
  __shared__ double ys[PRE ? SQD_T * 16 : SQD_T * SQD_LD];
  __shared__ double rcore[SQD_T], ccore[SQD_T];
  __shared__ int rcomp[SQD_T], ccomp[SQD_T];
  __shared__ int red_j[SQD_T * 16];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int bi = blockIdx.x, q0 = bi * SQD_T;
  const int b_lo = blockIdx.y * per_seg, b_hi = b_lo + per_seg < tiles ? b_lo + per_seg : tiles;
  if (t < SQD_T) {
    const int r = q0 + t;
    rcomp[t] = r < n ? comp[r] : -1;
    rcore[t] = r < n ? core[r] : 0.0;
  }
  const int2 rr = brange[bi];
  double bw[4], bm[4];
  int bj[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bw[i] = INFINITY;
    bm[i] = INFINITY;
    bj[i] = -1;
  }
  for (int b = b_lo; b < b_hi; ++b) {
    const int2 cr = brange[b];
    if (rr.x == rr.y && cr.x == cr.y && cr.x == rr.x) continue;     // uniform: one component on both sides
    const int r0 = b * SQD_T;
    __syncthreads();                                                 // the tile before has read ccomp / ccore
    if (t < SQD_T) {
      const int c = r0 + t;
      ccomp[t] = c < n ? comp[c] : -1;
      ccore[t] = c < n ? core[c] : 0.0;
    }
    double acc[4][4];
    sqd_pair_tile<T, PRE>(X, n, d, q0, r0, xs, ys, t, acc);         // its barriers also publish ccomp (d >= 1)
    if (PRE) __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                    // columns ascending: only a smaller (w, m) replaces
      const int cl = tx + 16 * j, c = r0 + cl;
      if (c >= n) continue;
      const int cc = ccomp[cl];
      const double ccr = ccore[cl];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rl = ty + 16 * i;
        if (q0 + rl >= n || rcomp[rl] == cc) continue;
        const double m = acc[i][j];
        const double w = fmax(fmax(rcore[rl], ccr), m);
        if (bj[i] < 0 || w < bw[i] || (w == bw[i] && m < bm[i])) {
          bw[i] = w;
          bm[i] = m;
          bj[i] = c;
        }
      }
    }
  }
  // the 16 partial candidates of every row through LDS (over the staging arrays), then a thread per row
  __syncthreads();                                                   // the last tile's stage is consumed
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int slot = (ty + 16 * i) * 16 + tx;
    xs[slot] = bw[i];
    ys[slot] = bm[i];
    red_j[slot] = bj[i];
  }
  __syncthreads();
  if (t < SQD_T && q0 + t < n) {
    double w = xs[t * 16], m = ys[t * 16];
    int j = red_j[t * 16];
    for (int q = 1; q < 16; ++q) {
      const double ow = xs[t * 16 + q], om = ys[t * 16 + q];
      const int oj = red_j[t * 16 + q];
      if (oj < 0) continue;
      if (j < 0 || ow < w || (ow == w && (om < m || (om == m && oj < j)))) {
        w = ow;
        m = om;
        j = oj;
      }
    }
    const size_t p = (size_t)blockIdx.y * n + q0 + t;
    cand_w[p] = w;
    cand_m[p] = m;
    cand_j[p] = j;
  }
}

// S = 0: w, 1: m among the candidates with the component's w, 2: the rows among those with its (w, m)
template <int S>
__global__ __launch_bounds__(256) void hd_compmin_kernel(const double* __restrict__ cand_w,
                                                         const double* __restrict__ cand_m,
                                                         const int* __restrict__ cand_j, const int* __restrict__ comp,
                                                         int n, int segs, hd_u64* bw, hd_u64* bm, hd_u64* be) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)n * segs) return;
  const int j = cand_j[p];
  if (j < 0) return;
  const int i = (int)(p % n), c = comp[i];
  const hd_u64 w = hd_ord(cand_w[p]);
  if (S == 0) {
    atomicMin(bw + c, w);
    return;
  }
  if (w != bw[c]) return;
  const hd_u64 m = hd_ord(cand_m[p]);
  if (S == 1) {
    atomicMin(bm + c, m);
    return;
  }
  if (m != bm[c]) return;
  const hd_u64 lo = (hd_u64)(i < j ? i : j), hi = (hd_u64)(i < j ? j : i);
  atomicMin(be + c, (lo << 32) | hi);
}

__global__ __launch_bounds__(256) void hd_hook_kernel(const int* __restrict__ comp, const hd_u64* __restrict__ bw,
                                                      const hd_u64* __restrict__ bm, const hd_u64* __restrict__ be,
                                                      int* __restrict__ parent, int n, int* cursor,
                                                      int* __restrict__ ei, int* __restrict__ ej,
                                                      double* __restrict__ ew, double* __restrict__ em) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n || comp[c] != c) return;                                // roots only
  const hd_u64 e = be[c];
  if (e == HD_NONE) return;
  const int lo = (int)(e >> 32), hi = (int)(e & 0xFFFFFFFFull);
  if (lo < 0 || lo >= n || hi < 0 || hi >= n) return;
  const int a = comp[lo], b = comp[hi];
  const int other = a == c ? b : a;
  if (be[other] == e && c < other) return;                           // a mutual pick: the smaller id stays the root
  parent[c] = other;
  const int pos = atomicAdd(cursor, 1);
  if (pos < n - 1) {
    ei[pos] = lo;
    ej[pos] = hi;
    ew[pos] = hd_unord(bw[c]);
    em[pos] = hd_unord(bm[c]);
  }
}

__global__ __launch_bounds__(256) void hd_jump_kernel(int* parent, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = parent[i];
  const int pp = parent[p];                                          // either value a racing write leaves is an ancestor
  if (pp != p) parent[i] = pp;
}

// a wave per 64-row block
__global__ __launch_bounds__(256) void hd_relabel_kernel(int* __restrict__ comp, const int* __restrict__ parent,
                                                         int2* __restrict__ brange, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int c = -1;
  if (i < n) {
    c = parent[comp[i]];
    comp[i] = c;
  }
  int lo = c < 0 ? INT_MAX : c, hi = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63) == 0 && i < n) brange[i / SQD_T] = make_int2(lo, hi);
}

// ---- host: the device driver ---------------------------------------------------------------------------------------------
static inline bool hd_shape_ok(int n, int d) { return n >= 2 && n <= HD_MAX_N && d >= 1 && d <= HD_MAX_D; }

static inline int hd_ceil_log2(int x) {
  int r = 0;
  while (((int64_t)1 << r) < x) ++r;
  return r;
}

static inline int hd_segs(int n) {
  const int tiles = ceil_div(n, SQD_T);
  int s = 4096 / tiles;
  if (s > HD_MAX_SEG) s = HD_MAX_SEG;
  if (s > tiles) s = tiles;
  return s < 1 ? 1 : s;
}

struct hd_ws {
  int *comp, *parent, *cand_j, *cursor;
  int2* brange;
  hd_u64 *bw, *bm, *be;
  double *cand_w, *cand_m;
};
static size_t hd_ws_layout(int n, void* base, hd_ws* out) {
  const size_t segs = hd_segs(n), tiles = ceil_div(n, SQD_T);
  ava_ws_cursor c(base);
  hd_ws w;
  w.comp = c.take<int>(n);
  w.parent = c.take<int>(n);
  w.cand_j = c.take<int>(segs * n);
  w.cursor = c.take<int>(1);
  w.brange = c.take<int2>(tiles);
  w.bw = c.take<hd_u64>(n);
  w.bm = c.take<hd_u64>(n);
  w.be = c.take<hd_u64>(n);
  w.cand_w = c.take<double>(segs * n);
  w.cand_m = c.take<double>(segs * n);
  if (out) *out = w;
  return c.bytes();
}

extern "C" size_t ava_hd_workspace_bytes(int n, int d) {
  if (!hd_shape_ok(n, d)) return 0;
  return hd_ws_layout(n, nullptr, nullptr);
}

extern "C" int ava_hd_core(const void* x, int dtype, int n, int d, const int64_t* kth, double* core, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !hd_shape_ok(n, d) || !kth || !core) return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  const dim3 grid(ceil_div(n, 256));
  if (dtype == 0)
    hipLaunchKernelGGL(hd_core_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), n, d, kth, core);
  else
    hipLaunchKernelGGL(hd_core_kernel<double>, grid, dim3(256), 0, st, static_cast<const double*>(x), n, d, kth, core);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_hd_core_pre(const void* dist, int dtype, int n, int k, double* core, ava_stream_t s) {
  if (!dist || (dtype != 0 && dtype != 1) || !hd_shape_ok(n, 1) || k < 1 || k > HD_MAX_K || k > n || !core)
    return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  if (dtype == 0)
    hipLaunchKernelGGL(hd_core_pre_kernel<float>, dim3(n), dim3(256), 0, st, static_cast<const float*>(dist), n, k, core);
  else
    hipLaunchKernelGGL(hd_core_pre_kernel<double>, dim3(n), dim3(256), 0, st, static_cast<const double*>(dist), n, k,
                       core);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename T, bool PRE>
static int hd_mst_typed(const void* x, int n, int d, const double* core, int* ei, int* ej, double* ew, double* em,
                        int* rounds, float* rowmin_ms, const hd_ws& w, hipStream_t st) {
  const T* X = static_cast<const T*>(x);
  const int tiles = ceil_div(n, SQD_T), segs = hd_segs(n), per_seg = ceil_div(tiles, segs);
  const dim3 rows(ceil_div(n, 256)), thr(256);
  const dim3 cands((unsigned)ceil_div64((int64_t)n * segs, 256));
  const int max_rounds = hd_ceil_log2(n);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (rowmin_ms && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) return AVA_ELAUNCH;
  int rc = AVA_OK, ncomp = n, done = 0;
  hipLaunchKernelGGL(hd_start_kernel, rows, thr, 0, st, w.comp, w.brange, n, w.cursor);
  while (rc == AVA_OK && ncomp > 1) {
    if (done >= max_rounds) {                                        // cannot happen: every round halves the components
      rc = AVA_ELAUNCH;
      break;
    }
    hipLaunchKernelGGL(hd_round_init_kernel, rows, thr, 0, st, w.bw, w.bm, w.be, w.parent, n);
    if (rowmin_ms && hipEventRecord(ev0, st) != hipSuccess) rc = AVA_ELAUNCH;
    hipLaunchKernelGGL((hd_rowmin_kernel<T, PRE>), dim3(tiles, segs), thr, 0, st, X, n, d, tiles, per_seg, core, w.comp,
                       w.brange, w.cand_w, w.cand_m, w.cand_j);
    if (rowmin_ms && hipEventRecord(ev1, st) != hipSuccess) rc = AVA_ELAUNCH;
    hipLaunchKernelGGL(hd_compmin_kernel<0>, cands, thr, 0, st, w.cand_w, w.cand_m, w.cand_j, w.comp, n, segs, w.bw, w.bm,
                       w.be);
    hipLaunchKernelGGL(hd_compmin_kernel<1>, cands, thr, 0, st, w.cand_w, w.cand_m, w.cand_j, w.comp, n, segs, w.bw, w.bm,
                       w.be);
    hipLaunchKernelGGL(hd_compmin_kernel<2>, cands, thr, 0, st, w.cand_w, w.cand_m, w.cand_j, w.comp, n, segs, w.bw, w.bm,
                       w.be);
    hipLaunchKernelGGL(hd_hook_kernel, rows, thr, 0, st, w.comp, w.bw, w.bm, w.be, w.parent, n, w.cursor, ei, ej, ew, em);
    int edges = 0;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&edges, w.cursor, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      rc = AVA_ELAUNCH;
      break;
    }
    if (rowmin_ms && hipEventElapsedTime(rowmin_ms + done, ev0, ev1) != hipSuccess) rowmin_ms[done] = -1.0f;
    const int left = n - edges;
    if (left < 1 || 2 * left > ncomp) {                              // every component must have found an edge
      rc = AVA_ELAUNCH;
      break;
    }
    for (int it = hd_ceil_log2(ncomp) + 1; it > 0; --it) hipLaunchKernelGGL(hd_jump_kernel, rows, thr, 0, st, w.parent, n);
    hipLaunchKernelGGL(hd_relabel_kernel, rows, thr, 0, st, w.comp, w.parent, w.brange, n);
    if (hipGetLastError() != hipSuccess) rc = AVA_ELAUNCH;
    ncomp = left;
    ++done;
  }
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  if (rc == AVA_OK && hipStreamSynchronize(st) != hipSuccess) rc = AVA_ELAUNCH;
  *rounds = done;
  return rc;
}

static int hd_mst(bool pre, const void* x, int dtype, int n, int d, const double* core, int* ei, int* ej, double* ew,
                  double* em, int* rounds, float* rowmin_ms, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !hd_shape_ok(n, d) || !core || !ei || !ej || !ew || !em || !rounds || !ws)
    return AVA_EINVAL;
  if (ws_bytes < ava_hd_workspace_bytes(n, d)) return AVA_EWORKSPACE;
  hd_ws w;
  hd_ws_layout(n, ws, &w);
  hipStream_t st = to_stream(s);
  if (pre)
    return dtype == 0 ? hd_mst_typed<float, true>(x, n, d, core, ei, ej, ew, em, rounds, rowmin_ms, w, st)
                      : hd_mst_typed<double, true>(x, n, d, core, ei, ej, ew, em, rounds, rowmin_ms, w, st);
  return dtype == 0 ? hd_mst_typed<float, false>(x, n, d, core, ei, ej, ew, em, rounds, rowmin_ms, w, st)
                    : hd_mst_typed<double, false>(x, n, d, core, ei, ej, ew, em, rounds, rowmin_ms, w, st);
}

extern "C" int ava_hd_max_rounds(int n) { return n >= 2 && n <= HD_MAX_N ? hd_ceil_log2(n) : 0; }

extern "C" int ava_hd_mst(const void* x, int dtype, int n, int d, const double* core, int* ei, int* ej, double* ew,
                          double* em, int* rounds, float* rowmin_ms, void* ws, size_t ws_bytes, ava_stream_t s) {
  return hd_mst(false, x, dtype, n, d, core, ei, ej, ew, em, rounds, rowmin_ms, ws, ws_bytes, s);
}

extern "C" int ava_hd_mst_pre(const void* dist, int dtype, int n, const double* core, int* ei, int* ej, double* ew,
                              double* em, int* rounds, float* rowmin_ms, void* ws, size_t ws_bytes, ava_stream_t s) {
  return hd_mst(true, dist, dtype, n, 1, core, ei, ej, ew, em, rounds, rowmin_ms, ws, ws_bytes, s);
}

// ---- host: the tree tail (no HIP call) -----------------------------------------------------------------------------------
static inline int hd_find(std::vector<int>& up, int x) {
  int r = x;
  while (up[r] >= 0) r = up[r];
  while (up[x] >= 0) {
    const int nx = up[x];
    up[x] = r;
    x = nx;
  }
  return r;
}

extern "C" int ava_hd_tree(const int64_t* ei, const int64_t* ej, const double* dist, int n, int min_cluster_size,
                           int method, int64_t* labels, double* prob, int* n_clusters, double* linkage) {
  if (!ei || !ej || !dist || !labels || !prob || !n_clusters || !linkage) return AVA_EINVAL;
  if (n < 2 || n > HD_MAX_N || min_cluster_size < 2 || (method != 0 && method != 1)) return AVA_EINVAL;
  const int m = n - 1, root = 2 * m;
  // make_single_linkage: node n + e is the union of the clusters of edge e's two rows
  std::vector<int> up(2 * n - 1, -1), size(2 * n - 1, 1), left(m), right(m);
  for (int e = 0; e < m; ++e) {
    if (ei[e] < 0 || ei[e] >= n || ej[e] < 0 || ej[e] >= n || dist[e] != dist[e]) return AVA_EINVAL;
    const int a = hd_find(up, (int)ei[e]), b = hd_find(up, (int)ej[e]);
    if (a == b) return AVA_EINVAL;                                   // not a spanning tree
    left[e] = a;
    right[e] = b;
    up[a] = up[b] = n + e;
    size[n + e] = size[a] + size[b];
    linkage[4 * (size_t)e] = a;
    linkage[4 * (size_t)e + 1] = b;
    linkage[4 * (size_t)e + 2] = dist[e];
    linkage[4 * (size_t)e + 3] = size[n + e];
  }
  // _condense_tree: breadth first from the root; cp / cc / cl / cs are the condensed tree's columns
  std::vector<int> order, sub, relabel(2 * n - 1, 0), cp, cc, cs;
  std::vector<double> cl;
  std::vector<char> ignore(2 * n - 1, 0);
  order.reserve(2 * n - 1);
  order.push_back(root);
  for (size_t q = 0; q < order.size(); ++q)
    if (order[q] >= n) {
      order.push_back(left[order[q] - n]);
      order.push_back(right[order[q] - n]);
    }
  relabel[root] = n;
  int next_label = n + 1;
  auto add = [&](int parent, int child, double lambda, int count) {
    cp.push_back(parent);
    cc.push_back(child);
    cl.push_back(lambda);
    cs.push_back(count);
  };
  auto shed = [&](int start, int parent, double lambda) {             // every row below `start` leaves `parent`
    sub.clear();
    sub.push_back(start);
    for (size_t q = 0; q < sub.size(); ++q) {
      const int v = sub[q];
      if (v < n) {
        add(parent, v, lambda, 1);
      } else {
        sub.push_back(left[v - n]);
        sub.push_back(right[v - n]);
      }
      ignore[v] = 1;
    }
  };
  for (size_t q = 0; q < order.size(); ++q) {
    const int node = order[q];
    if (ignore[node] || node < n) continue;
    const int l = left[node - n], r = right[node - n];
    const double distance = dist[node - n];
    const double lambda = distance > 0.0 ? 1.0 / distance : INFINITY;
    const int lc = size[l], rcnt = size[r];
    if (lc >= min_cluster_size && rcnt >= min_cluster_size) {
      relabel[l] = next_label++;
      add(relabel[node], relabel[l], lambda, lc);
      relabel[r] = next_label++;
      add(relabel[node], relabel[r], lambda, rcnt);
    } else if (lc < min_cluster_size && rcnt < min_cluster_size) {
      shed(l, relabel[node], lambda);
      shed(r, relabel[node], lambda);
    } else if (lc < min_cluster_size) {
      relabel[r] = relabel[node];
      shed(l, relabel[node], lambda);
    } else {
      relabel[l] = relabel[node];
      shed(r, relabel[node], lambda);
    }
  }
  const size_t rows = cp.size();
  const int ncl = next_label - n;                                    // condensed clusters n .. next_label - 1, n the root
  // _compute_stability
  std::vector<double> births(next_label, NAN), stab(ncl, 0.0);
  for (size_t q = 0; q < rows; ++q) births[cc[q]] = cl[q];
  births[n] = 0.0;
  for (size_t q = 0; q < rows; ++q) stab[cp[q] - n] += (cl[q] - births[cp[q]]) * cs[q];
  // the cluster tree
  std::vector<int> cpar(ncl, -1), kid0(ncl, -1), kid1(ncl, -1);
  for (size_t q = 0; q < rows; ++q)
    if (cs[q] > 1) {
      const int c = cc[q] - n, p = cp[q] - n;
      cpar[c] = p;
      (kid0[p] < 0 ? kid0[p] : kid1[p]) = c;
    }
  // _get_clusters
  std::vector<char> sel(ncl, 0);
  if (method == 0) {
    std::vector<char> keep(ncl, 0), under(ncl, 0);
    for (int c = ncl - 1; c >= 1; --c) {
      double below = 0.0;
      if (kid0[c] >= 0) below = stab[kid0[c]];
      if (kid1[c] >= 0) below = below + stab[kid1[c]];
      if (below > stab[c])
        stab[c] = below;
      else
        keep[c] = 1;
    }
    for (int c = 1; c < ncl; ++c) {                                  // a kept cluster unselects everything below it
      const int p = cpar[c];
      under[c] = p > 0 && (under[p] || keep[p]);
      sel[c] = keep[c] && !under[c];
    }
  } else {
    for (int c = 1; c < ncl; ++c) sel[c] = kid0[c] < 0;
  }
  // _do_labelling: a row belongs to the nearest selected cluster at or above the one it left; the root is noise
  std::vector<int> top(ncl, 0);
  for (int c = 1; c < ncl; ++c) top[c] = sel[c] ? c : top[cpar[c]];
  // max_lambdas: the largest lambda of the LAST run of consecutive rows of a parent, as sklearn computes it
  std::vector<double> deaths(next_label, 0.0);
  if (rows) {
    int current = cp[0];
    double max_lambda = cl[0];
    for (size_t q = 1; q < rows; ++q) {
      if (cp[q] == current) {
        max_lambda = max_lambda > cl[q] ? max_lambda : cl[q];
      } else {
        deaths[current] = max_lambda;
        current = cp[q];
        max_lambda = cl[q];
      }
    }
    deaths[current] = max_lambda;
  }
  std::vector<int> of(n, 0);                                         // the selected cluster of a row, 0: noise
  for (int i = 0; i < n; ++i) prob[i] = 0.0;
  for (size_t q = 0; q < rows; ++q) {
    if (cc[q] >= n) continue;
    const int c = top[cp[q] - n];
    of[cc[q]] = c;
    if (c == 0) continue;
    const double max_lambda = deaths[c + n];
    if (max_lambda == 0.0 || isinf(cl[q]))
      prob[cc[q]] = 1.0;
    else
      prob[cc[q]] = (cl[q] < max_lambda ? cl[q] : max_lambda) / max_lambda;
  }
  // clusters in ascending order of their smallest row
  std::vector<int> number(ncl, -1);
  int count = 0;
  for (int i = 0; i < n; ++i) {
    const int c = of[i];
    if (c == 0) {
      labels[i] = -1;
      continue;
    }
    if (number[c] < 0) number[c] = count++;
    labels[i] = number[c];
  }
  *n_clusters = count;
  return AVA_OK;
}
