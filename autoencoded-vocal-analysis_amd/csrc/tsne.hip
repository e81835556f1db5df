// Exact t-SNE of latent means or of a precomputed distance matrix: the device
// counterpart of scikit-learn 1.7's TSNE(method='exact', n_components=2), which the reference's mmd_tsne_plot_DC
// (ava/plotting/mmd_plots.py:171-252) calls on the MMD^2 matrix.  Everything is fp64; nothing uses atomics; the same
// inputs give the same bits on every run.
//
// Storage: the N x N matrix (squared distances, then conditional, then joint probabilities, each overwriting the one
// before) is row-major with a row stride ld >= N, ld even, on a 16-byte boundary, so every row starts on one and the
// row kernels read it as double2.  Column N of an odd N is padding: read, never used.
//
// 1. squared distances   ts_sqdist_kernel: the 64 x 64 tile of sqdist_tile.h under its order contract (the bits of
//                        ava_pair_sqdist); ts_square_kernel: d^2 of an uploaded distance matrix.  Both round to the
//                        nearest float32 and store that as fp64 (sklearn's distances.astype(np.float32)).
// 2. conditional P       ts_perplexity_kernel: a workgroup per row runs sklearn's _binary_search_perplexity (beta from
//                        1, at most 100 steps, the .pyx's float constants and its float desired_perplexity), reading
//                        the row from global memory (L2) at every step, and overwrites the row.
// 3. joint P, in place   ts_joint_sum_kernel -> ts_sum_kernel -> ts_joint_write_kernel: S = sum_ij (C_ij + C_ji), then
//                        P_ij = max((C_ij + C_ji) / max(S, eps), eps), P_ii = 0.  A workgroup owns tile (ti, tj),
//                        ti <= tj, and its mirror.
// 4. one descent iteration, three launches:
//      ts_z_kernel       Z = sum_{i != j} 1 / (1 + |y_i - y_j|^2), per (row tile, column chunk) partials
//      ts_grad_kernel    with Z: the partial gradient of every row over the chunk's columns and the chunk's share of
//                        the KL divergence; streams P once (16-byte loads; y_j of the lane's two columns stay in
//                        registers over the 8 rows of the wave, y_i of the tile's rows in LDS)
//      ts_update_kernel  sums the partials, applies sklearn's gains / momentum rule, writes {KL, |grad gains|}
//    The KL is computed in the last iteration of a call only (the one sklearn's checks read); the others report NaN.
//
// Orders of the sums (all fixed; "workgroup sum" = each thread's own terms in the order given, the xor butterfly of
// wave_sum_d over the 64 lanes, then the waves in ascending order):
//   * a row's sum_Pi and sum_j d_ij P_ij: thread t takes the column pairs t, t + 256, ... ascending; workgroup sum.
//   * S: per tile pair a workgroup sum of the thread's 4 x 4 entries (r, then c ascending), doubled for ti < tj; the
//     partials (tile pairs in grid order, 0 below the diagonal) by ts_sum_kernel: thread t takes t, t + 1024, ...;
//     workgroup sum.
//   * Z: per workgroup, lane l of wave w takes columns c0 + 2 l + 128 s (+ 1), s ascending, and for each the rows
//     8 w .. 8 w + 7 of the 32-row tile ascending; workgroup sum.  Then every workgroup of ts_grad_kernel sums the
//     partials: thread t takes t, t + 256, ...; workgroup sum (the same bits in every workgroup).
//   * gradient of row i: per chunk, lane l's columns ascending as for Z, the butterfly over the lanes; the chunks in
//     ascending order (ts_update_kernel); then times 4.
//   * KL: per workgroup as for Z (rows inside columns); the partials (chunk-major) and the squared gradient norm:
//     thread t of 1024 takes t, t + 1024, ...; workgroup sum.
// The number of column chunks decides which terms meet in which partial, so it changes the last bits of Z, the gradient
// and the KL; it is a function of N alone (ava_ts_col_chunks) unless the caller passes one.
#include <float.h>
#include <math.h>

#include "common.h"
#include "sqdist_tile.h"

#define TS_T SQD_T                 // rows of a tile of the distance and joint-probability kernels
#define TS_WROWS 8                 // descent kernels: rows of a wave
#define TS_GT (4 * TS_WROWS)       // descent kernels: rows of a workgroup
#define TS_STEP 128                // columns of a wave step: 64 lanes x double2
#define TS_BLD 65                  // row stride of the mirror tile in LDS (odd: transposed reads spread over the banks)
#define TS_MAX_N 32768
#define TS_MAX_CHUNKS 64
#define TS_SEARCH_STEPS 100

// workgroup sum of two values (order: see the header); valid in every thread.  red: 2 x 16 doubles of LDS
__device__ __forceinline__ void ts_block_sum2(double& a, double& b, double* red) {
  const int t = threadIdx.x, nw = blockDim.x >> 6;
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  __syncthreads();                                   // the previous use of red is over
  if ((t & 63) == 0) {
    red[t >> 6] = a;
    red[16 + (t >> 6)] = b;
  }
  __syncthreads();
  a = red[0];
  b = red[16];
  for (int w = 1; w < nw; ++w) {
    a += red[w];
    b += red[16 + w];
  }
}

__device__ __forceinline__ double ts_block_sum(double a, double* red) {
  double b = 0.0;
  ts_block_sum2(a, b, red);
  return a;
}

__device__ __forceinline__ double ts_round_f32(double v) { return (double)(float)v; }

// ---- 1. squared distances -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void ts_sqdist_kernel(const T* __restrict__ X, int n, int d, int round_f32,
                                                        double* __restrict__ out, int ld) {
  __shared__ double stage[2 * SQD_T * SQD_LD];
  double* xs = stage;
  double* ys = stage + SQD_T * SQD_LD;
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int i0 = blockIdx.y * SQD_T, j0 = blockIdx.x * SQD_T;
  double acc[4][4];
  sqd_tile(xs, ys, X, i0, n, X, j0, n, d, t, acc);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gi = i0 + ty + 16 * i, gj = j0 + tx + 16 * j;
      if (gi < n && gj < n) out[(size_t)gi * ld + gj] = round_f32 ? ts_round_f32(acc[i][j]) : acc[i][j];
    }
}

// out[i][j] = float32(dist[i][j]^2); dist [n][n] contiguous
__global__ __launch_bounds__(256) void ts_square_kernel(const double* __restrict__ dist, int n,
                                                        double* __restrict__ out, int ld) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * n) return;
  const int i = (int)(e / n), j = (int)(e - (int64_t)i * n);
  const double v = dist[e];
  out[(size_t)i * ld + j] = ts_round_f32(v * v);
}

// ---- 2. conditional probabilities -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ts_perplexity_kernel(double* __restrict__ P, int ld, int n,
                                                            double desired_entropy) {
  __shared__ double red[32];
  const int t = threadIdx.x, i = blockIdx.x;
  double2* row = reinterpret_cast<double2*>(P + (size_t)i * ld);
  const int n2 = (n + 1) >> 1;
  const double eps = (double)1e-8f, tol = (double)1e-5f;          // C floats in sklearn's _utils.pyx
  double beta = 1.0, bmin = -INFINITY, bmax = INFINITY, beta_used = 1.0, sum_pi = 1.0;
  for (int step = 0; step < TS_SEARCH_STEPS; ++step) {
    double s1 = 0.0, s2 = 0.0;
    for (int c2 = t; c2 < n2; c2 += 256) {
      const double2 dv = row[c2];
      const int c = 2 * c2;
      const double e0 = c != i ? exp(-dv.x * beta) : 0.0;
      const double e1 = (c + 1 < n && c + 1 != i) ? exp(-dv.y * beta) : 0.0;
      s1 += e0;
      s2 += dv.x * e0;
      s1 += e1;
      s2 += (c + 1 < n ? dv.y : 0.0) * e1;
    }
    ts_block_sum2(s1, s2, red);
    if (s1 == 0.0) s1 = eps;
    sum_pi = s1;
    beta_used = beta;
    const double diff = log(s1) + beta * (s2 / s1) - desired_entropy;
    if (fabs(diff) <= tol) break;                    // the same bits in every thread: uniform
    if (diff > 0.0) {
      bmin = beta;
      beta = bmax == INFINITY ? beta * 2.0 : (beta + bmax) / 2.0;
    } else {
      bmax = beta;
      beta = bmin == -INFINITY ? beta / 2.0 : (beta + bmin) / 2.0;
    }
  }
  for (int c2 = t; c2 < n2; c2 += 256) {
    const double2 dv = row[c2];
    const int c = 2 * c2;
    double2 o;
    o.x = c != i ? exp(-dv.x * beta_used) / sum_pi : 0.0;
    o.y = (c + 1 < n && c + 1 != i) ? exp(-dv.y * beta_used) / sum_pi : 0.0;
    row[c2] = o;
  }
}

// ---- 3. joint probabilities -----------------------------------------------------------------------------------------
// a[r][c] = C[ti 64 + ty + 16 r][tj 64 + tx + 16 c]; B[r'][c'] = C[tj 64 + r'][ti 64 + c'] (LDS, stride TS_BLD); entries
// that do not exist are 0.  Ends with a barrier: every global read of the two tiles precedes it.
__device__ __forceinline__ void ts_joint_load(const double* __restrict__ C, int ld, int n, int ti, int tj, int ty,
                                              int tx, double (&a)[4][4], double* B) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int lr = ty + 16 * r, lc = tx + 16 * c;
      const int gi = ti * TS_T + lr, gj = tj * TS_T + lc;
      a[r][c] = (gi < n && gj < n) ? C[(size_t)gi * ld + gj] : 0.0;
      const int mi = tj * TS_T + lr, mj = ti * TS_T + lc;
      B[lr * TS_BLD + lc] = (mi < n && mj < n) ? C[(size_t)mi * ld + mj] : 0.0;
    }
  __syncthreads();
}

__global__ __launch_bounds__(256) void ts_joint_sum_kernel(const double* __restrict__ C, int ld, int n,
                                                           double* __restrict__ partials) {
  __shared__ double B[TS_T * TS_BLD];
  __shared__ double red[32];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int ti = blockIdx.y, tj = blockIdx.x;
  const size_t slot = (size_t)ti * gridDim.x + tj;
  if (tj < ti) {                                     // the mirror of a tile above the diagonal
    if (t == 0) partials[slot] = 0.0;
    return;
  }
  double a[4][4];
  ts_joint_load(C, ld, n, ti, tj, ty, tx, a, B);
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) s += a[r][c] + B[(tx + 16 * c) * TS_BLD + ty + 16 * r];
  s = ts_block_sum(s, red);
  if (t == 0) partials[slot] = ti < tj ? 2.0 * s : s;
}

// out[0] = sum of v[0 .. count): one workgroup of 1024
__global__ __launch_bounds__(1024) void ts_sum_kernel(const double* __restrict__ v, int64_t count,
                                                      double* __restrict__ out) {
  __shared__ double red[32];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 1024) s += v[i];
  s = ts_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__(256) void ts_joint_write_kernel(double* __restrict__ C, int ld, int n,
                                                             const double* __restrict__ S) {
  __shared__ double B[TS_T * TS_BLD];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  double a[4][4];
  ts_joint_load(C, ld, n, ti, tj, ty, tx, a, B);
  const double sum_p = fmax(S[0], DBL_EPSILON);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int gi = ti * TS_T + ty + 16 * r, gj = tj * TS_T + tx + 16 * c;
      const double v = fmax((a[r][c] + B[(tx + 16 * c) * TS_BLD + ty + 16 * r]) / sum_p, DBL_EPSILON);
      a[r][c] = gi == gj ? 0.0 : v;
      if (gi < n && gj < n) C[(size_t)gi * ld + gj] = a[r][c];
    }
  if (ti == tj) return;                              // uniform
  __syncthreads();                                   // B read by everyone
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) B[(tx + 16 * c) * TS_BLD + ty + 16 * r] = a[r][c];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int lr = ty + 16 * r, lc = tx + 16 * c;
      const int mi = tj * TS_T + lr, mj = ti * TS_T + lc;
      if (mi < n && mj < n) C[(size_t)mi * ld + mj] = B[lr * TS_BLD + lc];
    }
}

// ---- 4. descent -----------------------------------------------------------------------------------------------------
// grid (row tiles, column chunks); chunk b owns the columns [b cw, min((b + 1) cw, n)), cw even
__global__ __launch_bounds__(256) void ts_z_kernel(const double2* __restrict__ Y, int n, int cw,
                                                   double* __restrict__ zpart) {
  __shared__ double2 yi[TS_GT];
  __shared__ double red[32];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int r0 = blockIdx.x * TS_GT;
  const int c0 = blockIdx.y * cw, c1 = min(c0 + cw, n);
  if (t < TS_GT) yi[t] = Y[min(r0 + t, n - 1)];
  __syncthreads();
  double s = 0.0;
  for (int cb = c0; cb < c1; cb += TS_STEP) {
    const int c = cb + 2 * l;
    const double2 ya = Y[min(c, n - 1)], yb = Y[min(c + 1, n - 1)];
#pragma unroll
    for (int r = 0; r < TS_WROWS; ++r) {
      const int row = r0 + w * TS_WROWS + r;
      const double2 yr = yi[w * TS_WROWS + r];
      const double ax = yr.x - ya.x, ay = yr.y - ya.y, bx = yr.x - yb.x, by = yr.y - yb.y;
      const double w0 = 1.0 / (1.0 + (ax * ax + ay * ay)), w1 = 1.0 / (1.0 + (bx * bx + by * by));
      s += (row < n && c < c1 && c != row) ? w0 : 0.0;
      s += (row < n && c + 1 < c1 && c + 1 != row) ? w1 : 0.0;
    }
  }
  s = ts_block_sum(s, red);
  if (t == 0) zpart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// gpart [chunks][n][2]: sum over the chunk's columns j of (e P_ij - Q_ij) w_ij (y_i - y_j); with KL, klpart [chunks][row
// tiles]: the workgroup's sum of e P_ij log(max(e P_ij, eps) / Q_ij) (a division and a logarithm per pair, more than the
// rest of the pass together: only the iterations whose KL the host may read pay for it, as sklearn's compute_error).
// The diagonal needs no case of its own: P_ii = 0 and y_i - y_i = 0.
template <bool KL>
__global__ __launch_bounds__(256) void ts_grad_kernel(const double2* __restrict__ Y, const double* __restrict__ P,
                                                      int ld, int n, int cw, const double* __restrict__ zpart,
                                                      int nz, double e, double* __restrict__ gpart,
                                                      double* __restrict__ klpart) {
  __shared__ double2 yi[TS_GT];
  __shared__ double red[32];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int r0 = blockIdx.x * TS_GT;
  const int c0 = blockIdx.y * cw, c1 = min(c0 + cw, n);
  if (t < TS_GT) yi[t] = Y[min(r0 + t, n - 1)];
  double z = 0.0;
  for (int i = t; i < nz; i += 256) z += zpart[i];
  z = ts_block_sum(z, red);                          // also the barrier behind yi
  const double inv_z = 1.0 / z;
  double gx[TS_WROWS], gy[TS_WROWS];
#pragma unroll
  for (int r = 0; r < TS_WROWS; ++r) gx[r] = gy[r] = 0.0;
  double kl = 0.0;
  for (int cb = c0; cb < c1; cb += TS_STEP) {
    const int c = cb + 2 * l;
    const bool ok0 = c < c1, ok1 = c + 1 < c1;
    const int cl = ok0 ? c : c0;                     // an idle lane reads the chunk's first pair
    const double2 ya = Y[min(c, n - 1)], yb = Y[min(c + 1, n - 1)];
    double2 p[TS_WROWS];
#pragma unroll
    for (int r = 0; r < TS_WROWS; ++r) {
      const int row = min(r0 + w * TS_WROWS + r, n - 1);
      p[r] = *reinterpret_cast<const double2*>(P + (size_t)row * ld + cl);
    }
#pragma unroll
    for (int r = 0; r < TS_WROWS; ++r) {
      const bool rok = r0 + w * TS_WROWS + r < n;
      const double2 yr = yi[w * TS_WROWS + r];
      const double ax = yr.x - ya.x, ay = yr.y - ya.y, bx = yr.x - yb.x, by = yr.y - yb.y;
      const double w0 = ok0 ? 1.0 / (1.0 + (ax * ax + ay * ay)) : 0.0;
      const double w1 = ok1 ? 1.0 / (1.0 + (bx * bx + by * by)) : 0.0;
      const double p0 = ok0 ? e * p[r].x : 0.0, p1 = ok1 ? e * p[r].y : 0.0;
      const double q0 = fmax(w0 * inv_z, DBL_EPSILON), q1 = fmax(w1 * inv_z, DBL_EPSILON);
      const double m0 = (p0 - q0) * w0, m1 = (p1 - q1) * w1;
      gx[r] += m0 * ax;
      gy[r] += m0 * ay;
      gx[r] += m1 * bx;
      gy[r] += m1 * by;
      if (KL) {
        const double k0 = p0 * log(fmax(p0, DBL_EPSILON) / q0), k1 = p1 * log(fmax(p1, DBL_EPSILON) / q1);
        kl += rok ? k0 : 0.0;
        kl += rok ? k1 : 0.0;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < TS_WROWS; ++r) {
    const int row = r0 + w * TS_WROWS + r;
    const double sx = wave_sum_d(gx[r]), sy = wave_sum_d(gy[r]);
    if (l == 0 && row < n) {
      double2 o;
      o.x = sx;
      o.y = sy;
      reinterpret_cast<double2*>(gpart)[(size_t)blockIdx.y * n + row] = o;
    }
  }
  if (KL) {
    kl = ts_block_sum(kl, red);
    if (t == 0) klpart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = kl;
  }
}

// One workgroup of 1024 over the 2 n coordinates: grad = 4 x the chunks' partials in ascending order (written to
// grad_out when given); with y given, sklearn's step: inc = update grad < 0; gains += 0.2 where inc, else *= 0.8; gains
// = max(gains, 0.01); grad *= gains; update = momentum update - lr grad; y += update.  stats = {KL, |grad|_2}, the norm
// of the gradient as it stands (times gains after a step, as sklearn's check takes it); nkl < 0: the KL was not computed
// and is reported as NaN, like sklearn's compute_error=False.
__global__ __launch_bounds__(1024) void ts_update_kernel(const double* __restrict__ gpart, const double* __restrict__ klpart,
                                                         int n, int chunks, int nkl, double momentum, double lr,
                                                         double* __restrict__ y, double* __restrict__ update,
                                                         double* __restrict__ gains, double* __restrict__ grad_out,
                                                         double* __restrict__ stats) {
  __shared__ double red[32];
  const int t = threadIdx.x;
  double nrm = 0.0, kl = 0.0;
#pragma unroll 4
  for (int i = t; i < 2 * n; i += 1024) {
    double g = gpart[i];
    for (int c = 1; c < chunks; ++c) g += gpart[(size_t)c * 2 * n + i];
    g *= 4.0;
    if (grad_out) grad_out[i] = g;
    if (y) {
      const double u = update[i];
      double ga = gains[i];
      ga = u * g < 0.0 ? ga + 0.2 : ga * 0.8;
      ga = fmax(ga, 0.01);
      g *= ga;
      const double un = momentum * u - lr * g;
      gains[i] = ga;
      update[i] = un;
      y[i] += un;
    }
    nrm += g * g;
  }
  for (int i = t; i < nkl; i += 1024) kl += klpart[i];
  ts_block_sum2(kl, nrm, red);
  if (t == 0) {
    stats[0] = nkl < 0 ? NAN : kl;
    stats[1] = sqrt(nrm);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
static inline int ts_tiles(int n) { return ceil_div(n, TS_T); }
static inline int ts_row_tiles(int n) { return ceil_div(n, TS_GT); }
static inline int ts_chunk_width(int n, int chunks) { return 2 * ceil_div(n, 2 * chunks); }
static inline bool ts_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool ts_matrix_ok(const void* p, int ld, int n) {
  return p && ts_aligned16(p) && n >= 2 && n <= TS_MAX_N && ld >= n && (ld & 1) == 0;
}

extern "C" int ava_ts_max_n(void) { return TS_MAX_N; }

// about 1024 workgroups for the gradient pass, none narrower than 512 columns, at most 32 chunks
extern "C" int ava_ts_col_chunks(int n) {
  if (n < 2 || n > TS_MAX_N) return 0;
  int c = 1024 / ts_row_tiles(n);
  if (c > n / 512) c = n / 512;
  if (c > 32) c = 32;
  return c < 1 ? 1 : c;
}

static size_t ts_descent_doubles(int n, int chunks) {
  return (size_t)2 * ts_row_tiles(n) * chunks + (size_t)chunks * n * 2;
}

extern "C" size_t ava_ts_workspace_bytes(int n, int col_chunks) {
  if (n < 2 || n > TS_MAX_N) return 0;
  if (col_chunks <= 0) col_chunks = ava_ts_col_chunks(n);
  if (col_chunks > TS_MAX_CHUNKS) return 0;
  const size_t joint = (size_t)ts_tiles(n) * ts_tiles(n) + 2;
  const size_t descent = ts_descent_doubles(n, col_chunks);
  return ava_up256((joint > descent ? joint : descent) * sizeof(double)) + 256;
}

extern "C" int ava_ts_sqdist(const void* x, int dtype, int n, int d, int round_f32, double* out, int ld,
                             ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || d < 1 || d > 65536 || !ts_matrix_ok(out, ld, n)) return AVA_EINVAL;
  const dim3 grid(ts_tiles(n), ts_tiles(n));
  if (dtype == 0)
    hipLaunchKernelGGL(ts_sqdist_kernel<float>, grid, dim3(256), 0, to_stream(s), static_cast<const float*>(x), n, d,
                       round_f32, out, ld);
  else
    hipLaunchKernelGGL(ts_sqdist_kernel<double>, grid, dim3(256), 0, to_stream(s), static_cast<const double*>(x), n,
                       d, round_f32, out, ld);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_ts_square(const double* dist, int n, double* out, int ld, ava_stream_t s) {
  if (!dist || !ts_matrix_ok(out, ld, n)) return AVA_EINVAL;
  const int64_t blocks = ceil_div64((int64_t)n * n, 256);
  hipLaunchKernelGGL(ts_square_kernel, dim3((unsigned)blocks), dim3(256), 0, to_stream(s), dist, n, out, ld);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_ts_joint(double* p, int ld, int n, double perplexity, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!ts_matrix_ok(p, ld, n) || !ws || !(perplexity > 0.0) || !(perplexity < (double)n)) return AVA_EINVAL;
  if (ws_bytes < ava_ts_workspace_bytes(n, 0)) return AVA_EWORKSPACE;
  double* partials = reinterpret_cast<double*>(ava_align256(ws));
  const int T = ts_tiles(n);
  double* S = partials + (size_t)T * T;
  const double desired_entropy = log((double)(float)perplexity);     // sklearn's `float desired_perplexity`
  hipLaunchKernelGGL(ts_perplexity_kernel, dim3(n), dim3(256), 0, to_stream(s), p, ld, n, desired_entropy);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(ts_joint_sum_kernel, dim3(T, T), dim3(256), 0, to_stream(s), p, ld, n, partials);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(ts_sum_kernel, dim3(1), dim3(1024), 0, to_stream(s), partials, (int64_t)T * T, S);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(ts_joint_write_kernel, dim3(T, T), dim3(256), 0, to_stream(s), p, ld, n, S);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// iterations of the descent (y != null) or one evaluation of the objective (grad_out != null)
static int ts_iterate(double* y, double* update, double* gains, const double* yc, const double* p, int ld, int n,
                      int n_iters, double momentum, double lr, double e, int chunks, double* grad_out, double* stats,
                      void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!ts_matrix_ok(p, ld, n) || !yc || !ts_aligned16(yc) || !stats || !ws || n_iters < 1 || !(e > 0.0))
    return AVA_EINVAL;
  if (chunks <= 0) chunks = ava_ts_col_chunks(n);
  if (chunks > TS_MAX_CHUNKS) return AVA_EINVAL;
  if (ws_bytes < ava_ts_workspace_bytes(n, chunks)) return AVA_EWORKSPACE;
  const int T = ts_row_tiles(n), cw = ts_chunk_width(n, chunks), nz = T * chunks;
  double* zpart = reinterpret_cast<double*>(ava_align256(ws));
  double* klpart = zpart + nz;
  double* gpart = klpart + nz;                       // 2 nz doubles in: still on a 16-byte boundary
  const double2* Y = reinterpret_cast<const double2*>(yc);
  const dim3 grid(T, chunks);
  for (int it = 0; it < n_iters; ++it) {
    hipLaunchKernelGGL(ts_z_kernel, grid, dim3(256), 0, to_stream(s), Y, n, cw, zpart);
    AVA_CHECK_LAUNCH();
    const bool want_kl = it == n_iters - 1;          // the only KL the caller's host code reads (sklearn's checks)
    if (want_kl)
      hipLaunchKernelGGL(ts_grad_kernel<true>, grid, dim3(256), 0, to_stream(s), Y, p, ld, n, cw, zpart, nz, e, gpart,
                         klpart);
    else
      hipLaunchKernelGGL(ts_grad_kernel<false>, grid, dim3(256), 0, to_stream(s), Y, p, ld, n, cw, zpart, nz, e, gpart,
                         klpart);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL(ts_update_kernel, dim3(1), dim3(1024), 0, to_stream(s), gpart, klpart, n, chunks,
                       want_kl ? nz : -1, momentum, lr, y, update, gains, grad_out, stats + 2 * it);
    AVA_CHECK_LAUNCH();
  }
  return AVA_OK;
}

extern "C" int ava_ts_kl_gradient(const double* y, const double* p, int ld, int n, double exaggeration,
                                  int col_chunks, double* grad, double* stats, void* ws, size_t ws_bytes,
                                  ava_stream_t s) {
  if (!grad) return AVA_EINVAL;
  return ts_iterate(nullptr, nullptr, nullptr, y, p, ld, n, 1, 0.0, 0.0, exaggeration, col_chunks, grad, stats, ws,
                    ws_bytes, s);
}

extern "C" int ava_ts_descend(double* y, double* update, double* gains, const double* p, int ld, int n, int n_iters,
                              double momentum, double lr, double exaggeration, int col_chunks, double* stats,
                              void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!y || !update || !gains) return AVA_EINVAL;
  return ts_iterate(y, update, gains, y, p, ld, n, n_iters, momentum, lr, exaggeration, col_chunks, nullptr, stats, ws,
                    ws_bytes, s);
}
