// MMD^2 between two sets of latent means.
//
// Replaces the pure-Python O(n^2) double loops of the reference's `_estimate_mmd2`
// (ava/plotting/mmd_plots.py:255-296), `_estimate_mmd2_linear_time` (:299-312) and the pair distances of
// `estimate_median_sigma` (:450-474).  The reference works on float64 numpy arrays; so do these kernels (fp64 VALU;
// the differences are formed directly, sum_k (x_k - y_k)^2, exactly as the reference does -- no |x|^2 + |y|^2 - 2xy
// expansion, which cancels for near pairs; the pairwise kernel's tile and the order of its sums are those of
// sqdist_tile.h).  Every sum is a fixed-order two-stage reduction (per-workgroup partial, then one workgroup over the
// partials): deterministic, no atomics.
//
// Pairwise kernel: a workgroup owns a 64 x 64 tile of (i, j) pairs; the 64 + 64 latent rows are gathered through the
// index lists into LDS once (row stride z|1 doubles: conflict-free column walks) and each thread accumulates a 4 x 4
// block of squared distances in registers while sweeping the z latent dimensions, then adds exp(A * dist) of the
// pairs that exist (and, for the within-set terms, lie above the diagonal: i < j).
//
// There is one implementation of the sums.  The condition-by-condition matrix of `_calculate_mmd2` (:337-447, row f16)
// is one launch sequence over the index lists of all conditions, sorted by condition: a workgroup per tile of every
// block of condition pairs (mmd_matrix_pair_kernel; mmd_matrix_linear_kernel for the linear-time estimator), then one
// workgroup per block for the second stage (mmd_matrix_finalize_kernel).  One pair of index lists is that matrix with
// two conditions, which is how ava_amd.mmd serves `_estimate_mmd2` and `_estimate_mmd2_linear_time`.  A block's bits
// depend on its own two lists, z and sigma alone -- not on the other conditions of the launch sequence, nor on where
// its workgroups fall in it.  The order of every sum is stated once, on the functions below:
//   first stage   mmd_tile_sum (a tile), mmd_linear_sum and mmd_matrix_linear_kernel (a workgroup's quadruples)
//   second stage  mmd_matrix_finalize_kernel
#include "common.h"
#include "sqdist_tile.h"

#define MMD_T SQD_T

// One 64 x 64 tile of (i, j) pairs of the index lists ia (rows i0 ..) and ib (rows j0 ..): gathers the rows into LDS,
// accumulates the squared distances and returns, in thread 0, the sum of exp(A * dist) over the pairs that exist (and,
// with sym, lie above the diagonal).  Order: a thread adds its 4 x 4 pairs row by row (r outer, c inner), then the wave
// sums of wave_sum_d, then (r0 + r1) + (r2 + r3) over the four waves.  sm: 2 * 64 * (z | 1) doubles of LDS, red: 4
// doubles of LDS.
__device__ __forceinline__ double mmd_tile_sum(double* sm, double* red, const double* __restrict__ L, int z,
                                               const int64_t* __restrict__ ia, int na,
                                               const int64_t* __restrict__ ib, int nb, double A, int sym, int i0,
                                               int j0) {
  const int zp = z | 1;
  double* xs = sm;                       // [64][zp]
  double* ys = sm + MMD_T * zp;          // [64][zp]
  const int t = threadIdx.x;
  for (int e = t; e < MMD_T * z; e += 256) {
    const int r = e / z, k = e - r * z;
    const int gi = i0 + r, gj = j0 + r;
    xs[r * zp + k] = gi < na ? L[(size_t)ia[gi] * z + k] : 0.0;
    ys[r * zp + k] = gj < nb ? L[(size_t)ib[gj] * z + k] : 0.0;
  }
  __syncthreads();
  const int ty = t >> 4, tx = t & 15;
  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  sqd_accumulate(xs, ys, zp, z, ty, tx, acc);
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int gi = i0 + ty + 16 * r, gj = j0 + tx + 16 * c;
      const bool ok = gi < na && gj < nb && (!sym || gi < gj);
      if (ok) s += exp(A * acc[r][c]);
    }
  s = wave_sum_d(s);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// out[p] = sum_k (L[a[p]][k] - L[b[p]][k])^2   (estimate_median_sigma's sampled pairs, mmd_plots.py:468-471)
__global__ __launch_bounds__(256) void pair_sqdist_kernel(const double* __restrict__ L, int z,
                                                          const int64_t* __restrict__ a,
                                                          const int64_t* __restrict__ b, int n,
                                                          double* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const double* x = L + (size_t)a[p] * z;
  const double* y = L + (size_t)b[p] * z;
  double s = 0.0;
  for (int k = 0; k < z; ++k) {
    const double d = x[k] - y[k];
    s = fma(d, d, s);
  }
  out[p] = s;
}

// linear-time estimator (mmd_plots.py:299-312): one thread per i < m, h(x1,y1,x2,y2) = k(x1,x2)+k(y1,y2)-k(x1,y2)-k(x2,y1).
// This thread's sum over i = first, first + stride, ... < m, in that order; a quadruple's four kernel values are added
// left to right.
__device__ __forceinline__ double mmd_linear_sum(const double* __restrict__ L, int z, const int64_t* __restrict__ i1,
                                                 const int64_t* __restrict__ i2, int m, double A, int first,
                                                 int stride) {
  double s = 0.0;
  for (int i = first; i < m; i += stride) {
    const double* x1 = L + (size_t)i1[2 * i] * z;
    const double* y1 = L + (size_t)i2[2 * i] * z;
    const double* x2 = L + (size_t)i1[2 * i + 1] * z;
    const double* y2 = L + (size_t)i2[2 * i + 1] * z;
    double dxx = 0.0, dyy = 0.0, dxy = 0.0, dyx = 0.0;
    for (int k = 0; k < z; ++k) {
      const double a1 = x1[k], b1 = y1[k], a2 = x2[k], b2 = y2[k];
      dxx = fma(a1 - a2, a1 - a2, dxx);
      dyy = fma(b1 - b2, b1 - b2, dyy);
      dxy = fma(a1 - b2, a1 - b2, dxy);
      dyx = fma(a2 - b1, a2 - b1, dyx);
    }
    s += exp(A * dxx) + exp(A * dyy) - exp(A * dxy) - exp(A * dyx);
  }
  return s;
}

// ---- all condition pairs in one launch sequence (the loop of _calculate_mmd2, mmd_plots.py:395-418) -------------------
// idx: the index lists of all C conditions, concatenated in condition order; off[c] .. off[c + 1]: the list of
// condition c.  A table row is 4 int64: {first workgroup of the launch, first workspace slot, a, b}; row n_rows is the
// sentinel {total workgroups, total slots, 0, 0}.  Every row owns at least one workgroup, so column 0 is strictly
// increasing and the row of a workgroup is found by bisection.
#define MMD_ROW 4
#define MMD_MAX_C 4096        // conditions: the finalise launch has one workgroup per block, C (C + 1) / 2 < 2^24
#define MMD_CHUNK (1 << 20)   // workgroups per launch (grid x block stays far below 2^32 threads)

__device__ __forceinline__ int mmd_find_row(const int64_t* __restrict__ table, int n_rows, int64_t g) {
  int lo = 0, hi = n_rows;               // table[lo][0] <= g < table[hi][0]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[(size_t)mid * MMD_ROW] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// Quadratic estimator: a row is a block (a, b), a <= b, in row-major order.  A block with a < b launches its whole
// ti x tj tile grid; a block with a = b is symmetric (i < j only) and launches the tiles with tj >= ti, row by row.
// Either way the tile's sum (mmd_tile_sum) lands at slot ti * tiles_j + tj of the block's row-major grid in the
// workspace, and the slots below the diagonal of a symmetric block are never written nor read.
__global__ __launch_bounds__(256) void mmd_matrix_pair_kernel(const double* __restrict__ L, int z,
                                                              const int64_t* __restrict__ idx,
                                                              const int64_t* __restrict__ off,
                                                              const int64_t* __restrict__ blocks, int n_blocks,
                                                              double A, int64_t g0, double* __restrict__ partials) {
  extern __shared__ __align__(16) double sm[];
  __shared__ double red[4];
  const int64_t g = g0 + blockIdx.x;     // workgroup of the whole sequence: a launch covers at most MMD_CHUNK of them
  const int p = mmd_find_row(blocks, n_blocks, g);
  const int64_t* row = blocks + (size_t)p * MMD_ROW;
  const int a = (int)row[2], b = (int)row[3];
  const int64_t oa = off[a], ob = off[b];
  const int na = (int)(off[a + 1] - oa), nb = (int)(off[b + 1] - ob);
  const int tiles_j = (nb + MMD_T - 1) / MMD_T;
  const int64_t l = g - row[0];
  int ti, tj;
  if (a == b) {
    // rows 0 .. r - 1 of the upper triangle hold r * tiles_j - r (r - 1) / 2 tiles: the last r with that many <= l
    int lo = 0, hi = tiles_j;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)mid * tiles_j - (int64_t)mid * (mid - 1) / 2 <= l) lo = mid; else hi = mid;
    }
    ti = lo;
    tj = ti + (int)(l - ((int64_t)ti * tiles_j - (int64_t)ti * (ti - 1) / 2));
  } else {
    ti = (int)(l / tiles_j);
    tj = (int)(l - (int64_t)ti * tiles_j);
  }
  const double s = mmd_tile_sum(sm, red, L, z, idx + oa, na, idx + ob, nb, A, a == b, ti * MMD_T, tj * MMD_T);
  if (threadIdx.x == 0) partials[row[1] + (int64_t)ti * tiles_j + tj] = s;
}

// Linear estimator: a row is a pair (a, b), a < b, with m = min(n_a, n_b) / 2 quadruples and min(ceil(m / 256), 1024)
// workgroups.  Thread t of the pair's workgroup wg takes the quadruples wg * 256 + t, + 256 * (the pair's workgroups),
// ... (mmd_linear_sum); then the wave sums, then (r0 + r1) + (r2 + r3) over the four waves, into slot wg of the pair.
__global__ __launch_bounds__(256) void mmd_matrix_linear_kernel(const double* __restrict__ L, int z,
                                                                const int64_t* __restrict__ idx,
                                                                const int64_t* __restrict__ off,
                                                                const int64_t* __restrict__ pairs, int n_pairs,
                                                                double A, int64_t g0, double* __restrict__ partials) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t g = g0 + blockIdx.x;
  const int p = mmd_find_row(pairs, n_pairs, g);
  const int64_t* row = pairs + (size_t)p * MMD_ROW;
  const int a = (int)row[2], b = (int)row[3];
  const int64_t oa = off[a], ob = off[b];
  const int na = (int)(off[a + 1] - oa), nb = (int)(off[b + 1] - ob);
  const int m = (na < nb ? na : nb) / 2;
  const int wg = (int)(g - row[0]), n_wg = (int)(row[MMD_ROW] - row[0]);
  double s = mmd_linear_sum(L, z, idx + oa, idx + ob, m, A, wg * 256 + t, n_wg * 256);
  s = wave_sum_d(s);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) partials[row[1] + wg] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Second stage: one workgroup per table row reduces the row's slots.  Thread t adds the slots t, t + 256, ... of the
// row-major grid in that order (passing over the slots below the diagonal of a symmetric block, which stand for +0.0:
// a sum of exp() values is never -0.0, so adding them would change no bit), then the wave sums, then (r0 + r1) +
// (r2 + r3) over the four waves, then one multiply by c.  linear = 0: within[a] = sum * c, c = 2 / (n_a (n_a - 1)), for
// a = b (and cross[a][a] = 0); cross[a][b] = cross[b][a] = sum * c, c = 2 / (n_a n_b), otherwise.  linear = 1:
// cross[a][b] = cross[b][a] = sum * c, c = 1 / m.
__global__ __launch_bounds__(256) void mmd_matrix_finalize_kernel(const double* __restrict__ partials,
                                                                  const int64_t* __restrict__ off,
                                                                  const int64_t* __restrict__ table, int C, int linear,
                                                                  double* __restrict__ within,
                                                                  double* __restrict__ cross) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t* row = table + (size_t)blockIdx.x * MMD_ROW;
  const int a = (int)row[2], b = (int)row[3];
  const int na = (int)(off[a + 1] - off[a]), nb = (int)(off[b + 1] - off[b]);
  const double* p = partials + row[1];
  const int64_t n_p = row[MMD_ROW + 1] - row[1];
  const int tiles_j = (nb + MMD_T - 1) / MMD_T;
  const bool sym = !linear && a == b;
  double s = 0.0;
  for (int64_t i = t; i < n_p; i += 256) {
    if (sym) {
      const int64_t ti = i / tiles_j;
      if (i - ti * tiles_j < ti) continue;
    }
    s += p[i];
  }
  const double r = wave_sum_d(s);
  if ((t & 63) == 0) red[t >> 6] = r;
  __syncthreads();
  if (t == 0) {
    const double sum = (red[0] + red[1]) + (red[2] + red[3]);
    double c;
    if (linear) c = 1.0 / (double)((na < nb ? na : nb) / 2);
    else if (a == b) c = 2.0 / ((double)na * (na - 1));
    else c = 2.0 / ((double)na * nb);
    const double v = sum * c;
    if (sym) {
      within[a] = v;
      cross[(size_t)a * C + a] = 0.0;
    } else {
      cross[(size_t)a * C + b] = v;
      cross[(size_t)b * C + a] = v;
    }
  }
}

// ---- host side of the one-pass matrix ----------------------------------------------------------------------------------
// walks the C + 1 host offsets: every count >= 2 and < 2^31; returns the workgroups and workspace slots of the sequence
static bool mmd_matrix_totals(const int64_t* offsets, int C, int linear, int64_t* n_wg, int64_t* n_slots) {
  int64_t wg = 0, slots = 0;
  for (int a = 0; a < C; ++a) {
    const int64_t na = offsets[a + 1] - offsets[a];
    if (na < 2 || na > 0x7fffffff) return false;
  }
  for (int a = 0; a < C; ++a) {
    const int64_t na = offsets[a + 1] - offsets[a], ta = (na + MMD_T - 1) / MMD_T;
    for (int b = linear ? a + 1 : a; b < C; ++b) {
      const int64_t nb = offsets[b + 1] - offsets[b], tb = (nb + MMD_T - 1) / MMD_T;
      if (linear) {
        const int64_t m = (na < nb ? na : nb) / 2;
        int64_t g = (m + 255) / 256;
        if (g > 1024) g = 1024;
        wg += g;
        slots += g;
      } else {
        wg += a == b ? ta * (ta + 1) / 2 : ta * tb;
        slots += ta * tb;
      }
      if (slots > ((int64_t)1 << 40)) return false;
    }
  }
  *n_wg = wg;
  *n_slots = slots;
  return true;
}

extern "C" size_t ava_mmd2_matrix_workspace_bytes(const int64_t* offsets, int C, int linear) {
  int64_t wg, slots;
  if (offsets == nullptr || C < 2 || C > MMD_MAX_C || !mmd_matrix_totals(offsets, C, linear, &wg, &slots)) return 0;
  return (size_t)(slots + 8) * sizeof(double);
}

static int mmd_matrix_check(const double* latent, int z, const int64_t* idx, const int64_t* offsets,
                            const int64_t* offsets_dev, int C, const int64_t* table, int64_t total, int linear,
                            double sigma, const void* out, const void* ws, size_t ws_bytes) {
  if (latent == nullptr || idx == nullptr || offsets == nullptr || offsets_dev == nullptr || table == nullptr ||
      out == nullptr || ws == nullptr || z < 1 || z > 128 || C < 2 || C > MMD_MAX_C || !(sigma > 0.0))
    return AVA_EINVAL;
  int64_t wg, slots;
  if (!mmd_matrix_totals(offsets, C, linear, &wg, &slots)) return AVA_EINVAL;
  if (wg != total || wg > 0x7fffffff) return AVA_EINVAL;
  if (ws_bytes < (size_t)(slots + 8) * sizeof(double)) return AVA_EWORKSPACE;
  return AVA_OK;
}

extern "C" int ava_mmd2_matrix(const double* latent, int z, const int64_t* idx, const int64_t* offsets,
                               const int64_t* offsets_dev, int C, const int64_t* blocks, int64_t total_tiles,
                               double sigma, double* within, double* cross, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (within == nullptr) return AVA_EINVAL;
  int rc = mmd_matrix_check(latent, z, idx, offsets, offsets_dev, C, blocks, total_tiles, 0, sigma, cross, ws, ws_bytes);
  if (rc != AVA_OK) return rc;
  hipStream_t st = to_stream(s);
  const size_t lds = (size_t)2 * MMD_T * (z | 1) * sizeof(double);
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&mmd_matrix_pair_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)((size_t)2 * MMD_T * 129 * sizeof(double))) != hipSuccess)
      return AVA_ELAUNCH;
    attr = true;
  }
  const int n_blocks = C * (C + 1) / 2;
  const double A = -0.5 / (sigma * sigma);
  double* partials = reinterpret_cast<double*>(ws);
  for (int64_t g0 = 0; g0 < total_tiles; g0 += MMD_CHUNK) {
    const int64_t left = total_tiles - g0;
    const int grid = (int)(left < MMD_CHUNK ? left : MMD_CHUNK);
    hipLaunchKernelGGL(mmd_matrix_pair_kernel, dim3(grid), dim3(256), lds, st, latent, z, idx, offsets_dev, blocks,
                       n_blocks, A, g0, partials);
    AVA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mmd_matrix_finalize_kernel, dim3(n_blocks), dim3(256), 0, st, partials, offsets_dev, blocks, C, 0,
                     within, cross);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_mmd2_matrix_linear(const double* latent, int z, const int64_t* idx, const int64_t* offsets,
                                      const int64_t* offsets_dev, int C, const int64_t* pairs, int64_t total_workgroups,
                                      double sigma, double* out, void* ws, size_t ws_bytes, ava_stream_t s) {
  int rc = mmd_matrix_check(latent, z, idx, offsets, offsets_dev, C, pairs, total_workgroups, 1, sigma, out, ws, ws_bytes);
  if (rc != AVA_OK) return rc;
  hipStream_t st = to_stream(s);
  const int n_pairs = C * (C - 1) / 2;
  const double A = -0.5 / (sigma * sigma);
  double* partials = reinterpret_cast<double*>(ws);
  for (int64_t g0 = 0; g0 < total_workgroups; g0 += MMD_CHUNK) {
    const int64_t left = total_workgroups - g0;
    const int grid = (int)(left < MMD_CHUNK ? left : MMD_CHUNK);
    hipLaunchKernelGGL(mmd_matrix_linear_kernel, dim3(grid), dim3(256), 0, st, latent, z, idx, offsets_dev, pairs,
                       n_pairs, A, g0, partials);
    AVA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mmd_matrix_finalize_kernel, dim3(n_pairs), dim3(256), 0, st, partials, offsets_dev, pairs, C, 1,
                     nullptr, out);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_pair_sqdist(const double* latent, int z, const int64_t* a, const int64_t* b, int n, double* out,
                               ava_stream_t s) {
  if (latent == nullptr || a == nullptr || b == nullptr || out == nullptr || z < 1 || n < 1) return AVA_EINVAL;
  hipLaunchKernelGGL(pair_sqdist_kernel, dim3((n + 255) / 256), dim3(256), 0, to_stream(s), latent, z, a, b, n, out);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
