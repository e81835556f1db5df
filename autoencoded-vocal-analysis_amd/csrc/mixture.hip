// Gaussian mixture models of latent means: the device counterpart of scikit-learn 1.7's
// GaussianMixture with 'full' or 'diag' covariances (sklearn/mixture/_gaussian_mixture.py, _base.py).  X is [N][d]
// float32 or float64 and is converted on load; everything else is fp64; nothing uses floating-point atomics; the same
// inputs give the same bits on every run, whatever the grid or the number of CUs.
//
// One EM iteration is six launches:
//   1. gm_estep_full_kernel / gm_estep_diag_kernel   per 64 (32) rows: log_prob[n][k] = -(d log 2pi + |y|^2) / 2 + log det
//        P_k + log w_k with y = (x_n - mu_k)^T P_k ('full': on the fp64 matrix cores, the mean subtracted as the rows are
//        written into LDS, never X P - mu P) or (x_n - mu_k) o p_k ('diag'); then the row's max-shifted logsumexp,
//        log_prob_norm[n], log_resp[n][k], resp[n][k] = exp(log_resp)
//   2. gm_moments_kernel<0>   per chunk of GM_CHUNK rows (and slice of the K d outputs): sums of log_prob_norm,
//        of resp[:, k] and of resp[:, k] x
//   3. gm_finish_kernel       nk, means, weights, lower bound, the stopping rule
//   4. gm_cov_full_kernel     per (chunk, component): sum_n z z^T, z = sqrt(resp[n][k]) (x_n - mu_k) staged once for both
//        operands of the MFMA (features are the tile's rows, samples the contraction), blocks on or below the diagonal
//      gm_moments_kernel<1>   'diag': sum_n resp[n][k] (x_n - mu_k)^2, centred, never E[x^2] - mu^2
//   5. gm_cov_finish_kernel   chunks in order, / nk, + reg_covar on the diagonal; the upper triangle is the mirror
//   6. gm_factor_kernel       a workgroup per component: lower Cholesky factor L, P = (L^-1)^T, sum log diag P
//      gm_factor_diag_kernel  p = 1 / sqrt(c)
// The E-step is a separate launch from the chunk sums, so that the k-means start (labels from ava_nn_argmin, one-hot resp
// from gm_onehot_kernel) shares launches 2 and 3 with the M-step.
//
// Order contract (every sum is one of these; none depends on the grid, on the tile a row falls in or on N):
//   |y|^2 'full'   y_j of a row: ascending 4-wide MFMA steps from feature 0 (corr_mfma_stage); the squares: lane (j & 15)
//                  adds its blocks j >> 4 ascending by fma, then the xor butterfly 8, 4, 2, 1 over the 16 lanes.  Padded
//                  features are exact zeros.
//   |y|^2 'diag'   features ascending, by fma
//   logsumexp      components ascending: the maximum, then sum_k exp(lp_k - max)
//   chunk sums     chunk c owns rows [c GM_CHUNK, (c + 1) GM_CHUNK); every sum of launches 2 and 4 'diag' takes its rows
//                  ascending by fma from 0; launch 4 'full' takes them in ascending 4-wide MFMA steps from the chunk's
//                  first row.  Rows past N are exact zeros.
//   across chunks  ascending from chunk 0 (launches 3 and 5)
//   weights        nk / N, then divided by their ascending sum; log det: ascending sum of log P_jj
//   Cholesky       L_ij = (c_ij - sum_{m<j} L_im L_jm) / L_jj, m ascending by fma; inverse: column c of L^-1 by forward
//                  substitution, -(sum_{m=c}^{i-1} L_im M_mc) / L_ii, m ascending by fma
//
// Iterations without the host: ctl[0] is the status word (1: a covariance was not positive definite), ctl[1] the number
// of iterations that ran, ctl[2 + it] whether the loop had stopped BEFORE iteration it.  Every launch of iteration it
// begins with a uniform read of ctl[2 + it] (and, up to the factorisation, of ctl[0]) and returns at once if it is set;
// gm_finish_kernel writes lower_bounds[it], ctl[1] = it + 1 and ctl[2 + it + 1] = stopped before | |lb - previous| < tol.
// A flag per iteration instead of one `done` word: a word written by one workgroup of a launch and read by the others
// of the same launch would race, and the covariance launches of the stopping iteration still have to run (sklearn keeps
// that iteration's M-step).
#include <float.h>
#include <math.h>

#include "common.h"
#include "corr_tile.h"

#define GM_MAX_D 128
#define GM_MAX_K 64
#define GM_CHUNK 2048            // rows of a chunk of the partial sums: a constant, never derived from the grid
#define GM_MANY_CHUNKS 64        // gm_moments_kernel: outputs per thread by the number of chunks (no result depends on it)
#define GM_ET 64                 // rows of an E-step tile ('full'): 16 per wave
#define GM_DT 32                 // rows of an E-step tile ('diag') and of a stage of gm_moments_kernel
#define GM_LPLD (GM_MAX_K + 1)   // row stride of the log_prob tile in LDS
#define GM_LOG_2PI 1.8378770664093453

__device__ __forceinline__ bool gm_stopped(const int* __restrict__ ctl, int it, bool with_status) {
  return ctl != nullptr && (ctl[2 + it] != 0 || (with_status && ctl[0] != 0));
}

// lp [rows][GM_LPLD] holds the weighted log probabilities of the tile's rows; writes log_prob_norm, log_resp and resp of
// rows [r0, min(r0 + rows, n)).  lse: rows doubles of LDS.  Starts with a barrier (lp complete).
__device__ __forceinline__ void gm_normalise_rows(const double* lp, double* lse, int rows, int64_t r0, int n, int K, int t,
                                                  double* __restrict__ lpn, double* __restrict__ log_resp,
                                                  double* __restrict__ resp) {
  __syncthreads();
  if (t < rows && r0 + t < n) {
    const double* row = lp + t * GM_LPLD;
    double m = row[0];
    for (int k = 1; k < K; ++k) m = fmax(m, row[k]);
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp(row[k] - m);
    const double v = log(s) + m;
    lse[t] = v;
    lpn[r0 + t] = v;
  }
  __syncthreads();
  for (int e = t; e < rows * K; e += 256) {
    const int r = e / K, k = e - r * K;
    if (r0 + r < n) {
      const double lr = lp[r * GM_LPLD + k] - lse[r];
      log_resp[(size_t)(r0 + r) * K + k] = lr;
      resp[(size_t)(r0 + r) * K + k] = exp(lr);
    }
  }
}

// ---- 1. E-step ------------------------------------------------------------------------------------------------------
// NB = 16-feature blocks (d <= 16 NB).  Wave w owns rows [16 w, 16 w + 16) of the tile and all NB blocks of y.
template <int NB, typename T>
__global__ __launch_bounds__(256) void gm_estep_full_kernel(const T* __restrict__ X, int n, int d, int K,
                                                            const double* __restrict__ weights,
                                                            const double* __restrict__ means,
                                                            const double* __restrict__ pchol,
                                                            const double* __restrict__ logdet, double* __restrict__ lpn,
                                                            double* __restrict__ log_resp, double* __restrict__ resp,
                                                            const int* __restrict__ ctl, int it) {
  __shared__ double xs[GM_ET * CORR_LD];
  __shared__ double ps[NB * 16 * CORR_LD];
  __shared__ double lp[GM_ET * GM_LPLD];
  __shared__ double lse[GM_ET];
  if (gm_stopped(ctl, it, true)) return;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63, sr = t >> 4, sc = t & 15;
  const int64_t r0 = (int64_t)blockIdx.x * GM_ET;
  // the tile's rows stay in registers over the components: element (row sr + 16 j, feature 16 b + sc)
  T xv[NB][GM_ET / 16];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int j = 0; j < GM_ET / 16; ++j) {
      const int64_t g = r0 + sr + 16 * j;
      const int f = 16 * b + sc;
      xv[b][j] = (f < d && g < n) ? X[(size_t)g * d + f] : (T)0;
    }
  for (int k = 0; k < K; ++k) {
    corr_d4 acc[1][NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[0][b] = corr_d4{0.0, 0.0, 0.0, 0.0};
    const double* mu = means + (size_t)k * d;
    const double* P = pchol + (size_t)k * d * d;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int k0 = 16 * b;
      if (k0 < d) {                                    // uniform
        __syncthreads();                               // the stage before is consumed
        const int f = k0 + sc;
        const double m = f < d ? mu[f] : 0.0;
#pragma unroll
        for (int j = 0; j < GM_ET / 16; ++j) {
          const int r = sr + 16 * j;
          xs[r * CORR_LD + sc] = (f < d && r0 + r < n) ? (double)xv[b][j] - m : 0.0;
        }
        // ps row jo (output feature), column i (contracted feature k0 + i) = P[k0 + i][jo]; 16 consecutive jo per load
        const int fi = k0 + sr;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int jo = sc + 16 * j;
          ps[jo * CORR_LD + sr] = (fi < d && jo < d) ? P[(size_t)fi * d + jo] : 0.0;
        }
        __syncthreads();
        corr_mfma_stage<1, NB>(xs, ps, w * 16, 0, lane, acc);
      }
    }
    const double tail = logdet[k] + log(weights[k]);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < NB; ++b) s = fma(acc[0][b][reg], acc[0][b][reg], s);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if ((lane & 15) == 0) lp[(w * 16 + (lane >> 4) + 4 * reg) * GM_LPLD + k] = -0.5 * ((double)d * GM_LOG_2PI + s) + tail;
    }
  }
  gm_normalise_rows(lp, lse, GM_ET, r0, n, K, t, lpn, log_resp, resp);
}

// thread (row t & 31, component t >> 5 + 8 i); the tile's rows in LDS as fp64
template <typename T>
__global__ __launch_bounds__(256) void gm_estep_diag_kernel(const T* __restrict__ X, int n, int d, int K,
                                                            const double* __restrict__ weights,
                                                            const double* __restrict__ means,
                                                            const double* __restrict__ pdiag,
                                                            const double* __restrict__ logdet, double* __restrict__ lpn,
                                                            double* __restrict__ log_resp, double* __restrict__ resp,
                                                            const int* __restrict__ ctl, int it) {
  __shared__ double xs[GM_DT * (GM_MAX_D + 1)];
  __shared__ double lp[GM_DT * GM_LPLD];
  __shared__ double lse[GM_DT];
  if (gm_stopped(ctl, it, true)) return;
  const int t = threadIdx.x, ld = d + 1;
  const int64_t r0 = (int64_t)blockIdx.x * GM_DT;
  for (int e = t; e < GM_DT * d; e += 256) {
    const int r = e / d, f = e - r * d;
    xs[r * ld + f] = r0 + r < n ? (double)X[(size_t)(r0 + r) * d + f] : 0.0;
  }
  __syncthreads();
  const int r = t & (GM_DT - 1);
  for (int k = t >> 5; k < K; k += 256 / GM_DT) {
    const double* mu = means + (size_t)k * d;
    const double* p = pdiag + (size_t)k * d;
    double s = 0.0;
    for (int f = 0; f < d; ++f) {
      const double y = (xs[r * ld + f] - mu[f]) * p[f];
      s = fma(y, y, s);
    }
    lp[r * GM_LPLD + k] = -0.5 * ((double)d * GM_LOG_2PI + s) + (logdet[k] + log(weights[k]));
  }
  gm_normalise_rows(lp, lse, GM_DT, r0, n, K, t, lpn, log_resp, resp);
}

// ---- 2. chunk sums --------------------------------------------------------------------------------------------------
// grid (chunks, ceil(K d / (256 OUT))): workgroup (c, y) owns chunk c and OUT outputs per thread, e = 256 (OUT y + i) + t
// = k d + j < K d.  MODE 0: s1[c][e] = sum_r resp[r][k] x[r][j]; the workgroups y = 0 also write s0[c][k] = sum_r
// resp[r][k] and ll[c] = sum_r lpn[r] (0 when lpn is not given).  MODE 1: s1[c][e] = sum_r resp[r][k] (x[r][j] -
// means[k][j])^2.  An output's sum does not depend on OUT, which the host chooses by the number of chunks: every
// workgroup stages the chunk's rows, so many chunks want few workgroups per chunk and few chunks want many.
template <typename T, int MODE, int OUT>
__global__ __launch_bounds__(256) void gm_moments_kernel(const T* __restrict__ X, int n, int d, int K,
                                                         const double* __restrict__ resp,
                                                         const double* __restrict__ lpn,
                                                         const double* __restrict__ means, double* __restrict__ s0,
                                                         double* __restrict__ s1, double* __restrict__ ll,
                                                         const int* __restrict__ ctl, int it) {
  __shared__ double xs[GM_DT * (GM_MAX_D + 1)];
  __shared__ double rs[GM_DT * GM_LPLD];
  if (gm_stopped(ctl, it, true)) return;
  const int t = threadIdx.x, ld = d + 1, KD = K * d;
  const bool first = MODE == 0 && blockIdx.y == 0;
  const int64_t c0 = (int64_t)blockIdx.x * GM_CHUNK;
  double acc[OUT], mu[OUT];
  int ok[OUT], oj[OUT];
#pragma unroll
  for (int i = 0; i < OUT; ++i) {
    const int e = 256 * (OUT * blockIdx.y + i) + t;
    acc[i] = 0.0;
    ok[i] = e < KD ? e / d : 0;
    oj[i] = e < KD ? e - ok[i] * d : 0;
    mu[i] = (MODE == 1 && e < KD) ? means[e] : 0.0;
  }
  double a0 = 0.0, al = 0.0;
  for (int64_t q0 = c0; q0 < c0 + GM_CHUNK && q0 < n; q0 += GM_DT) {
    __syncthreads();                                   // the stage before is consumed
    for (int i = t; i < GM_DT * d; i += 256) {
      const int r = i / d, f = i - r * d;
      xs[r * ld + f] = q0 + r < n ? (double)X[(size_t)(q0 + r) * d + f] : 0.0;
    }
    for (int i = t; i < GM_DT * K; i += 256) {
      const int r = i / K, k = i - r * K;
      rs[r * GM_LPLD + k] = q0 + r < n ? resp[(size_t)(q0 + r) * K + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < OUT; ++i) {
      if (256 * (OUT * blockIdx.y + i) + t < KD) {
        double a = acc[i];
#pragma unroll 8
        for (int r = 0; r < GM_DT; ++r) {
          if (MODE == 0) {
            a = fma(rs[r * GM_LPLD + ok[i]], xs[r * ld + oj[i]], a);
          } else {
            const double c = xs[r * ld + oj[i]] - mu[i];
            a = fma(rs[r * GM_LPLD + ok[i]] * c, c, a);
          }
        }
        acc[i] = a;
      }
    }
    if (first) {
      if (t < K)
        for (int r = 0; r < GM_DT; ++r) a0 += rs[r * GM_LPLD + t];
      if (t == 255 && lpn != nullptr)
        for (int r = 0; r < GM_DT; ++r) al += q0 + r < n ? lpn[q0 + r] : 0.0;
    }
  }
#pragma unroll
  for (int i = 0; i < OUT; ++i) {
    const int e = 256 * (OUT * blockIdx.y + i) + t;
    if (e < KD) s1[(size_t)blockIdx.x * KD + e] = acc[i];
  }
  if (first) {
    if (t < K) s0[(size_t)blockIdx.x * K + t] = a0;
    if (t == 255) ll[blockIdx.x] = al;
  }
}

// GM_MANY_CHUNKS chunks or more: 4 outputs per thread; fewer: 1, for more workgroups
template <typename T, int MODE>
static void gm_launch_moments(const T* X, int n, int d, int K, const double* resp, const double* lpn,
                              const double* means, double* s0, double* s1, double* ll, const int* ctl, int it,
                              hipStream_t st) {
  const int chunks = ceil_div(n, GM_CHUNK);
  if (chunks >= GM_MANY_CHUNKS)
    hipLaunchKernelGGL((gm_moments_kernel<T, MODE, 4>), dim3(chunks, ceil_div(K * d, 1024)), dim3(256), 0, st, X, n, d, K,
                       resp, lpn, means, s0, s1, ll, ctl, it);
  else
    hipLaunchKernelGGL((gm_moments_kernel<T, MODE, 1>), dim3(chunks, ceil_div(K * d, 256)), dim3(256), 0, st, X, n, d, K,
                       resp, lpn, means, s0, s1, ll, ctl, it);
}

// ---- 3. nk, means, weights, lower bound, stopping rule --------------------------------------------------------------
// grid K + 1, 128 threads.  Workgroup k < K: means[k][:].  Workgroup K: nk, weights and (lower_bounds given) the bound
// of iteration it and the flags of the header.
__global__ __launch_bounds__(128) void gm_finish_kernel(const double* __restrict__ s0, const double* __restrict__ s1,
                                                        const double* __restrict__ ll, int chunks, int n, int d, int K,
                                                        double* __restrict__ nk_out, double* __restrict__ means,
                                                        double* __restrict__ weights, double* __restrict__ lower_bounds,
                                                        double tol, int* __restrict__ ctl, int it) {
  __shared__ double wk[GM_MAX_K];
  const int t = threadIdx.x, k = blockIdx.x;
  if (gm_stopped(ctl, it, true)) {
    if (k == K && t == 0) ctl[2 + it + 1] = 1;         // the loop stays stopped
    return;
  }
  if (k < K) {
    double nk = 0.0;
    for (int c = 0; c < chunks; ++c) nk += s0[(size_t)c * K + k];
    nk += 10.0 * DBL_EPSILON;
    if (t < d) {
      double m = 0.0;
      for (int c = 0; c < chunks; ++c) m += s1[((size_t)c * K + k) * d + t];
      means[(size_t)k * d + t] = m / nk;
    }
    return;
  }
  if (t < K) {
    double nk = 0.0;
    for (int c = 0; c < chunks; ++c) nk += s0[(size_t)c * K + t];
    nk += 10.0 * DBL_EPSILON;
    nk_out[t] = nk;
    wk[t] = nk / (double)n;
  }
  __syncthreads();
  if (t < K) {
    double s = 0.0;
    for (int j = 0; j < K; ++j) s += wk[j];
    weights[t] = wk[t] / s;
  }
  if (t == 0 && lower_bounds != nullptr) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += ll[c];
    const double lb = s / (double)n;
    lower_bounds[it] = lb;
    if (ctl != nullptr) {
      const double prev = it > 0 ? lower_bounds[it - 1] : -INFINITY;
      ctl[1] = it + 1;
      ctl[2 + it + 1] = fabs(lb - prev) < tol ? 1 : 0;
    }
  }
}

// ---- 4. covariance partials, 'full' ---------------------------------------------------------------------------------
// grid (chunks, K).  cpart [chunk][k][DP][DP], DP = 16 NB: the 16 x 16 blocks (a, b), b <= a, are written, block
// a (a + 1) / 2 + b by wave (a (a + 1) / 2 + b) & 3.  A stage holds 16 samples: zs row = feature, column = sample.
template <int NB, typename T>
__global__ __launch_bounds__(256) void gm_cov_full_kernel(const T* __restrict__ X, int n, int d, int K,
                                                          const double* __restrict__ resp,
                                                          const double* __restrict__ means, double* __restrict__ cpart,
                                                          const int* __restrict__ ctl, int it) {
  __shared__ double zs[NB * 16 * CORR_LD];
  if (gm_stopped(ctl, it, true)) return;
  constexpr int BLOCKS = NB * (NB + 1) / 2, PER = (BLOCKS + 3) / 4, DP = NB * 16;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63, fl = t & 15, sr = t >> 4;
  const int k = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * GM_CHUNK;
  int ba[PER], bb[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int idx = w + 4 * i;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= idx) ++a;
    ba[i] = a;
    bb[i] = idx - a * (a + 1) / 2;
  }
  corr_d4 acc[PER][1][1];
#pragma unroll
  for (int i = 0; i < PER; ++i) acc[i][0][0] = corr_d4{0.0, 0.0, 0.0, 0.0};
  double mu[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) mu[j] = fl + 16 * j < d ? means[(size_t)k * d + fl + 16 * j] : 0.0;
  for (int64_t q0 = c0; q0 < c0 + GM_CHUNK && q0 < n; q0 += CORR_KC) {
    const int64_t g = q0 + sr;
    const double sq = g < n ? sqrt(resp[(size_t)g * K + k]) : 0.0;
    double z[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int f = fl + 16 * j;
      z[j] = (f < d && g < n) ? sq * ((double)X[(size_t)g * d + f] - mu[j]) : 0.0;
    }
    __syncthreads();                                   // the stage before is consumed
#pragma unroll
    for (int j = 0; j < NB; ++j) zs[(fl + 16 * j) * CORR_LD + sr] = z[j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if (w + 4 * i < BLOCKS) corr_mfma_stage<1, 1>(zs, zs, ba[i] * 16, bb[i] * 16, lane, acc[i]);   // wave-uniform
  }
  double* out = cpart + ((size_t)blockIdx.x * K + k) * DP * DP;
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (w + 4 * i < BLOCKS) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        out[(size_t)(ba[i] * 16 + (lane >> 4) + 4 * reg) * DP + bb[i] * 16 + (lane & 15)] = acc[i][0][0][reg];
    }
}

// ---- 5. covariances -------------------------------------------------------------------------------------------------
// grid (ceil(d d / 256), K) 'full', (ceil(d / 256), K) 'diag'.  part: cpart (ldp = DP) or the MODE 1 chunk sums.
__global__ __launch_bounds__(256) void gm_cov_finish_kernel(const double* __restrict__ part, int chunks, int d, int ldp,
                                                            int K, int diag, const double* __restrict__ nk,
                                                            double reg_covar, double* __restrict__ cov,
                                                            const int* __restrict__ ctl, int it) {
  if (gm_stopped(ctl, it, true)) return;
  const int e = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (diag) {
    if (e >= d) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[((size_t)c * K + k) * d + e];
    cov[(size_t)k * d + e] = s / nk[k] + reg_covar;
    return;
  }
  if (e >= d * d) return;
  const int i = e / d, j = e - i * d;
  if (j > i) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[((size_t)c * K + k) * ldp * ldp + (size_t)i * ldp + j];
  s /= nk[k];
  if (i == j) s += reg_covar;
  cov[((size_t)k * d + i) * d + j] = s;
  cov[((size_t)k * d + j) * d + i] = s;
}

// ---- 6. factorisation -----------------------------------------------------------------------------------------------
// A workgroup of 256 per component; dynamic LDS: a [d][d + 1], inv [d], pivot [d].  A pivot that is not a positive finite number
// sets status[0] = 1 and ends the workgroup (the branch is uniform: every thread reads the pivot from LDS).
__global__ __launch_bounds__(256) void gm_factor_kernel(const double* __restrict__ cov, int d, double* __restrict__ pchol,
                                                        double* __restrict__ logdet, int* __restrict__ status,
                                                        const int* __restrict__ ctl, int it) {
  extern __shared__ __align__(16) double gm_sm[];
  if (gm_stopped(ctl, it, false)) return;
  const int t = threadIdx.x, k = blockIdx.x, ld = d + 1;
  double* a = gm_sm;
  double* inv = gm_sm + (size_t)d * ld;
  double* pivot = inv + d;
  const double* C = cov + (size_t)k * d * d;
  double* P = pchol + (size_t)k * d * d;
  for (int e = t; e < d * d; e += 256) {
    const int i = e / d, j = e - i * d;
    a[i * ld + j] = C[e];
  }
  __syncthreads();
  for (int j = 0; j < d; ++j) {                        // column j; the columns before it are final
    const int i = j + t;
    double s = 0.0;
    if (i < d) {
      s = a[i * ld + j];
      for (int m = 0; m < j; ++m) s = fma(-a[i * ld + m], a[j * ld + m], s);
    }
    if (t == 0) pivot[j] = s;
    __syncthreads();
    const double piv = pivot[j];
    if (!(piv > 0.0) || !(piv <= DBL_MAX)) {           // uniform: every thread reads the same word
      if (t == 0) status[0] = 1;
      return;
    }
    const double ljj = sqrt(piv);
    if (i < d) a[i * ld + j] = i == j ? ljj : s / ljj;
    if (t == 0) inv[j] = 1.0 / ljj;
    __syncthreads();
  }
  // column c of M = L^-1 into row c of the upper triangle: a[c][i] = M[i][c], i > c
  if (t < d) {
    const int c = t;
    for (int i = c + 1; i < d; ++i) {
      double s = a[i * ld + c] * inv[c];
      for (int m = c + 1; m < i; ++m) s = fma(a[i * ld + m], a[c * ld + m], s);
      a[c * ld + i] = -s / a[i * ld + i];
    }
  }
  __syncthreads();
  for (int e = t; e < d * d; e += 256) {
    const int c = e / d, i = e - c * d;
    P[e] = i > c ? a[c * ld + i] : (i == c ? inv[c] : 0.0);
  }
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) s += log(inv[j]);
    logdet[k] = s;
  }
}

// grid K, 128 threads
__global__ __launch_bounds__(128) void gm_factor_diag_kernel(const double* __restrict__ cov, int d,
                                                             double* __restrict__ pdiag, double* __restrict__ logdet,
                                                             int* __restrict__ status, const int* __restrict__ ctl,
                                                             int it) {
  __shared__ double p[GM_MAX_D];
  if (gm_stopped(ctl, it, false)) return;
  const int t = threadIdx.x, k = blockIdx.x;
  if (t < d) {
    const double c = cov[(size_t)k * d + t];
    const bool bad = !(c > 0.0) || !(c <= DBL_MAX);
    if (bad) status[0] = 1;
    p[t] = bad ? 1.0 : 1.0 / sqrt(c);
    pdiag[(size_t)k * d + t] = p[t];
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) s += log(p[j]);
    logdet[k] = s;
  }
}

// ---- k-means start: labels -> one-hot responsibilities --------------------------------------------------------------
// resp[i][k] = (labels[i] == k); changed[0] += the number of rows whose label differs from prev[i]; prev[i] = labels[i]
__global__ __launch_bounds__(256) void gm_onehot_kernel(const int64_t* __restrict__ labels, int64_t* __restrict__ prev,
                                                        int n, int K, double* __restrict__ resp,
                                                        int* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool diff = false;
  if (i < n) {
    const int64_t lab = labels[i];
    for (int k = 0; k < K; ++k) resp[(size_t)i * K + k] = k == lab ? 1.0 : 0.0;
    diff = prev[i] != lab;
    prev[i] = lab;
  }
  const int c = __popcll(__ballot(diff));
  if ((threadIdx.x & 63) == 0 && c > 0) atomicAdd(changed, c);        // an integer count: exact in any order
}

// ---- host -----------------------------------------------------------------------------------------------------------
static inline int gm_chunks(int n) { return ceil_div(n, GM_CHUNK); }
static inline int gm_nb(int d) { return d <= 16 ? 1 : d <= 32 ? 2 : d <= 64 ? 4 : 8; }
static inline bool gm_shape_ok(int n, int d, int K, int cov_type) {
  return d >= 1 && d <= GM_MAX_D && K >= 1 && K <= GM_MAX_K && n >= K && (cov_type == 0 || cov_type == 1);
}

struct gm_ws {
  double *s0, *s1, *ll, *nk, *cpart;
};
static size_t gm_ws_layout(int n, int d, int K, int cov_type, void* base, gm_ws* out) {
  const size_t chunks = gm_chunks(n), dp = 16 * (size_t)gm_nb(d);
  ava_ws_cursor c(base);
  double* s0 = c.take<double>(chunks * K);
  double* s1 = c.take<double>(chunks * K * d);
  double* ll = c.take<double>(chunks);
  double* nk = c.take<double>(K);
  double* cpart = c.take<double>(cov_type == 0 ? chunks * K * dp * dp : 0);
  if (out) *out = gm_ws{s0, s1, ll, nk, cpart};
  return c.bytes();
}

extern "C" int ava_gm_max_d(void) { return GM_MAX_D; }
extern "C" int ava_gm_max_k(void) { return GM_MAX_K; }
extern "C" int ava_gm_chunk_rows(void) { return GM_CHUNK; }

extern "C" size_t ava_gm_workspace_bytes(int n, int d, int k, int cov_type) {
  if (!gm_shape_ok(n, d, k, cov_type)) return 0;
  return gm_ws_layout(n, d, k, cov_type, nullptr, nullptr);
}

template <typename T>
static int gm_launch_estep(const T* X, int n, int d, int K, int cov_type, const double* weights, const double* means,
                           const double* pchol, const double* logdet, double* lpn, double* log_resp, double* resp,
                           const int* ctl, int it, hipStream_t st) {
  if (cov_type == 1) {
    hipLaunchKernelGGL(gm_estep_diag_kernel<T>, dim3(ceil_div(n, GM_DT)), dim3(256), 0, st, X, n, d, K, weights, means,
                       pchol, logdet, lpn, log_resp, resp, ctl, it);
  } else {
    const dim3 grid(ceil_div(n, GM_ET));
#define GM_ESTEP(NB_)                                                                                                  \
  hipLaunchKernelGGL((gm_estep_full_kernel<NB_, T>), grid, dim3(256), 0, st, X, n, d, K, weights, means, pchol, logdet, \
                     lpn, log_resp, resp, ctl, it)
    switch (gm_nb(d)) {
      case 1: GM_ESTEP(1); break;
      case 2: GM_ESTEP(2); break;
      case 4: GM_ESTEP(4); break;
      default: GM_ESTEP(8); break;
    }
#undef GM_ESTEP
  }
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// launches 2 and 3: nk, means, weights (and the bound / flags when lower_bounds is given)
template <typename T>
static int gm_launch_means(const T* X, int n, int d, int K, const double* resp, const double* lpn, const gm_ws& w,
                           double* means, double* weights, double* lower_bounds, double tol, int* ctl, int it,
                           hipStream_t st) {
  const int chunks = gm_chunks(n);
  gm_launch_moments<T, 0>(X, n, d, K, resp, lpn, nullptr, w.s0, w.s1, w.ll, ctl, it, st);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(gm_finish_kernel, dim3(K + 1), dim3(128), 0, st, w.s0, w.s1, w.ll, chunks, n, d, K, w.nk, means,
                     weights, lower_bounds, tol, ctl, it);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

static int gm_factor_attr(void) {
  static bool attr = false;
  if (!attr) {
    const int bytes = (GM_MAX_D * (GM_MAX_D + 1) + 2 * GM_MAX_D) * (int)sizeof(double);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gm_factor_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            bytes) != hipSuccess)
      return AVA_ELAUNCH;
    attr = true;
  }
  return AVA_OK;
}

// launches 4 to 6 at the means of launch 3
template <typename T>
static int gm_launch_cov(const T* X, int n, int d, int K, int cov_type, const double* resp, const gm_ws& w,
                         const double* means, double reg_covar, double* cov, double* pchol, double* logdet,
                         int* status, const int* ctl, int it, hipStream_t st) {
  const int chunks = gm_chunks(n);
  if (cov_type == 1) {
    gm_launch_moments<T, 1>(X, n, d, K, resp, nullptr, means, w.s0, w.s1, w.ll, ctl, it, st);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL(gm_cov_finish_kernel, dim3(ceil_div(d, 256), K), dim3(256), 0, st, w.s1, chunks, d, d, K, 1, w.nk,
                       reg_covar, cov, ctl, it);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL(gm_factor_diag_kernel, dim3(K), dim3(128), 0, st, cov, d, pchol, logdet, status, ctl, it);
    AVA_CHECK_LAUNCH();
    return AVA_OK;
  }
  const dim3 grid(chunks, K);
#define GM_COV(NB_)                                                                                              \
  hipLaunchKernelGGL((gm_cov_full_kernel<NB_, T>), grid, dim3(256), 0, st, X, n, d, K, resp, means, w.cpart, ctl, it)
  switch (gm_nb(d)) {
    case 1: GM_COV(1); break;
    case 2: GM_COV(2); break;
    case 4: GM_COV(4); break;
    default: GM_COV(8); break;
  }
#undef GM_COV
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(gm_cov_finish_kernel, dim3(ceil_div(d * d, 256), K), dim3(256), 0, st, w.cpart, chunks, d,
                     16 * gm_nb(d), K, 0, w.nk, reg_covar, cov, ctl, it);
  AVA_CHECK_LAUNCH();
  const size_t lds = ((size_t)d * (d + 1) + 2 * d) * sizeof(double);
  hipLaunchKernelGGL(gm_factor_kernel, dim3(K), dim3(256), lds, st, cov, d, pchol, logdet, status, ctl, it);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_gm_e_step(const void* x, int dtype, int n, int d, int k, int cov_type, const double* weights,
                             const double* means, const double* prec_chol, const double* log_det,
                             double* log_prob_norm, double* log_resp, double* resp, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !gm_shape_ok(n, d, k, cov_type) || !weights || !means || !prec_chol ||
      !log_det || !log_prob_norm || !log_resp || !resp)
    return AVA_EINVAL;
  return dtype == 0 ? gm_launch_estep(static_cast<const float*>(x), n, d, k, cov_type, weights, means, prec_chol,
                                      log_det, log_prob_norm, log_resp, resp, nullptr, 0, to_stream(s))
                    : gm_launch_estep(static_cast<const double*>(x), n, d, k, cov_type, weights, means, prec_chol,
                                      log_det, log_prob_norm, log_resp, resp, nullptr, 0, to_stream(s));
}

extern "C" int ava_gm_means(const void* x, int dtype, int n, int d, int k, const double* resp, double* weights,
                            double* means, double* nk, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !gm_shape_ok(n, d, k, 1) || !resp || !weights || !means || !nk || !ws)
    return AVA_EINVAL;
  if (ws_bytes < ava_gm_workspace_bytes(n, d, k, 1)) return AVA_EWORKSPACE;
  gm_ws w;
  gm_ws_layout(n, d, k, 1, ws, &w);
  w.nk = nk;
  return dtype == 0 ? gm_launch_means(static_cast<const float*>(x), n, d, k, resp, nullptr, w, means, weights, nullptr,
                                      0.0, nullptr, 0, to_stream(s))
                    : gm_launch_means(static_cast<const double*>(x), n, d, k, resp, nullptr, w, means, weights, nullptr,
                                      0.0, nullptr, 0, to_stream(s));
}

template <typename T>
static int gm_m_step(const T* X, int n, int d, int K, int cov_type, const double* resp, double reg_covar,
                     double* weights, double* means, double* cov, double* pchol, double* logdet, int* status,
                     const gm_ws& w, hipStream_t st) {
  int rc = gm_launch_means(X, n, d, K, resp, nullptr, w, means, weights, nullptr, 0.0, nullptr, 0, st);
  if (rc != AVA_OK) return rc;
  return gm_launch_cov(X, n, d, K, cov_type, resp, w, means, reg_covar, cov, pchol, logdet, status, nullptr, 0, st);
}

extern "C" int ava_gm_m_step(const void* x, int dtype, int n, int d, int k, int cov_type, const double* resp,
                             double reg_covar, double* weights, double* means, double* cov, double* prec_chol,
                             double* log_det, int* status, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !gm_shape_ok(n, d, k, cov_type) || !resp || !(reg_covar >= 0.0) || !weights ||
      !means || !cov || !prec_chol || !log_det || !status || !ws)
    return AVA_EINVAL;
  if (ws_bytes < ava_gm_workspace_bytes(n, d, k, cov_type)) return AVA_EWORKSPACE;
  if (cov_type == 0 && gm_factor_attr() != AVA_OK) return AVA_ELAUNCH;
  gm_ws w;
  gm_ws_layout(n, d, k, cov_type, ws, &w);
  return dtype == 0 ? gm_m_step(static_cast<const float*>(x), n, d, k, cov_type, resp, reg_covar, weights, means, cov,
                                prec_chol, log_det, status, w, to_stream(s))
                    : gm_m_step(static_cast<const double*>(x), n, d, k, cov_type, resp, reg_covar, weights, means, cov,
                                prec_chol, log_det, status, w, to_stream(s));
}

template <typename T>
static int gm_fit(const T* X, int n, int d, int K, int cov_type, double* weights, double* means, double* cov,
                  double* pchol, double* logdet, double tol, double reg_covar, int it0, int n_iters,
                  double* lower_bounds, int* ctl, double* lpn, double* log_resp, double* resp, const gm_ws& w,
                  hipStream_t st) {
  for (int it = it0; it < it0 + n_iters; ++it) {
    int rc = gm_launch_estep(X, n, d, K, cov_type, weights, means, pchol, logdet, lpn, log_resp, resp, ctl, it, st);
    if (rc != AVA_OK) return rc;
    rc = gm_launch_means(X, n, d, K, resp, lpn, w, means, weights, lower_bounds, tol, ctl, it, st);
    if (rc != AVA_OK) return rc;
    rc = gm_launch_cov(X, n, d, K, cov_type, resp, w, means, reg_covar, cov, pchol, logdet, ctl, ctl, it, st);
    if (rc != AVA_OK) return rc;
  }
  return AVA_OK;
}

extern "C" int ava_gm_fit(const void* x, int dtype, int n, int d, int k, int cov_type, double* weights, double* means,
                          double* cov, double* prec_chol, double* log_det, double tol, double reg_covar, int it0,
                          int n_iters, double* lower_bounds, int* ctl, double* log_prob_norm, double* log_resp,
                          double* resp, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (!x || (dtype != 0 && dtype != 1) || !gm_shape_ok(n, d, k, cov_type) || !weights || !means || !cov || !prec_chol ||
      !log_det || !(tol >= 0.0) || !(reg_covar >= 0.0) || it0 < 0 || n_iters < 1 || n_iters > (1 << 20) ||
      it0 > (1 << 20) || !lower_bounds || !ctl || !log_prob_norm || !log_resp || !resp || !ws)
    return AVA_EINVAL;
  if (ws_bytes < ava_gm_workspace_bytes(n, d, k, cov_type)) return AVA_EWORKSPACE;
  if (cov_type == 0 && gm_factor_attr() != AVA_OK) return AVA_ELAUNCH;
  gm_ws w;
  gm_ws_layout(n, d, k, cov_type, ws, &w);
  return dtype == 0 ? gm_fit(static_cast<const float*>(x), n, d, k, cov_type, weights, means, cov, prec_chol, log_det,
                             tol, reg_covar, it0, n_iters, lower_bounds, ctl, log_prob_norm, log_resp, resp, w,
                             to_stream(s))
                    : gm_fit(static_cast<const double*>(x), n, d, k, cov_type, weights, means, cov, prec_chol, log_det,
                             tol, reg_covar, it0, n_iters, lower_bounds, ctl, log_prob_norm, log_resp, resp, w,
                             to_stream(s));
}

extern "C" int ava_gm_onehot(const int64_t* labels, int64_t* prev, int n, int k, double* resp, int* changed,
                             ava_stream_t s) {
  if (!labels || !prev || n < 1 || k < 1 || k > GM_MAX_K || !resp || !changed) return AVA_EINVAL;
  hipLaunchKernelGGL(gm_onehot_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, to_stream(s), labels, prev, n, k, resp,
                     changed);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
