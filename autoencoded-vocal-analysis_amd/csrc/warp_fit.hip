// The shift-and-slope time-warp fit on the device: the arithmetic of the reference's
// ava/preprocessing/warping.py (apply_warp :25-50, the objectives :148-163) and the kernels ava_amd/warp_fit.py chains
// into align_specs.  All arithmetic is fp64; spectrograms are [N][F][T] contiguous, fp32 or fp64.
//
//   warpfit_apply_kernel       out[n][f][j] = interp1d(spec[n][f][:])(shift + slope j), the ends held (fill_value)
//   warpfit_mean_kernel        target[f][j] = sum_n spec[n][f][j] / N, summed n = 0, 1, ... (np.mean(axis=0))
//   warpfit_candidates_kernel  the grid of (shift, log slope) candidates around every motif's current best
//   warpfit_loss_kernel        loss[n][c] = sum_{f,j} (interp(n; candidate c) - target)^2 + the two penalties: the hot one
//   warpfit_argmin_kernel      per motif the best candidate (lowest index on ties, NaN never wins) and its parameters
//
// The interpolation restates scipy's interp1d(kind='linear') on the grid 0 .. T-1 operation for operation:
// i = clip(searchsorted(x, p), 1, T-1), lo = i - 1, value = (y[lo+1] - y[lo]) * (p - lo) + y[lo], every product and sum
// rounded on its own (__dmul_rn / __dadd_rn: -ffp-contract=on must not fuse them), so a warped pixel has the reference's
// bits.  p < 0 gives y[0], p > T-1 gives y[T-1]; p == T-1 takes lo = T-2 and weight 1 and reads nothing behind the row.
//
// The loss kernel: one workgroup (4 waves) per (motif, block of WF_CB = 8 candidates).  A wave owns two candidates and
// first writes their per-column (lo, weight) tables to LDS, once for all F rows.  Then WF_FR = 4 rows of the motif and of
// the target are staged in LDS at a time (one coalesced HBM read per candidate BLOCK, not per candidate) and every lane
// walks the columns j = lane, lane + 64, ... of its candidates over the staged rows: two adjacent LDS reads of the
// motif row (neighbouring lanes read neighbouring columns, since slopes are near 1), one of the target, five fp64
// operations.  Sums run lane-sequentially and then through one xor-shuffle tree: a fixed order, no atomics.
// LDS: (4 (T+1) + 4 T + 8 T) 8 + 8 T 4 bytes = 160 T + 32: 20.5 KB at T = 128 (7 workgroups / CU), 82 KB at the cap
// T = 512, where one more row set no longer fits twice on a CU.
//
// The piecewise-linear warp (row f14): K = n_knots + 2 knots per motif, u[k] the source position of the template column
// t_k = k (T-1) / (K-1).  Column j lies in segment k = min(j (K-1) / (T-1), K-2) (integers) and reads the source at
// p(j) = u_k + s_k (j - t_k), s_k = (u_{k+1} - u_k) / (t_{k+1} - t_k), every operation rounded on its own; with K = 2 that
// is wf_pos(u_0, s_0, j).  A candidate with some s_k <= 0 has loss +inf.
//
//   warpfit_pl_apply_kernel       warpfit_apply_kernel under knots [N][K]
//   warpfit_pl_candidates_kernel  candidates [N][C][K] around u [N][K]: one knot, or all knots together, moved by 0, -h, +h, ...
//   warpfit_pl_loss_kernel        warpfit_loss_kernel with the column tables made from knots: the same LDS, the same sums
//                                 (wf_block_sums), + shift_l u_0^2 + slope_l mean_k (log s_k)^2
//   warpfit_argmin_kernel         serves both fits: its parameter width is 2 or K
//
// The grouped fits (row f17): many fit problems over the same spec in one launch.  A group is a sorted list of motifs, a
// sorted list of bins and two lambdas of its own; a virtual row is one (motif, group) pair (struct WfPlan).
//
//   warpfit_group_loss_kernel     warpfit_loss_kernel per virtual row: the motif, the target, the bins and the lambdas come
//   warpfit_group_pl_loss_kernel  through the plan, the bins are staged through their list in list order, and everything
//                                 else is the plain kernel's body (wf_loss_body / wf_pl_loss_body over wf_block_sums), so a
//                                 virtual row's losses have the bits of the plain kernel on the gathered tensor
//   warpfit_group_mean_kernel     every group's mean warped motif without the warped motifs: the apply kernels' values,
//                                 summed over the group's rows in rising order
//   the candidates and argmin kernels serve virtual rows as they are
#include "common.h"

#define WF_CB 8          // candidates per workgroup (two per wave)
#define WF_FR 4          // motif / target rows staged per pass
#define WF_MAX_T 512
#define WF_MAX_C 4096
#define WF_MAX_K 16      // knots of a piecewise-linear warp, the two outer ones included

struct WfTap { int lo; double w; };

// scipy interp1d's tap for position p on the grid 0 .. T-1 (T >= 2).  Above the grid: lo = T-1, w = 0, and the caller
// supplies y[T] = y[T-1] (LDS) or clamps (global).  NaN: weight NaN, so the value and any sum over it are NaN.
__device__ __forceinline__ WfTap wf_tap(double p, int T) {
  if (p != p) return {0, p};
  if (p < 0.0) return {0, 0.0};
  if (p > (double)(T - 1)) return {T - 1, 0.0};
  int i = (int)ceil(p);                                     // searchsorted(arange(T), p), side='left'
  i = i < 1 ? 1 : i;                                        // .clip(1, T-1)
  return {i - 1, __dsub_rn(p, (double)(i - 1))};
}

__device__ __forceinline__ double wf_lerp(double a, double b, double w) {
  return __dadd_rn(__dmul_rn(__dsub_rn(b, a), w), a);       // slope * (x_new - x_lo) + y_lo, scipy's order
}

__device__ __forceinline__ double wf_pos(double shift, double slope, int j) {
  return __dadd_rn(shift, __dmul_rn(slope, (double)j));     // shifts[i] + slopes[i] * np.arange(T)
}

// template column of knot k: k (T-1) / (K-1), the product exact, one rounded division
__device__ __forceinline__ double wf_knot_t(int k, int T, int K) { return __ddiv_rn((double)(k * (T - 1)), (double)(K - 1)); }

// slope of segment k (0 <= k <= K-2) of the knots u[0 .. K-1]
__device__ __forceinline__ double wf_pl_slope(const double* __restrict__ u, int k, int T, int K) {
  return __ddiv_rn(__dsub_rn(u[k + 1], u[k]), __dsub_rn(wf_knot_t(k + 1, T, K), wf_knot_t(k, T, K)));
}

// source position of column j under the knots u[0 .. K-1]; T - 1 >= K - 1, so every segment holds a column
__device__ __forceinline__ double wf_pl_pos(const double* __restrict__ u, int j, int T, int K) {
  int k = j * (K - 1) / (T - 1);
  k = k > K - 2 ? K - 2 : k;
  return __dadd_rn(u[k], __dmul_rn(wf_pl_slope(u, k, T, K), __dsub_rn((double)j, wf_knot_t(k, T, K))));
}

template <typename T_>
__global__ __launch_bounds__(256) void warpfit_pl_apply_kernel(const T_* __restrict__ spec, const double* __restrict__ knots,
                                                               int F, int T, int K, T_* __restrict__ out) {
  const int n = blockIdx.x;
  const double* u = knots + (size_t)n * K;
  for (int j = threadIdx.x; j < T; j += 256) {
    const WfTap t = wf_tap(wf_pl_pos(u, j, T, K), T);
    const int hi = t.lo + 1 < T ? t.lo + 1 : T - 1;
    for (int f = blockIdx.y; f < F; f += gridDim.y) {
      const T_* row = spec + ((size_t)n * F + f) * T;
      out[((size_t)n * F + f) * T + j] = (T_)wf_lerp((double)row[t.lo], (double)row[hi], t.w);
    }
  }
}

template <typename T_>
__global__ __launch_bounds__(256) void warpfit_apply_kernel(const T_* __restrict__ spec, const double* __restrict__ params,
                                                            int F, int T, T_* __restrict__ out) {
  const int n = blockIdx.x;
  const double shift = params[2 * (size_t)n], slope = params[2 * (size_t)n + 1];
  for (int j = threadIdx.x; j < T; j += 256) {
    const WfTap t = wf_tap(wf_pos(shift, slope, j), T);
    const int hi = t.lo + 1 < T ? t.lo + 1 : T - 1;
    for (int f = blockIdx.y; f < F; f += gridDim.y) {
      const T_* row = spec + ((size_t)n * F + f) * T;
      out[((size_t)n * F + f) * T + j] = (T_)wf_lerp((double)row[t.lo], (double)row[hi], t.w);
    }
  }
}

template <typename T_>
__global__ __launch_bounds__(256) void warpfit_mean_kernel(const T_* __restrict__ spec, int N, int64_t FT,
                                                           double* __restrict__ target) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= FT) return;
  double acc = 0.0;
  for (int n = 0; n < N; ++n) acc += (double)spec[(size_t)n * FT + e];
  target[e] = acc / (double)N;
}

// Candidate c = a * (2 kl + 1) + b of motif n, (a, b) walking the offsets 0, -1, +1, -2, +2, ... of each axis, so that
// candidate 0 is the centre x[n].  log slope = l0 + ob hl; the shift is moved so that the warp pivots about the middle
// column, shift = s0 + oa hs - (exp(log slope) - exp(l0)) (T-1)/2: the two axes of the grid are then nearly independent
// directions of the objective (a slope change about column 0 would drag the far end of the motif along).
__global__ __launch_bounds__(256) void warpfit_candidates_kernel(const double* __restrict__ x, int N, int T, int ks, int kl,
                                                                 double hs, double hl, double* __restrict__ cand) {
  const int C = (2 * ks + 1) * (2 * kl + 1);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)N * C) return;
  const int n = (int)(e / C), c = (int)(e - (int64_t)n * C);
  const int a = c / (2 * kl + 1), b = c - a * (2 * kl + 1);
  const int oa = (a & 1) ? -((a + 1) >> 1) : (a >> 1), ob = (b & 1) ? -((b + 1) >> 1) : (b >> 1);
  const double s0 = x[2 * (size_t)n], l0 = x[2 * (size_t)n + 1];
  double shift = s0 + oa * hs, ls = l0;
  if (ob != 0) {
    ls = l0 + ob * hl;
    shift -= (exp(ls) - exp(l0)) * (0.5 * (T - 1));
  }
  cand[2 * e] = shift;
  cand[2 * e + 1] = ls;
}

// Candidate c of motif n: the knots u[n][:] with knot `axis` (axis = -1: every knot) moved by o h, o = 0, -1, +1, -2, +2, ...
// so that candidate 0 is u[n] itself.  C = 2 ks + 1.
__global__ __launch_bounds__(256) void warpfit_pl_candidates_kernel(const double* __restrict__ u, int N, int K, int axis, int ks,
                                                                    double h, double* __restrict__ cand) {
  const int C = 2 * ks + 1;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)N * C * K) return;
  const int k = (int)(e % K);
  const int64_t nc = e / K;
  const int n = (int)(nc / C), c = (int)(nc - (int64_t)n * C);
  const int o = (c & 1) ? -((c + 1) >> 1) : (c >> 1);
  const double v = u[(size_t)n * K + k];
  cand[e] = (o != 0 && (axis < 0 || axis == k)) ? __dadd_rn(v, __dmul_rn((double)o, h)) : v;
}

// The sums of the loss kernels: with the (lo, weight) tables of the workgroup's candidates in LDS (written by the wave
// that owns the candidate; the first barrier below publishes them), acc[k] = this lane's share of
// sum_{f,j} (interp - target)^2 for candidate c0 + wave + 4 k.
// G (the grouped fits, row f17): staged row f0 + r is row bins[f0 + r] of the motif, which has Fall rows; the target is
// compact, [F][T] by list position.  The plain form reads rows 0 .. F-1 and never looks at bins.
template <typename T_, bool G>
__device__ __forceinline__ void wf_block_sums(const T_* __restrict__ motif, const double* __restrict__ target,
                                              const int* __restrict__ bins, int Fall, int F, int T,
                                              int C, int c0, double* s_spec, double* s_tgt, const double* s_w,
                                              const int* s_lo, double (&acc)[2]) {
  const int TS = T + 1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int f0 = 0; f0 < F; f0 += WF_FR) {
    const int nr = F - f0 < WF_FR ? F - f0 : WF_FR;
    __syncthreads();                                        // the previous rows are consumed (first pass: tables written)
    for (int e = tid; e < nr * T; e += 256) {
      const int r = e / T, j = e - r * T;
      double v;
      if constexpr (G) {
        const int b = bins[f0 + r];                         // one coalesced read of T columns per staged row
        v = (unsigned)b < (unsigned)Fall ? (double)motif[(size_t)b * T + j] : __builtin_nan("");
      } else {
        v = (double)motif[(size_t)f0 * T + e];
      }
      s_spec[r * TS + j] = v;
      if (j == T - 1) s_spec[r * TS + T] = v;
      s_tgt[r * T + j] = target[(size_t)f0 * T + e];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int cc = wave + 4 * k;
      if (c0 + cc >= C) continue;
      for (int j = lane; j < T; j += 64) {
        const int lo = s_lo[cc * T + j];
        const double w = s_w[cc * T + j];
        for (int r = 0; r < nr; ++r) {
          const double d = wf_lerp(s_spec[r * TS + lo], s_spec[r * TS + lo + 1], w) - s_tgt[r * T + j];
          acc[k] += d * d;
        }
      }
    }
  }
}

// The loss of one (motif, candidate block): the body of warpfit_loss_kernel and of its grouped form.  raw: the tables are
// lo = j, w = 0, the unwarped row read exactly, no candidate is read and no penalty added.
template <typename T_, bool G>
__device__ __forceinline__ void wf_loss_body(const T_* __restrict__ motif, const double* __restrict__ target,
                                             const int* __restrict__ bins, int Fall, const double* __restrict__ cand, int F,
                                             int T, int C, double shift_lambda, double slope_lambda, int fixed_slope, int raw,
                                             double* __restrict__ loss) {
  extern __shared__ __align__(16) double wf_sm[];
  const int TS = T + 1;
  double* s_spec = wf_sm;                                   // [WF_FR][T + 1], column T repeats column T-1
  double* s_tgt = s_spec + WF_FR * TS;                      // [WF_FR][T]
  double* s_w = s_tgt + WF_FR * T;                          // [WF_CB][T]
  int* s_lo = reinterpret_cast<int*>(s_w + WF_CB * T);      // [WF_CB][T]
  const int c0 = blockIdx.y * WF_CB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  double shift[2], ls[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int cc = wave + 4 * k, c = c0 + cc;
    shift[k] = ls[k] = 0.0;
    if (c < C) {                                            // wave-uniform
      if (G && raw) {
        for (int j = lane; j < T; j += 64) {
          s_lo[cc * T + j] = j;
          s_w[cc * T + j] = 0.0;
        }
        continue;
      }
      shift[k] = cand[2 * (size_t)c];
      ls[k] = cand[2 * (size_t)c + 1];
      const double slope = fixed_slope ? 1.0 : exp(ls[k]);
      for (int j = lane; j < T; j += 64) {
        const WfTap t = wf_tap(wf_pos(shift[k], slope, j), T);
        s_lo[cc * T + j] = t.lo;
        s_w[cc * T + j] = t.w;
      }
    }
  }

  double acc[2] = {0.0, 0.0};
  wf_block_sums<T_, G>(motif, target, bins, Fall, F, T, C, c0, s_spec, s_tgt, s_w, s_lo, acc);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = c0 + wave + 4 * k;
    if (c >= C) continue;
    double tot = wave_sum_d(acc[k]);
    if (!(G && raw)) {
      // loss + shift_l * x[0]**2 + slope_l * x[1]**2, left to right
      tot = __dadd_rn(tot, __dmul_rn(shift_lambda, __dmul_rn(shift[k], shift[k])));
      if (!fixed_slope) tot = __dadd_rn(tot, __dmul_rn(slope_lambda, __dmul_rn(ls[k], ls[k])));
    }
    if (lane == 0) loss[c] = tot;
  }
}

template <typename T_>
__global__ __launch_bounds__(256) void warpfit_loss_kernel(const T_* __restrict__ spec, const double* __restrict__ target,
                                                           const double* __restrict__ cand, int F, int T, int C,
                                                           double shift_lambda, double slope_lambda, int fixed_slope,
                                                           double* __restrict__ loss) {
  const int n = blockIdx.x;
  wf_loss_body<T_, false>(spec + (size_t)n * F * T, target, nullptr, F, cand + 2 * (size_t)n * C, F, T, C, shift_lambda,
                          slope_lambda, fixed_slope, 0, loss + (size_t)n * C);
}

// The plan of the grouped fits (row f17): V virtual rows, row v being motif row_src[v] of spec [N][Fall][T] seen by group
// row_group[v]; group g owns the rows group_row_off[g] .. group_row_off[g+1] - 1 (rising source order), the bins
// bins[bin_off[g] .. bin_off[g+1] - 1] (rising) and the compact target [F_g][T] at targets + bin_off[g] T.
struct WfPlan {
  const int* row_src;
  const int* row_group;
  const int* group_row_off;
  const int* bin_off;
  const int* bins;
  int N, Fall;
};

// warpfit_loss_kernel over virtual rows: the motif, the target, the bins and both lambdas come through the plan, the rest
// is the plain kernel's, operation for operation; cand [V][C][2], loss [V][C]
template <typename T_>
__global__ __launch_bounds__(256) void warpfit_group_loss_kernel(const T_* __restrict__ spec, WfPlan pl,
                                                                 const double* __restrict__ targets,
                                                                 const double* __restrict__ cand, int T, int C,
                                                                 const double* __restrict__ shift_lambda,
                                                                 const double* __restrict__ slope_lambda, int fixed_slope,
                                                                 int raw, double* __restrict__ loss) {
  const int v = blockIdx.x, g = pl.row_group[v], n = pl.row_src[v];
  if ((unsigned)n >= (unsigned)pl.N) return;                // a broken plan reads nothing
  const int b0 = pl.bin_off[g], F = pl.bin_off[g + 1] - b0;
  wf_loss_body<T_, true>(spec + (size_t)n * pl.Fall * T, targets + (size_t)b0 * T, pl.bins + b0, pl.Fall,
                         raw ? nullptr : cand + 2 * (size_t)v * C, F, T, C, raw ? 0.0 : shift_lambda[g],
                         (raw || fixed_slope) ? 0.0 : slope_lambda[g], fixed_slope, raw, loss + (size_t)v * C);
}

// The loss body for candidates of K knots each, cand [C][K]: only the tables differ (a lane reads the two knots of its
// column's segment from the candidate, K <= 16 doubles that stay in cache).  fixed_slope: every slope is 1 and the
// positions are u_0 + j, the shift objective.  Crossed knots do not stop the sums -- wf_tap keeps every tap inside the
// row -- and the total is replaced by +inf.
template <typename T_, bool G>
__device__ __forceinline__ void wf_pl_loss_body(const T_* __restrict__ motif, const double* __restrict__ target,
                                                const int* __restrict__ bins, int Fall, const double* __restrict__ cand,
                                                int F, int T, int C, int K, double shift_lambda, double slope_lambda,
                                                int fixed_slope, int raw, double* __restrict__ loss) {
  extern __shared__ __align__(16) double wf_sm[];
  const int TS = T + 1;
  double* s_spec = wf_sm;                                   // as in wf_loss_body
  double* s_tgt = s_spec + WF_FR * TS;
  double* s_w = s_tgt + WF_FR * T;
  int* s_lo = reinterpret_cast<int*>(s_w + WF_CB * T);
  const int c0 = blockIdx.y * WF_CB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int cc = wave + 4 * k, c = c0 + cc;
    if (c < C) {                                            // wave-uniform
      if (G && raw) {
        for (int j = lane; j < T; j += 64) {
          s_lo[cc * T + j] = j;
          s_w[cc * T + j] = 0.0;
        }
        continue;
      }
      const double* u = cand + (size_t)c * K;
      for (int j = lane; j < T; j += 64) {
        const WfTap t = wf_tap(fixed_slope ? wf_pos(u[0], 1.0, j) : wf_pl_pos(u, j, T, K), T);
        s_lo[cc * T + j] = t.lo;
        s_w[cc * T + j] = t.w;
      }
    }
  }

  double acc[2] = {0.0, 0.0};
  wf_block_sums<T_, G>(motif, target, bins, Fall, F, T, C, c0, s_spec, s_tgt, s_w, s_lo, acc);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = c0 + wave + 4 * k;
    if (c >= C) continue;
    double tot = wave_sum_d(acc[k]);
    if (!(G && raw)) {
      const double* u = cand + (size_t)c * K;
      tot = __dadd_rn(tot, __dmul_rn(shift_lambda, __dmul_rn(u[0], u[0])));
      if (!fixed_slope) {
        double sq = 0.0;                                    // sum_k (log s_k)^2, k = 0, 1, ...
        bool crossed = false;
        for (int i = 0; i < K - 1; ++i) {
          const double sl = wf_pl_slope(u, i, T, K);
          crossed |= sl <= 0.0;
          const double l = log(sl);
          sq = __dadd_rn(sq, __dmul_rn(l, l));
        }
        tot = __dadd_rn(tot, __dmul_rn(slope_lambda, __ddiv_rn(sq, (double)(K - 1))));
        if (crossed) tot = __builtin_inf();
      }
    }
    if (lane == 0) loss[c] = tot;
  }
}

template <typename T_>
__global__ __launch_bounds__(256) void warpfit_pl_loss_kernel(const T_* __restrict__ spec, const double* __restrict__ target,
                                                              const double* __restrict__ cand, int F, int T, int C, int K,
                                                              double shift_lambda, double slope_lambda, int fixed_slope,
                                                              double* __restrict__ loss) {
  const int n = blockIdx.x;
  wf_pl_loss_body<T_, false>(spec + (size_t)n * F * T, target, nullptr, F, cand + (size_t)n * C * K, F, T, C, K, shift_lambda,
                             slope_lambda, fixed_slope, 0, loss + (size_t)n * C);
}

// warpfit_pl_loss_kernel over virtual rows; cand [V][C][K]
template <typename T_>
__global__ __launch_bounds__(256) void warpfit_group_pl_loss_kernel(const T_* __restrict__ spec, WfPlan pl,
                                                                    const double* __restrict__ targets,
                                                                    const double* __restrict__ cand, int T, int C, int K,
                                                                    const double* __restrict__ shift_lambda,
                                                                    const double* __restrict__ slope_lambda, int fixed_slope,
                                                                    int raw, double* __restrict__ loss) {
  const int v = blockIdx.x, g = pl.row_group[v], n = pl.row_src[v];
  if ((unsigned)n >= (unsigned)pl.N) return;
  const int b0 = pl.bin_off[g], F = pl.bin_off[g + 1] - b0;
  wf_pl_loss_body<T_, true>(spec + (size_t)n * pl.Fall * T, targets + (size_t)b0 * T, pl.bins + b0, pl.Fall,
                            raw ? nullptr : cand + (size_t)v * C * K, F, T, C, K, raw ? 0.0 : shift_lambda[g],
                            (raw || fixed_slope) ? 0.0 : slope_lambda[g], fixed_slope, raw, loss + (size_t)v * C);
}

// The grouped template (row f17): target_g[f][j] = sum over the group's rows, in rising order, of the value the apply
// kernels would store for that row -- interpolated under the row's own parameters and rounded to spec's dtype -- divided
// by the row count: warpfit_mean_kernel of warpfit_apply_kernel's output without that output.  One workgroup per (group,
// WM_TJ columns, share of the bins): WM_TR rows at a time, a row's tap for a column is computed once into LDS and then
// used for every bin of the workgroup's share; thread (column, bin lane) carries the running sum of its (bin, column)
// cells from one row set to the next through the target itself, which only that thread touches.  fp64, a fixed order,
// no atomics.  mode 0: params [V][2] = (shift, slope) through wf_pos; 1: knots [V][K] through wf_pl_pos; 2 (raw): the
// unwarped value, which an identity warp does not reproduce bit for bit.
#define WM_TJ 64
#define WM_TR 16
template <typename T_>
__global__ __launch_bounds__(256) void warpfit_group_mean_kernel(const T_* __restrict__ spec, WfPlan pl,
                                                                 const double* __restrict__ params, int T, int K, int mode,
                                                                 double* __restrict__ targets) {
  __shared__ int s_lo[WM_TR][WM_TJ];
  __shared__ double s_w[WM_TR][WM_TJ];
  const int g = blockIdx.x, j0 = blockIdx.y * WM_TJ;
  const int v0 = pl.group_row_off[g], R = pl.group_row_off[g + 1] - v0;
  const int b0 = pl.bin_off[g], F = pl.bin_off[g + 1] - b0;
  const int jc = threadIdx.x & (WM_TJ - 1), bl = threadIdx.x >> 6, j = j0 + jc;
  const int* bins = pl.bins + b0;
  double* tgt = targets + (size_t)b0 * T;
  for (int r0 = 0; r0 < R; r0 += WM_TR) {
    const int nr = R - r0 < WM_TR ? R - r0 : WM_TR;
    __syncthreads();                                        // the previous row set's taps are consumed
    if (mode != 2) {
      for (int e = threadIdx.x; e < nr * WM_TJ; e += 256) {
        const int r = e >> 6, jj = j0 + (e & (WM_TJ - 1));
        if (jj >= T) continue;
        const size_t v = (size_t)(v0 + r0 + r);
        const double p = mode == 0 ? wf_pos(params[2 * v], params[2 * v + 1], jj) : wf_pl_pos(params + v * K, jj, T, K);
        const WfTap t = wf_tap(p, T);
        s_lo[r][e & (WM_TJ - 1)] = t.lo;
        s_w[r][e & (WM_TJ - 1)] = t.w;
      }
    }
    __syncthreads();
    if (j >= T) continue;                                   // no barrier depends on this thread's work below
    for (int f = blockIdx.z * 4 + bl; f < F; f += 4 * gridDim.z) {
      const int b = bins[f];
      double acc = r0 == 0 ? 0.0 : tgt[(size_t)f * T + j];
      for (int r = 0; r < nr; ++r) {
        const int n = pl.row_src[v0 + r0 + r];
        T_ val;
        if ((unsigned)n >= (unsigned)pl.N || (unsigned)b >= (unsigned)pl.Fall) {
          val = (T_)__builtin_nan("");
        } else {
          const T_* row = spec + ((size_t)n * pl.Fall + b) * T;
          if (mode == 2) {
            val = row[j];
          } else {
            const int lo = s_lo[r][jc], hi = lo + 1 < T ? lo + 1 : T - 1;
            val = (T_)wf_lerp((double)row[lo], (double)row[hi], s_w[r][jc]);
          }
        }
        acc += (double)val;
      }
      tgt[(size_t)f * T + j] = r0 + nr >= R ? acc / (double)R : acc;
    }
  }
}

// one wave per motif: lanes take candidates lane, lane + 64, ... in rising order, then a (loss, index) min over the wave,
// which leaves the result in every lane; W <= 64 parameters per candidate (2: shift and log slope; K: knots)
__global__ __launch_bounds__(256) void warpfit_argmin_kernel(const double* __restrict__ loss, const double* __restrict__ cand,
                                                             int N, int C, int W, int* __restrict__ best,
                                                             double* __restrict__ x, double* __restrict__ best_loss) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  double bv = 0.0;
  int bi = -1;                                              // -1: nothing but NaN seen
  for (int c = lane; c < C; c += 64) {
    const double v = loss[(size_t)n * C + c];
    if (v == v && (bi < 0 || v < bv)) { bv = v; bi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi >= 0 && (bi < 0 || ov < bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
  }
  const int c = bi < 0 ? 0 : bi;                            // all NaN: candidate 0 and its NaN
  if (x != nullptr && lane < W) x[(size_t)W * n + lane] = cand[(size_t)W * ((size_t)n * C + c) + lane];
  if (lane == 0) {
    best[n] = c;
    if (best_loss != nullptr) best_loss[n] = loss[(size_t)n * C + c];
  }
}

static bool wf_shape_ok(int dtype, int N, int F, int T) {
  return (dtype == 0 || dtype == 1) && N >= 1 && F >= 1 && T >= 2 && T <= WF_MAX_T;
}

static size_t wf_loss_lds(int T) {
  return ((size_t)WF_FR * (T + 1) + (size_t)WF_FR * T + (size_t)WF_CB * T) * sizeof(double) + (size_t)WF_CB * T * sizeof(int);
}

extern "C" int ava_warpfit_max_t(void) { return WF_MAX_T; }

extern "C" int ava_warpfit_apply(const void* spec, int dtype, int N, int F, int T, const double* params, void* out,
                                 ava_stream_t s) {
  if (spec == nullptr || params == nullptr || out == nullptr || !wf_shape_ok(dtype, N, F, T)) return AVA_EINVAL;
  const dim3 grid(N, F < 64 ? F : 64);
  if (dtype == 0)
    hipLaunchKernelGGL(warpfit_apply_kernel<float>, grid, dim3(256), 0, to_stream(s), static_cast<const float*>(spec), params,
                       F, T, static_cast<float*>(out));
  else
    hipLaunchKernelGGL(warpfit_apply_kernel<double>, grid, dim3(256), 0, to_stream(s), static_cast<const double*>(spec),
                       params, F, T, static_cast<double*>(out));
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_mean(const void* spec, int dtype, int N, int F, int T, double* target, ava_stream_t s) {
  if (spec == nullptr || target == nullptr || !wf_shape_ok(dtype, N, F, T)) return AVA_EINVAL;
  const int64_t FT = (int64_t)F * T;
  if (ceil_div64(FT, 256) > 2147483647) return AVA_EINVAL;
  const dim3 grid((unsigned)ceil_div64(FT, 256));
  if (dtype == 0)
    hipLaunchKernelGGL(warpfit_mean_kernel<float>, grid, dim3(256), 0, to_stream(s), static_cast<const float*>(spec), N, FT,
                       target);
  else
    hipLaunchKernelGGL(warpfit_mean_kernel<double>, grid, dim3(256), 0, to_stream(s), static_cast<const double*>(spec), N, FT,
                       target);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_candidates(const double* x, int N, int T, int ks, int kl, double hs, double hl, double* cand,
                                      ava_stream_t s) {
  if (x == nullptr || cand == nullptr || N < 1 || T < 2 || T > WF_MAX_T || ks < 0 || kl < 0 || ks > 31 || kl > 31) return AVA_EINVAL;
  if (!(hs >= 0.0) || !(hl >= 0.0) || (2 * ks + 1) * (2 * kl + 1) > WF_MAX_C) return AVA_EINVAL;
  const int64_t total = (int64_t)N * (2 * ks + 1) * (2 * kl + 1);
  if (ceil_div64(total, 256) > 2147483647) return AVA_EINVAL;
  hipLaunchKernelGGL(warpfit_candidates_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, to_stream(s), x, N, T, ks,
                     kl, hs, hl, cand);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename T_>
static int wf_launch_loss(const T_* spec, int N, int F, int T, const double* target, const double* cand, int C,
                          double shift_lambda, double slope_lambda, double* loss, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&warpfit_loss_kernel<T_>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)wf_loss_lds(WF_MAX_T)) != hipSuccess)
      return AVA_ELAUNCH;
    attr = true;
  }
  const int fixed = slope_lambda > 1.7976931348623157e308;  // +inf: the shift objective
  hipLaunchKernelGGL(warpfit_loss_kernel<T_>, dim3(N, ceil_div(C, WF_CB)), dim3(256), wf_loss_lds(T), st, spec, target, cand, F,
                     T, C, shift_lambda, fixed ? 0.0 : slope_lambda, fixed, loss);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_loss(const void* spec, int dtype, int N, int F, int T, const double* target, const double* cand,
                                int C, double shift_lambda, double slope_lambda, double* loss, ava_stream_t s) {
  if (spec == nullptr || target == nullptr || cand == nullptr || loss == nullptr || !wf_shape_ok(dtype, N, F, T)) return AVA_EINVAL;
  if (C < 1 || C > WF_MAX_C || shift_lambda != shift_lambda || slope_lambda != slope_lambda) return AVA_EINVAL;
  if (dtype == 0)
    return wf_launch_loss(static_cast<const float*>(spec), N, F, T, target, cand, C, shift_lambda, slope_lambda, loss, to_stream(s));
  return wf_launch_loss(static_cast<const double*>(spec), N, F, T, target, cand, C, shift_lambda, slope_lambda, loss, to_stream(s));
}

static int wf_launch_argmin(const double* loss, const double* cand, int N, int C, int W, int32_t* best, double* x,
                            double* best_loss, ava_stream_t s) {
  if (loss == nullptr || best == nullptr || N < 1 || C < 1 || C > WF_MAX_C) return AVA_EINVAL;
  if (x != nullptr && cand == nullptr) return AVA_EINVAL;
  hipLaunchKernelGGL(warpfit_argmin_kernel, dim3(ceil_div(N, 4)), dim3(256), 0, to_stream(s), loss, cand, N, C, W, best, x,
                     best_loss);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_argmin(const double* loss, const double* cand, int N, int C, int32_t* best, double* x,
                                  double* best_loss, ava_stream_t s) {
  return wf_launch_argmin(loss, cand, N, C, 2, best, x, best_loss, s);
}

// ---- the piecewise-linear warp (row f14) ------------------------------------------------------------------------------

static bool wf_knots_ok(int T, int K) { return K >= 2 && K <= WF_MAX_K && T - 1 >= 2 * (K - 1); }

extern "C" int ava_warpfit_max_knots(void) { return WF_MAX_K; }

extern "C" int ava_warpfit_pl_apply(const void* spec, int dtype, int N, int F, int T, const double* knots, int K, void* out,
                                    ava_stream_t s) {
  if (spec == nullptr || knots == nullptr || out == nullptr || !wf_shape_ok(dtype, N, F, T) || !wf_knots_ok(T, K)) return AVA_EINVAL;
  const dim3 grid(N, F < 64 ? F : 64);
  if (dtype == 0)
    hipLaunchKernelGGL(warpfit_pl_apply_kernel<float>, grid, dim3(256), 0, to_stream(s), static_cast<const float*>(spec), knots,
                       F, T, K, static_cast<float*>(out));
  else
    hipLaunchKernelGGL(warpfit_pl_apply_kernel<double>, grid, dim3(256), 0, to_stream(s), static_cast<const double*>(spec),
                       knots, F, T, K, static_cast<double*>(out));
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_pl_candidates(const double* u, int N, int K, int axis, int ks, double h, double* cand,
                                         ava_stream_t s) {
  if (u == nullptr || cand == nullptr || N < 1 || K < 2 || K > WF_MAX_K || axis < -1 || axis >= K) return AVA_EINVAL;
  if (ks < 0 || ks > 31 || !(h >= 0.0)) return AVA_EINVAL;
  const int64_t total = (int64_t)N * (2 * ks + 1) * K;
  if (ceil_div64(total, 256) > 2147483647) return AVA_EINVAL;
  hipLaunchKernelGGL(warpfit_pl_candidates_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, to_stream(s), u, N, K,
                     axis, ks, h, cand);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename T_>
static int wf_launch_pl_loss(const T_* spec, int N, int F, int T, const double* target, const double* cand, int C, int K,
                             double shift_lambda, double slope_lambda, double* loss, hipStream_t st) {
  // dynamic LDS over 64 KB (T > 409) has to be asked for, per device; asked whenever it is needed rather than once per
  // process, so that neither a second device nor two threads' first calls can miss it
  if (wf_loss_lds(T) > 65536 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&warpfit_pl_loss_kernel<T_>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)wf_loss_lds(WF_MAX_T)) != hipSuccess)
    return AVA_ELAUNCH;
  const int fixed = slope_lambda > 1.7976931348623157e308;  // +inf: the shift objective
  hipLaunchKernelGGL(warpfit_pl_loss_kernel<T_>, dim3(N, ceil_div(C, WF_CB)), dim3(256), wf_loss_lds(T), st, spec, target, cand,
                     F, T, C, K, shift_lambda, fixed ? 0.0 : slope_lambda, fixed, loss);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_pl_loss(const void* spec, int dtype, int N, int F, int T, const double* target, const double* cand,
                                   int C, int K, double shift_lambda, double slope_lambda, double* loss, ava_stream_t s) {
  if (spec == nullptr || target == nullptr || cand == nullptr || loss == nullptr || !wf_shape_ok(dtype, N, F, T)) return AVA_EINVAL;
  if (!wf_knots_ok(T, K) || C < 1 || C > WF_MAX_C || shift_lambda != shift_lambda || slope_lambda != slope_lambda) return AVA_EINVAL;
  if (dtype == 0)
    return wf_launch_pl_loss(static_cast<const float*>(spec), N, F, T, target, cand, C, K, shift_lambda, slope_lambda, loss,
                             to_stream(s));
  return wf_launch_pl_loss(static_cast<const double*>(spec), N, F, T, target, cand, C, K, shift_lambda, slope_lambda, loss,
                           to_stream(s));
}

extern "C" int ava_warpfit_pl_argmin(const double* loss, const double* cand, int N, int C, int K, int32_t* best, double* u,
                                     double* best_loss, ava_stream_t s) {
  if (K < 2 || K > WF_MAX_K) return AVA_EINVAL;
  return wf_launch_argmin(loss, cand, N, C, K, best, u, best_loss, s);
}

// ---- the grouped fits (row f17) -----------------------------------------------------------------------------------------

template <typename T_>
static int wf_launch_group_loss(const T_* spec, const WfPlan& pl, int V, int T, const double* targets, const double* cand,
                                int C, int K, const double* shift_lambda, const double* slope_lambda, int fixed_slope,
                                int raw, double* loss, hipStream_t st) {
  const void* fn = K == 0 ? reinterpret_cast<const void*>(&warpfit_group_loss_kernel<T_>)
                          : reinterpret_cast<const void*>(&warpfit_group_pl_loss_kernel<T_>);
  if (wf_loss_lds(T) > 65536 &&                             // as in wf_launch_pl_loss
      hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wf_loss_lds(WF_MAX_T)) != hipSuccess)
    return AVA_ELAUNCH;
  const dim3 grid(V, ceil_div(C, WF_CB));
  if (K == 0)
    hipLaunchKernelGGL(warpfit_group_loss_kernel<T_>, grid, dim3(256), wf_loss_lds(T), st, spec, pl, targets, cand, T, C,
                       shift_lambda, slope_lambda, fixed_slope, raw, loss);
  else
    hipLaunchKernelGGL(warpfit_group_pl_loss_kernel<T_>, grid, dim3(256), wf_loss_lds(T), st, spec, pl, targets, cand, T, C, K,
                       shift_lambda, slope_lambda, fixed_slope, raw, loss);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// K = 0: the shift-and-slope form
static int wf_group_loss(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src, const int32_t* row_group,
                         const int32_t* bin_off, const int32_t* bins, int V, const double* targets, const double* cand, int C,
                         int K, const double* shift_lambda, const double* slope_lambda, int fixed_slope, int raw, double* loss,
                         ava_stream_t s) {
  if (spec == nullptr || targets == nullptr || loss == nullptr || !wf_shape_ok(dtype, N, F, T)) return AVA_EINVAL;
  if (row_src == nullptr || row_group == nullptr || bin_off == nullptr || bins == nullptr || V < 1) return AVA_EINVAL;
  if (C < 1 || C > WF_MAX_C || (fixed_slope != 0 && fixed_slope != 1) || (raw != 0 && raw != 1)) return AVA_EINVAL;
  if (!raw && (cand == nullptr || shift_lambda == nullptr || slope_lambda == nullptr)) return AVA_EINVAL;
  const WfPlan pl{row_src, row_group, nullptr, bin_off, bins, N, F};
  if (dtype == 0)
    return wf_launch_group_loss(static_cast<const float*>(spec), pl, V, T, targets, cand, C, K, shift_lambda, slope_lambda,
                                fixed_slope, raw, loss, to_stream(s));
  return wf_launch_group_loss(static_cast<const double*>(spec), pl, V, T, targets, cand, C, K, shift_lambda, slope_lambda,
                              fixed_slope, raw, loss, to_stream(s));
}

extern "C" int ava_warpfit_group_loss(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                                      const int32_t* row_group, const int32_t* bin_off, const int32_t* bins, int V,
                                      const double* targets, const double* cand, int C, const double* shift_lambda,
                                      const double* slope_lambda, int fixed_slope, int raw, double* loss, ava_stream_t s) {
  return wf_group_loss(spec, dtype, N, F, T, row_src, row_group, bin_off, bins, V, targets, cand, C, 0, shift_lambda,
                       slope_lambda, fixed_slope, raw, loss, s);
}

extern "C" int ava_warpfit_group_pl_loss(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                                         const int32_t* row_group, const int32_t* bin_off, const int32_t* bins, int V,
                                         const double* targets, const double* cand, int C, int K, const double* shift_lambda,
                                         const double* slope_lambda, int fixed_slope, int raw, double* loss, ava_stream_t s) {
  if (!wf_knots_ok(T, K)) return AVA_EINVAL;
  return wf_group_loss(spec, dtype, N, F, T, row_src, row_group, bin_off, bins, V, targets, cand, C, K, shift_lambda,
                       slope_lambda, fixed_slope, raw, loss, s);
}

// mode as in warpfit_group_mean_kernel; max_bins: the longest bin list of the G groups (sizes the grid only)
static int wf_group_mean(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src, const int32_t* group_row_off,
                         const int32_t* bin_off, const int32_t* bins, int G, int max_bins, const double* params, int K,
                         int mode, double* targets, ava_stream_t s) {
  if (spec == nullptr || targets == nullptr || !wf_shape_ok(dtype, N, F, T)) return AVA_EINVAL;
  if (row_src == nullptr || group_row_off == nullptr || bin_off == nullptr || bins == nullptr) return AVA_EINVAL;
  if (G < 1 || max_bins < 1 || (mode != 2 && params == nullptr)) return AVA_EINVAL;
  const WfPlan pl{row_src, nullptr, group_row_off, bin_off, bins, N, F};
  int z = ceil_div(max_bins, 4);
  z = z > 32 ? 32 : z;
  const dim3 grid(G, ceil_div(T, WM_TJ), z);
  if (dtype == 0)
    hipLaunchKernelGGL(warpfit_group_mean_kernel<float>, grid, dim3(256), 0, to_stream(s), static_cast<const float*>(spec), pl,
                       params, T, K, mode, targets);
  else
    hipLaunchKernelGGL(warpfit_group_mean_kernel<double>, grid, dim3(256), 0, to_stream(s), static_cast<const double*>(spec),
                       pl, params, T, K, mode, targets);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_group_mean(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                                      const int32_t* group_row_off, const int32_t* bin_off, const int32_t* bins, int G,
                                      int max_bins, const double* params, int raw, double* targets, ava_stream_t s) {
  if (raw != 0 && raw != 1) return AVA_EINVAL;
  return wf_group_mean(spec, dtype, N, F, T, row_src, group_row_off, bin_off, bins, G, max_bins, params, 2, raw ? 2 : 0,
                       targets, s);
}

extern "C" int ava_warpfit_group_pl_mean(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                                         const int32_t* group_row_off, const int32_t* bin_off, const int32_t* bins, int G,
                                         int max_bins, const double* knots, int K, int raw, double* targets, ava_stream_t s) {
  if ((raw != 0 && raw != 1) || !wf_knots_ok(T, K)) return AVA_EINVAL;
  return wf_group_mean(spec, dtype, N, F, T, row_src, group_row_off, bin_off, bins, G, max_bins, knots, K, raw ? 2 : 1,
                       targets, s);
}
