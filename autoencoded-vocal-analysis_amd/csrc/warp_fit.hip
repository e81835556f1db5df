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
// is wf_pos(u_0, s_0, j).  A candidate with some s_k <= 0 has loss +inf.  The penalties are shift_l u_0^2 + slope_l
// mean_k (log s_k)^2.
//
// The two warps are two models, WfAffine and WfKnots: how a candidate or a fitted warp is read, where column j reads the
// source, what is added to a finished sum.  The apply, loss and grouped kernels are templates over the model and nothing
// else in them knows which warp it is: the LDS, the staging, the sums (wf_block_sums) and their order exist once.
//
//   warpfit_apply_kernel<T, Model>   under (shift, slope) [N][2] or knots [N][K]
//   warpfit_loss_kernel<T, Model>    candidates [N][C][2] or [N][C][K]
//   warpfit_pl_candidates_kernel     candidates [N][C][K] around u [N][K]: one knot, or all knots together, moved by 0, -h, +h, ...
//   warpfit_argmin_kernel            serves both fits: its parameter width is 2 or K
//
// The grouped fits (row f17): many fit problems over the same spec in one launch.  A group is a sorted list of motifs, a
// sorted list of bins and two lambdas of its own; a virtual row is one (motif, group) pair (struct WfPlan).
//
//   warpfit_group_loss_kernel<T, Model>   warpfit_loss_kernel per virtual row: the motif, the target, the bins and the
//                                         lambdas come through the plan, the bins are staged through their list in list
//                                         order, and everything else is wf_loss_body, the plain kernel's body, so a virtual
//                                         row's losses have the bits of the plain kernel on the gathered tensor
//   warpfit_group_mean_kernel<T, Model>   every group's mean warped motif without the warped motifs: the apply kernel's
//                                         values, summed over the group's rows in rising order
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

// The two warp models.  A model is one warp: warp(p, i, K) is warp i of the fitted parameters p, candidate(cand, c, K,
// fixed_slope) is candidate c of a search; pos(j, T, K, fixed_slope) is the source position of column j (fixed_slope: the
// shift objective, every slope 1) and penalised(tot, ...) the finished sum of squares plus the model's penalties.  Every
// kernel below that warps is written once over the model; the operations inside a model, and their order, are the
// objective's definition and the tests hold them to the bit.
//
// Shift and slope.  A candidate is (shift, log slope), a fitted warp (shift, slope).  The loss body holds shift and
// log slope in registers across its sums for the penalties; the slope is dead once the tables are written.
struct WfAffine {
  double shift, ls, slope;
  static __device__ __forceinline__ int width(int) { return 2; }
  static __device__ __forceinline__ WfAffine warp(const double* __restrict__ p, size_t i, int) {
    return {p[2 * i], 0.0, p[2 * i + 1]};
  }
  static __device__ __forceinline__ WfAffine candidate(const double* __restrict__ cand, size_t c, int, int fixed_slope) {
    const double ls = cand[2 * c + 1];
    return {cand[2 * c], ls, fixed_slope ? 1.0 : exp(ls)};
  }
  __device__ __forceinline__ double pos(int j, int, int, int) const { return wf_pos(shift, slope, j); }
  // loss + shift_l * x[0]**2 + slope_l * x[1]**2, left to right
  __device__ __forceinline__ double penalised(double tot, double shift_lambda, double slope_lambda, int fixed_slope, int,
                                              int) const {
    tot = __dadd_rn(tot, __dmul_rn(shift_lambda, __dmul_rn(shift, shift)));
    if (!fixed_slope) tot = __dadd_rn(tot, __dmul_rn(slope_lambda, __dmul_rn(ls, ls)));
    return tot;
  }
};

// K knots.  The model keeps a pointer: a lane reads the two knots of its column's segment from memory, K <= 16 doubles
// that stay in cache, and the penalty re-reads them after the sums.  fixed_slope: the positions are u_0 + j.  Crossed
// knots do not stop the sums -- wf_tap keeps every tap inside the row -- and the total is replaced by +inf.
struct WfKnots {
  const double* u;
  static __device__ __forceinline__ int width(int K) { return K; }
  static __device__ __forceinline__ WfKnots warp(const double* __restrict__ p, size_t i, int K) { return {p + i * K}; }
  static __device__ __forceinline__ WfKnots candidate(const double* __restrict__ cand, size_t c, int K, int) {
    return {cand + c * K};
  }
  __device__ __forceinline__ double pos(int j, int T, int K, int fixed_slope) const {
    return fixed_slope ? wf_pos(u[0], 1.0, j) : wf_pl_pos(u, j, T, K);
  }
  // loss + shift_l u_0^2 + slope_l mean_k (log s_k)^2
  __device__ __forceinline__ double penalised(double tot, double shift_lambda, double slope_lambda, int fixed_slope, int T,
                                              int K) const {
    tot = __dadd_rn(tot, __dmul_rn(shift_lambda, __dmul_rn(u[0], u[0])));
    if (fixed_slope) return tot;
    double sq = 0.0;                                        // sum_k (log s_k)^2, k = 0, 1, ...
    bool crossed = false;
    for (int i = 0; i < K - 1; ++i) {
      const double sl = wf_pl_slope(u, i, T, K);
      crossed |= sl <= 0.0;
      const double l = log(sl);
      sq = __dadd_rn(sq, __dmul_rn(l, l));
    }
    tot = __dadd_rn(tot, __dmul_rn(slope_lambda, __ddiv_rn(sq, (double)(K - 1))));
    return crossed ? __builtin_inf() : tot;
  }
};

// params: (shift, slope) [N][2] or knots [N][K]
template <typename T_, typename Model>
__global__ __launch_bounds__(256) void warpfit_apply_kernel(const T_* __restrict__ spec, const double* __restrict__ params,
                                                            int F, int T, int K, T_* __restrict__ out) {
  const int n = blockIdx.x;
  const Model m = Model::warp(params, n, K);
  for (int j = threadIdx.x; j < T; j += 256) {
    const WfTap t = wf_tap(m.pos(j, T, K, 0), T);
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

// The loss of one (motif, candidate block) under either model: the body of warpfit_loss_kernel and of its grouped form.
// cand: the motif's candidates [C][Model::width(K)].  raw (grouped only): the tables are lo = j, w = 0, the unwarped row
// read exactly, no candidate is read (cand may be null) and no penalty added.
template <typename T_, typename Model, bool G>
__device__ __forceinline__ void wf_loss_body(const T_* __restrict__ motif, const double* __restrict__ target,
                                             const int* __restrict__ bins, int Fall, const double* __restrict__ cand, int F,
                                             int T, int C, int K, double shift_lambda, double slope_lambda, int fixed_slope,
                                             int raw, double* __restrict__ loss) {
  extern __shared__ __align__(16) double wf_sm[];
  const int TS = T + 1;
  double* s_spec = wf_sm;                                   // [WF_FR][T + 1], column T repeats column T-1
  double* s_tgt = s_spec + WF_FR * TS;                      // [WF_FR][T]
  double* s_w = s_tgt + WF_FR * T;                          // [WF_CB][T]
  int* s_lo = reinterpret_cast<int*>(s_w + WF_CB * T);      // [WF_CB][T]
  const int c0 = blockIdx.y * WF_CB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  Model m[2] = {};
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
      m[k] = Model::candidate(cand, c, K, fixed_slope);
      for (int j = lane; j < T; j += 64) {
        const WfTap t = wf_tap(m[k].pos(j, T, K, fixed_slope), T);
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
    if (!(G && raw)) tot = m[k].penalised(tot, shift_lambda, slope_lambda, fixed_slope, T, K);
    if (lane == 0) loss[c] = tot;
  }
}

// loss[n][c] of spec [N][F][T] against one target [F][T]; cand [N][C][width]
template <typename T_, typename Model>
__global__ __launch_bounds__(256) void warpfit_loss_kernel(const T_* __restrict__ spec, const double* __restrict__ target,
                                                           const double* __restrict__ cand, int F, int T, int C, int K,
                                                           double shift_lambda, double slope_lambda, int fixed_slope,
                                                           double* __restrict__ loss) {
  const int n = blockIdx.x;
  wf_loss_body<T_, Model, false>(spec + (size_t)n * F * T, target, nullptr, F, cand + (size_t)n * C * Model::width(K), F, T, C,
                                 K, shift_lambda, slope_lambda, fixed_slope, 0, loss + (size_t)n * C);
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
// is the plain kernel's, operation for operation; cand [V][C][width], loss [V][C]
template <typename T_, typename Model>
__global__ __launch_bounds__(256) void warpfit_group_loss_kernel(const T_* __restrict__ spec, WfPlan pl,
                                                                 const double* __restrict__ targets,
                                                                 const double* __restrict__ cand, int T, int C, int K,
                                                                 const double* __restrict__ shift_lambda,
                                                                 const double* __restrict__ slope_lambda, int fixed_slope,
                                                                 int raw, double* __restrict__ loss) {
  const int v = blockIdx.x, g = pl.row_group[v], n = pl.row_src[v];
  if ((unsigned)n >= (unsigned)pl.N) return;                // a broken plan reads nothing
  const int b0 = pl.bin_off[g], F = pl.bin_off[g + 1] - b0;
  wf_loss_body<T_, Model, true>(spec + (size_t)n * pl.Fall * T, targets + (size_t)b0 * T, pl.bins + b0, pl.Fall,
                                raw ? nullptr : cand + (size_t)v * C * Model::width(K), F, T, C, K,
                                raw ? 0.0 : shift_lambda[g], (raw || fixed_slope) ? 0.0 : slope_lambda[g], fixed_slope, raw,
                                loss + (size_t)v * C);
}

// The grouped template (row f17): target_g[f][j] = sum over the group's rows, in rising order, of the value the apply
// kernels would store for that row -- interpolated under the row's own parameters and rounded to spec's dtype -- divided
// by the row count: warpfit_mean_kernel of warpfit_apply_kernel's output without that output.  One workgroup per (group,
// WM_TJ columns, share of the bins): WM_TR rows at a time, a row's tap for a column is computed once into LDS and then
// used for every bin of the workgroup's share; thread (column, bin lane) carries the running sum of its (bin, column)
// cells from one row set to the next through the target itself, which only that thread touches.  fp64, a fixed order,
// no atomics.  params [V][2] = (shift, slope) or knots [V][K], by the model; raw: no warp at all but the unwarped value,
// which an identity warp does not reproduce bit for bit, and params is not read.
#define WM_TJ 64
#define WM_TR 16
template <typename T_, typename Model>
__global__ __launch_bounds__(256) void warpfit_group_mean_kernel(const T_* __restrict__ spec, WfPlan pl,
                                                                 const double* __restrict__ params, int T, int K, int raw,
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
    if (!raw) {
      for (int e = threadIdx.x; e < nr * WM_TJ; e += 256) {
        const int r = e >> 6, jj = j0 + (e & (WM_TJ - 1));
        if (jj >= T) continue;
        const WfTap t = wf_tap(Model::warp(params, (size_t)(v0 + r0 + r), K).pos(jj, T, K, 0), T);
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
          if (raw) {
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

static bool wf_knots_ok(int T, int K) { return K >= 2 && K <= WF_MAX_K && T - 1 >= 2 * (K - 1); }

static size_t wf_loss_lds(int T) {
  return ((size_t)WF_FR * (T + 1) + (size_t)WF_FR * T + (size_t)WF_CB * T) * sizeof(double) + (size_t)WF_CB * T * sizeof(int);
}

extern "C" int ava_warpfit_max_t(void) { return WF_MAX_T; }
extern "C" int ava_warpfit_max_knots(void) { return WF_MAX_K; }

// ---- apply, mean, candidates, argmin -------------------------------------------------------------------------------------

template <typename Model>
static int wf_apply(const void* spec, int dtype, int N, int F, int T, const double* params, int K, void* out, ava_stream_t s) {
  const dim3 grid(N, F < 64 ? F : 64);
  if (dtype == 0)
    hipLaunchKernelGGL((warpfit_apply_kernel<float, Model>), grid, dim3(256), 0, to_stream(s), static_cast<const float*>(spec),
                       params, F, T, K, static_cast<float*>(out));
  else
    hipLaunchKernelGGL((warpfit_apply_kernel<double, Model>), grid, dim3(256), 0, to_stream(s),
                       static_cast<const double*>(spec), params, F, T, K, static_cast<double*>(out));
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_apply(const void* spec, int dtype, int N, int F, int T, const double* params, void* out,
                                 ava_stream_t s) {
  if (spec == nullptr || params == nullptr || out == nullptr || !wf_shape_ok(dtype, N, F, T)) return AVA_EINVAL;
  return wf_apply<WfAffine>(spec, dtype, N, F, T, params, 2, out, s);
}

extern "C" int ava_warpfit_pl_apply(const void* spec, int dtype, int N, int F, int T, const double* knots, int K, void* out,
                                    ava_stream_t s) {
  if (spec == nullptr || knots == nullptr || out == nullptr || !wf_shape_ok(dtype, N, F, T) || !wf_knots_ok(T, K)) return AVA_EINVAL;
  return wf_apply<WfKnots>(spec, dtype, N, F, T, knots, K, out, s);
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

extern "C" int ava_warpfit_pl_argmin(const double* loss, const double* cand, int N, int C, int K, int32_t* best, double* u,
                                     double* best_loss, ava_stream_t s) {
  if (K < 2 || K > WF_MAX_K) return AVA_EINVAL;
  return wf_launch_argmin(loss, cand, N, C, K, best, u, best_loss, s);
}

// ---- the losses ----------------------------------------------------------------------------------------------------------

// Every loss launch: `kernel` over (rows, blocks of WF_CB candidates).  Dynamic LDS over 64 KB (T > 409) has to be asked
// for, per device; asked whenever it is needed rather than once per process, so that neither a second device nor two
// threads' first calls can miss it.
template <typename... P, typename... A>
static int wf_launch_loss(void (*kernel)(P...), int rows, int T, int C, ava_stream_t s, A... args) {
  if (wf_loss_lds(T) > 65536 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)wf_loss_lds(WF_MAX_T)) != hipSuccess)
    return AVA_ELAUNCH;
  hipLaunchKernelGGL(kernel, dim3(rows, ceil_div(C, WF_CB)), dim3(256), wf_loss_lds(T), to_stream(s), args...);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <typename Model>
static int wf_loss(const void* spec, int dtype, int N, int F, int T, const double* target, const double* cand, int C, int K,
                   double shift_lambda, double slope_lambda, double* loss, ava_stream_t s) {
  if (spec == nullptr || target == nullptr || cand == nullptr || loss == nullptr || !wf_shape_ok(dtype, N, F, T)) return AVA_EINVAL;
  if (C < 1 || C > WF_MAX_C || shift_lambda != shift_lambda || slope_lambda != slope_lambda) return AVA_EINVAL;
  const int fixed = slope_lambda > 1.7976931348623157e308;  // +inf: the shift objective
  if (fixed) slope_lambda = 0.0;
  if (dtype == 0)
    return wf_launch_loss(&warpfit_loss_kernel<float, Model>, N, T, C, s, static_cast<const float*>(spec), target, cand, F, T, C,
                          K, shift_lambda, slope_lambda, fixed, loss);
  return wf_launch_loss(&warpfit_loss_kernel<double, Model>, N, T, C, s, static_cast<const double*>(spec), target, cand, F, T, C,
                        K, shift_lambda, slope_lambda, fixed, loss);
}

extern "C" int ava_warpfit_loss(const void* spec, int dtype, int N, int F, int T, const double* target, const double* cand,
                                int C, double shift_lambda, double slope_lambda, double* loss, ava_stream_t s) {
  return wf_loss<WfAffine>(spec, dtype, N, F, T, target, cand, C, 2, shift_lambda, slope_lambda, loss, s);
}

extern "C" int ava_warpfit_pl_loss(const void* spec, int dtype, int N, int F, int T, const double* target, const double* cand,
                                   int C, int K, double shift_lambda, double slope_lambda, double* loss, ava_stream_t s) {
  if (!wf_knots_ok(T, K)) return AVA_EINVAL;
  return wf_loss<WfKnots>(spec, dtype, N, F, T, target, cand, C, K, shift_lambda, slope_lambda, loss, s);
}

// ---- the grouped fits (row f17) -----------------------------------------------------------------------------------------

template <typename Model>
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
    return wf_launch_loss(&warpfit_group_loss_kernel<float, Model>, V, T, C, s, static_cast<const float*>(spec), pl, targets,
                          cand, T, C, K, shift_lambda, slope_lambda, fixed_slope, raw, loss);
  return wf_launch_loss(&warpfit_group_loss_kernel<double, Model>, V, T, C, s, static_cast<const double*>(spec), pl, targets,
                        cand, T, C, K, shift_lambda, slope_lambda, fixed_slope, raw, loss);
}

extern "C" int ava_warpfit_group_loss(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                                      const int32_t* row_group, const int32_t* bin_off, const int32_t* bins, int V,
                                      const double* targets, const double* cand, int C, const double* shift_lambda,
                                      const double* slope_lambda, int fixed_slope, int raw, double* loss, ava_stream_t s) {
  return wf_group_loss<WfAffine>(spec, dtype, N, F, T, row_src, row_group, bin_off, bins, V, targets, cand, C, 2, shift_lambda,
                                 slope_lambda, fixed_slope, raw, loss, s);
}

extern "C" int ava_warpfit_group_pl_loss(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                                         const int32_t* row_group, const int32_t* bin_off, const int32_t* bins, int V,
                                         const double* targets, const double* cand, int C, int K, const double* shift_lambda,
                                         const double* slope_lambda, int fixed_slope, int raw, double* loss, ava_stream_t s) {
  if (!wf_knots_ok(T, K)) return AVA_EINVAL;
  return wf_group_loss<WfKnots>(spec, dtype, N, F, T, row_src, row_group, bin_off, bins, V, targets, cand, C, K, shift_lambda,
                                slope_lambda, fixed_slope, raw, loss, s);
}

// max_bins: the longest bin list of the G groups (sizes the grid only)
template <typename Model>
static int wf_group_mean(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src, const int32_t* group_row_off,
                         const int32_t* bin_off, const int32_t* bins, int G, int max_bins, const double* params, int K,
                         int raw, double* targets, ava_stream_t s) {
  if (spec == nullptr || targets == nullptr || !wf_shape_ok(dtype, N, F, T) || (raw != 0 && raw != 1)) return AVA_EINVAL;
  if (row_src == nullptr || group_row_off == nullptr || bin_off == nullptr || bins == nullptr) return AVA_EINVAL;
  if (G < 1 || max_bins < 1 || (!raw && params == nullptr)) return AVA_EINVAL;
  const WfPlan pl{row_src, nullptr, group_row_off, bin_off, bins, N, F};
  int z = ceil_div(max_bins, 4);
  z = z > 32 ? 32 : z;
  const dim3 grid(G, ceil_div(T, WM_TJ), z);
  if (dtype == 0)
    hipLaunchKernelGGL((warpfit_group_mean_kernel<float, Model>), grid, dim3(256), 0, to_stream(s),
                       static_cast<const float*>(spec), pl, params, T, K, raw, targets);
  else
    hipLaunchKernelGGL((warpfit_group_mean_kernel<double, Model>), grid, dim3(256), 0, to_stream(s),
                       static_cast<const double*>(spec), pl, params, T, K, raw, targets);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_warpfit_group_mean(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                                      const int32_t* group_row_off, const int32_t* bin_off, const int32_t* bins, int G,
                                      int max_bins, const double* params, int raw, double* targets, ava_stream_t s) {
  return wf_group_mean<WfAffine>(spec, dtype, N, F, T, row_src, group_row_off, bin_off, bins, G, max_bins, params, 2, raw,
                                 targets, s);
}

extern "C" int ava_warpfit_group_pl_mean(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                                         const int32_t* group_row_off, const int32_t* bin_off, const int32_t* bins, int G,
                                         int max_bins, const double* knots, int K, int raw, double* targets, ava_stream_t s) {
  if (!wf_knots_ok(T, K)) return AVA_EINVAL;
  return wf_group_mean<WfKnots>(spec, dtype, N, F, T, row_src, group_row_off, bin_off, bins, G, max_bins, knots, K, raw,
                                targets, s);
}
