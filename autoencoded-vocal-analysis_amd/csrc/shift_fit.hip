// The integer-shift time-warp fit on the device: the alignment behind the reference's
// segment_sylls_from_songs (ava/segmenting/template_segmentation.py:455-627), which asks affinewarp's ShiftWarping for
// it.  This is the project's own model (ava_amd/shift_fit.py states it), not affinewarp's code or arithmetic.  Data is
// x [K][F][T] contiguous, fp32 or fp64; all arithmetic is fp64.  Template column t lies at raw column t + s_k, the end
// columns held: aligned[k][f][t] = x[k][f][clip(t + s_k, 0, T-1)].
//
//   shiftfit_partial_kernel  part[chunk][f][t] = sum of x[k][f][clip(t + s_k)] over the chunk's renditions
//   shiftfit_solve_kernel    mbar = (sum of the chunks) / K, then A m[f][:] = mbar[f][:] by a banded LDL^T
//   shiftfit_loss_kernel     loss[k][c] = sum_{f,t} (x[k][f][clip(t + lag_c)] - m[f][t])^2 / (F T): the hot one
//   shiftfit_argmin_kernel   s_k = lag of the least loss (lowest c on ties, NaN never wins) and that loss
//   shiftfit_apply_kernel    aligned, in the input's dtype: exact copies
//
// Lag order: lag_c = 0, -1, +1, -2, +2, ..., -L, +L for c = 0 .. 2 L, so candidate 0 is "no shift" and wins ties.
//
// The template.  K is the long axis (amplitude traces have F = 1), so it is cut into chunks of SF_KC = 128 renditions,
// whatever the grid: chunk j holds k = 128 j .. min(128 j + 127, K - 1).  A thread of the partial kernel owns one (f, t)
// of one chunk and adds its renditions in rising k, starting from 0.0.  The solve kernel adds the chunks in rising j,
// starting from chunk 0's sum, and divides by K once: the bits of mbar depend on (x, s, K) alone.
// A = (1 + l2 / K) I + lambda D2^T D2 is symmetric, positive definite and pentadiagonal and the same for every f, so
// every lane of the solve kernel (one wave per block, a lane per feature row, R rows per block staged in LDS) runs
// the same LDL^T recurrence in registers while it substitutes forward on its own row; lane 0 leaves the two
// sub-diagonals of L in LDS for the backward pass.  No pivoting (A is SPD).  LDS: (2 T + R (T + 1)) 8 bytes, R chosen
// so that this stays under 64000 bytes (R = 1 at T = 2048: 49 KB) and at most 16.
//
// The loss kernel: one workgroup (4 waves) per (rendition, block of SF_LB = 64 lags).  SF rows of x[k] are staged in
// LDS at a time, each with its held end columns written out (L copies of column 0 in front, L of column T-1 behind),
// so a tap is one LDS read at column L + t + lag and nothing is clamped per tap; the same rows of the template lie
// beside them.  A wave owns SF_WL = 16 consecutive lags (16 independent accumulators per lane, the template value read
// once for all of them); lanes walk t = lane, lane + 64, ...: neighbouring lanes read neighbouring LDS columns.
// Summation order of one (k, lag): lane l adds its terms (f, t), t = l mod 64, in rising f and within f in rising t,
// from 0.0; then one xor-shuffle tree (32, 16, .. 1); then one division by F T.  It does not depend on how many rows
// are staged per pass, nor on the lag block: a fixed order, no atomics, two runs give the same bits.  Every term is one
// rounded subtraction and one rounded multiplication, added by a rounded addition (__dsub_rn / __dmul_rn / __dadd_rn:
// -ffp-contract=on must not fuse the product into the running sum).
// LDS per workgroup: SF (2 T + 2 L) 8 bytes with SF = clamp(32768 / ((2 T + 2 L) 8), 1, 8) rows per pass:
// 23.8 KB at T = 155, L = 31 (8 rows, 6 workgroups / CU); 39.3 KB at T = 2048, L = 409 (1 row); never above
// (4 T - 2) 8 = 65520 bytes (L = T - 1 at T = 2048), so the 64 KB a kernel gets without asking is enough.
#include "common.h"

#define SF_MAX_T 2048
#define SF_KC 128        // renditions per chunk of the template's sum
#define SF_WL 16         // lags per wave
#define SF_LB 64         // lags per workgroup
#define SF_MAX_ROWS 8    // rows of x and of the template staged per pass, at most
#define SF_SOLVE_ROWS 16 // feature rows per block of the solve kernel, at most

__device__ __forceinline__ int sf_lag(int c) { return (c & 1) ? -((c + 1) >> 1) : (c >> 1); }

__device__ __forceinline__ int sf_clip(int t, int T) { return t < 0 ? 0 : (t > T - 1 ? T - 1 : t); }

// a shift as the kernels use it: anything outside [-T, T] acts like +-T (every tap on an end column)
__device__ __forceinline__ int sf_shift(int s, int T) { return s < -T ? -T : (s > T ? T : s); }

template <typename T_>
__global__ __launch_bounds__(256) void shiftfit_partial_kernel(const T_* __restrict__ x, const int* __restrict__ shifts, int K,
                                                               int F, int T, double* __restrict__ part) {
  const int64_t FT = (int64_t)F * T;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= FT) return;
  const int f = (int)(e / T), t = (int)(e - (int64_t)f * T);
  const int k0 = blockIdx.y * SF_KC, k1 = k0 + SF_KC < K ? k0 + SF_KC : K;
  double acc = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int c = sf_clip(t + sf_shift(shifts[k], T), T);
    acc = __dadd_rn(acc, (double)x[((size_t)k * F + f) * T + c]);
  }
  part[(size_t)blockIdx.y * FT + e] = acc;
}

// entries of D2^T D2 (D2: the (T-2) x T second differences (1, -2, 1)), T >= 3
__device__ __forceinline__ double sf_diag(int t, int T) { return (double)((t <= T - 3) + 4 * (t >= 1 && t <= T - 2) + (t >= 2)); }
__device__ __forceinline__ double sf_off1(int t, int T) { return -2.0 * (double)((t <= T - 3) + (t >= 1 && t <= T - 2)); }  // (t, t+1)

__global__ __launch_bounds__(64) void shiftfit_solve_kernel(const double* __restrict__ part, int nchunks, int K, int F, int T,
                                                            int R, double a0, double lam, double* __restrict__ mbar,
                                                            double* __restrict__ tmpl) {
  extern __shared__ __align__(16) double sf_sm[];
  const int TS = T + 1;
  double* s_l1 = sf_sm;                                     // L[t][t-1]
  double* s_l2 = s_l1 + T;                                  // L[t][t-2]
  double* s_row = s_l2 + T;                                 // [R][T + 1]
  const int lane = threadIdx.x;
  const int f0 = blockIdx.x * R, nr = F - f0 < R ? F - f0 : R;
  const int64_t FT = (int64_t)F * T;
  for (int e = lane; e < nr * T; e += 64) {
    const int r = e / T, t = e - r * T;
    const size_t g = (size_t)f0 * T + e;
    double s = part[g];
    for (int c = 1; c < nchunks; ++c) s = __dadd_rn(s, part[(size_t)c * FT + g]);
    s = __ddiv_rn(s, (double)K);
    if (mbar != nullptr) mbar[g] = s;
    s_row[r * TS + t] = s;
  }
  __syncthreads();
  const bool act = lane < nr;
  double* row = s_row + (act ? lane : 0) * TS;
  // forward: L z = mbar, w = z / d, with d and the rows of L made on the way (the same in every lane)
  double d1 = 0.0, d2 = 0.0, i1 = 0.0, i2 = 0.0, l1p = 0.0, z1 = 0.0, z2 = 0.0;   // d, 1/d at t-1 and t-2; L[t-1][t-2]; z
  for (int t = 0; t < T; ++t) {
    const double l2t = t >= 2 ? lam * i2 : 0.0;                                   // A[t][t-2] = lam
    const double l1t = t >= 1 ? (lam * sf_off1(t - 1, T) - l2t * l1p * d2) * i1 : 0.0;
    const double d = a0 + lam * sf_diag(t, T) - l1t * l1t * d1 - l2t * l2t * d2;
    const double inv = 1.0 / d;
    if (lane == 0) { s_l1[t] = l1t; s_l2[t] = l2t; }
    if (act) {
      const double z = row[t] - l1t * z1 - l2t * z2;
      row[t] = z * inv;
      z2 = z1; z1 = z;
    }
    d2 = d1; d1 = d; i2 = i1; i1 = inv; l1p = l1t;
  }
  __syncthreads();
  if (act) {                                                // backward: L^T m = w
    double m1 = 0.0, m2 = 0.0;
    for (int t = T - 1; t >= 0; --t) {
      const double l1n = t + 1 < T ? s_l1[t + 1] : 0.0, l2n = t + 2 < T ? s_l2[t + 2] : 0.0;
      const double m = row[t] - l1n * m1 - l2n * m2;
      row[t] = m;
      m2 = m1; m1 = m;
    }
  }
  __syncthreads();
  for (int e = lane; e < nr * T; e += 64) {
    const int r = e / T, t = e - r * T;
    tmpl[(size_t)f0 * T + e] = s_row[r * TS + t];
  }
}

template <typename T_>
__global__ __launch_bounds__(256) void shiftfit_loss_kernel(const T_* __restrict__ x, const double* __restrict__ tmpl, int F,
                                                            int T, int L, int SF, double* __restrict__ loss) {
  extern __shared__ __align__(16) double sf_sm[];
  const int P = T + 2 * L, C = 2 * L + 1;
  double* s_x = sf_sm;                                      // [SF][L + T + L]: column L + t is x[t], the ends held
  double* s_m = s_x + SF * P;                               // [SF][T]
  const int k = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cw = blockIdx.y * SF_LB + wave * SF_WL;         // this wave's first lag
  int off[SF_WL];
#pragma unroll
  for (int j = 0; j < SF_WL; ++j) off[j] = L + (cw + j < C ? sf_lag(cw + j) : 0);
  double acc[SF_WL];
#pragma unroll
  for (int j = 0; j < SF_WL; ++j) acc[j] = 0.0;
  const T_* xk = x + (size_t)k * F * T;
  for (int f0 = 0; f0 < F; f0 += SF) {
    const int nr = F - f0 < SF ? F - f0 : SF;
    __syncthreads();                                        // the previous rows are consumed
    for (int e = tid; e < nr * P; e += 256) {
      const int r = e / P, i = e - r * P;
      s_x[e] = (double)xk[(size_t)(f0 + r) * T + sf_clip(i - L, T)];
    }
    for (int e = tid; e < nr * T; e += 256) s_m[e] = tmpl[(size_t)f0 * T + e];
    __syncthreads();
    if (cw < C) {                                           // wave-uniform
      for (int r = 0; r < nr; ++r) {
        for (int t = lane; t < T; t += 64) {
          const double m = s_m[r * T + t];
          const double* xr = s_x + r * P + t;
#pragma unroll
          for (int j = 0; j < SF_WL; ++j) {
            const double d = __dsub_rn(xr[off[j]], m);
            acc[j] = __dadd_rn(acc[j], __dmul_rn(d, d));
          }
        }
      }
    }
  }
  const double ft = (double)F * (double)T;
#pragma unroll
  for (int j = 0; j < SF_WL; ++j) {
    if (cw + j >= C) continue;                              // wave-uniform
    const double tot = wave_sum_d(acc[j]);
    if (lane == 0) loss[(size_t)k * C + cw + j] = __ddiv_rn(tot, ft);
  }
}

// one wave per rendition: lanes take candidates lane, lane + 64, ... in rising order, then a (loss, index) min over the
// wave; the tie rule of warpfit_argmin_kernel
__global__ __launch_bounds__(256) void shiftfit_argmin_kernel(const double* __restrict__ loss, int K, int C,
                                                              int* __restrict__ shifts, double* __restrict__ best_loss) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  double bv = 0.0;
  int bi = -1;                                              // -1: nothing but NaN seen
  for (int c = lane; c < C; c += 64) {
    const double v = loss[(size_t)k * C + c];
    if (v == v && (bi < 0 || v < bv)) { bv = v; bi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi >= 0 && (bi < 0 || ov < bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
  }
  const int c = bi < 0 ? 0 : bi;                            // all NaN: no shift, and its NaN
  if (lane == 0) {
    shifts[k] = sf_lag(c);
    if (best_loss != nullptr) best_loss[k] = loss[(size_t)k * C + c];
  }
}

template <typename T_>
__global__ __launch_bounds__(256) void shiftfit_apply_kernel(const T_* __restrict__ x, const int* __restrict__ shifts, int F,
                                                             int T, T_* __restrict__ out) {
  const int k = blockIdx.x;
  const int s = sf_shift(shifts[k], T);
  for (int f = blockIdx.y; f < F; f += gridDim.y) {
    const T_* row = x + ((size_t)k * F + f) * T;
    for (int t = threadIdx.x; t < T; t += 256) out[((size_t)k * F + f) * T + t] = row[sf_clip(t + s, T)];
  }
}

static bool sf_shape_ok(int dtype, int K, int F, int T) {
  return (dtype == 0 || dtype == 1) && K >= 1 && F >= 1 && T >= 3 && T <= SF_MAX_T && (int64_t)F * T <= 2147483647 / 2;
}

static int sf_chunks(int K) { return ceil_div(K, SF_KC); }

static int sf_loss_rows(int T, int L) {
  const int rows = 32768 / ((2 * T + 2 * L) * (int)sizeof(double));
  return rows < 1 ? 1 : (rows > SF_MAX_ROWS ? SF_MAX_ROWS : rows);
}

static int sf_solve_rows(int F, int T) {
  int rows = (8000 - 2 * T) / (T + 1);
  rows = rows < 1 ? 1 : (rows > SF_SOLVE_ROWS ? SF_SOLVE_ROWS : rows);
  return rows < F ? rows : F;
}

extern "C" int ava_shiftfit_max_t(void) { return SF_MAX_T; }

extern "C" size_t ava_shiftfit_workspace_bytes(int K, int F, int T) {
  if (!sf_shape_ok(0, K, F, T)) return 0;
  return (size_t)sf_chunks(K) * F * T * sizeof(double) + 256;
}

extern "C" int ava_shiftfit_template(const void* x, int dtype, int K, int F, int T, const int32_t* shifts,
                                     double smoothness, double l2, double* mbar, double* tmpl, void* ws, size_t ws_bytes,
                                     ava_stream_t s) {
  if (x == nullptr || shifts == nullptr || tmpl == nullptr || ws == nullptr || !sf_shape_ok(dtype, K, F, T)) return AVA_EINVAL;
  if (!(smoothness >= 0.0) || !(l2 >= 0.0) || smoothness > 1.7976931348623157e308 || l2 > 1.7976931348623157e308) return AVA_EINVAL;
  const int nchunks = sf_chunks(K);
  if (nchunks > 65535) return AVA_EINVAL;
  double* part = reinterpret_cast<double*>(ava_align256(ws));
  if (reinterpret_cast<char*>(part) + (size_t)nchunks * F * T * sizeof(double) > static_cast<char*>(ws) + ws_bytes) return AVA_EWORKSPACE;
  const int64_t FT = (int64_t)F * T;
  const dim3 grid((unsigned)ceil_div64(FT, 256), nchunks);
  if (dtype == 0)
    hipLaunchKernelGGL(shiftfit_partial_kernel<float>, grid, dim3(256), 0, to_stream(s), static_cast<const float*>(x), shifts, K,
                       F, T, part);
  else
    hipLaunchKernelGGL(shiftfit_partial_kernel<double>, grid, dim3(256), 0, to_stream(s), static_cast<const double*>(x), shifts,
                       K, F, T, part);
  AVA_CHECK_LAUNCH();
  const int R = sf_solve_rows(F, T);
  const size_t lds = ((size_t)2 * T + (size_t)R * (T + 1)) * sizeof(double);
  hipLaunchKernelGGL(shiftfit_solve_kernel, dim3(ceil_div(F, R)), dim3(64), lds, to_stream(s), part, nchunks, K, F, T, R,
                     1.0 + l2 / (double)K, smoothness, mbar, tmpl);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_shiftfit_loss(const void* x, int dtype, int K, int F, int T, const double* tmpl, int L, double* loss,
                                 ava_stream_t s) {
  if (x == nullptr || tmpl == nullptr || loss == nullptr || !sf_shape_ok(dtype, K, F, T) || L < 0 || L > T - 1) return AVA_EINVAL;
  const int SF = sf_loss_rows(T, L);
  const size_t lds = (size_t)SF * (2 * T + 2 * L) * sizeof(double);
  const dim3 grid(K, ceil_div(2 * L + 1, SF_LB));
  if (dtype == 0)
    hipLaunchKernelGGL(shiftfit_loss_kernel<float>, grid, dim3(256), lds, to_stream(s), static_cast<const float*>(x), tmpl, F, T,
                       L, SF, loss);
  else
    hipLaunchKernelGGL(shiftfit_loss_kernel<double>, grid, dim3(256), lds, to_stream(s), static_cast<const double*>(x), tmpl, F,
                       T, L, SF, loss);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_shiftfit_argmin(const double* loss, int K, int L, int32_t* shifts, double* best_loss, ava_stream_t s) {
  if (loss == nullptr || shifts == nullptr || K < 1 || L < 0 || L > SF_MAX_T - 1) return AVA_EINVAL;
  hipLaunchKernelGGL(shiftfit_argmin_kernel, dim3(ceil_div(K, 4)), dim3(256), 0, to_stream(s), loss, K, 2 * L + 1, shifts,
                     best_loss);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_shiftfit_apply(const void* x, int dtype, int K, int F, int T, const int32_t* shifts, void* out,
                                  ava_stream_t s) {
  if (x == nullptr || shifts == nullptr || out == nullptr || !sf_shape_ok(dtype, K, F, T)) return AVA_EINVAL;
  const dim3 grid(K, F < 64 ? F : 64);
  if (dtype == 0)
    hipLaunchKernelGGL(shiftfit_apply_kernel<float>, grid, dim3(256), 0, to_stream(s), static_cast<const float*>(x), shifts, F, T,
                       static_cast<float*>(out));
  else
    hipLaunchKernelGGL(shiftfit_apply_kernel<double>, grid, dim3(256), 0, to_stream(s), static_cast<const double*>(x), shifts, F,
                       T, static_cast<double*>(out));
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
