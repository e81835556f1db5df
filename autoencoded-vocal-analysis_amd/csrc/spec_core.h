// get_spec (ava/preprocessing/utils.py:77-108) after the transform, shared by the shotgun spectrograms (spec.hip,
// SURVEY.md section 8 row f4) and the warped windows out of the motif cache (warp_spec.hip, row f9): the linear
// B-spline basis of a target time / frequency in FITPACK's order, the four-term sum, interp2d's fill rule, the
// normalisation and clip, within_syll_normalize -- and the ONE interpolation kernel, normalise kernel, argument check
// and launcher that run them.  The two rows differ only in where a window's frame count, frame times and log-magnitude
// coefficients are stored (a "coefficient source", below), so a window cut from the cache and the same window
// transformed on its own are the same bits.  Also the argument block of spec.hip's first two stages and their host
// launcher, which warp_spec.hip runs once per file.
#pragma once
#include "stft.h"

#define AVA_SPEC_EPS 1e-12
#define AVA_SPEC_ROWS 16         // frequency rows of one window a workgroup of the interpolation owns
#define AVA_SPEC_TMAX 512        // target times per window the column table holds (num_time_bins; larger: AVA_EINVAL)
#define AVA_SPEC_NORM_T 1024

struct SpecMeta {        // one per window, written by spec_prep_kernel
  long long lo;          // first sample of the slice inside the concatenated audio buffer
  int n;                 // samples in the slice
  int nframes;           // STFT frames (0: the reference returns zeros for this window; -1: scratch too small)
  int j0, j1;            // frames the interpolation can touch (inclusive): the others are never computed
  double mean;           // subtracted DC offset (0 when remove_dc_offset is off)
  double t_shift;        // max(0, t1)
};

struct SpecOut {          // the output half: what runs after the transform, whichever source the coefficients come from
  const double* target_times;    // [n][T]
  const double* target_freqs;    // [F]
  float* out;                    // [n][F][T]
  float* out_max;                // [n] or null
  double* vals;                  // [n][F*T]: clipped fp64 spectrograms handed to spec_normalize_kernel (normalize only)
  double q_gamma;                // within_syll_normalize: np.quantile's interpolation weight ...
  int q_lo, normalize;           // ... between the order statistics q_lo and q_lo + 1 (0-based)
  double fs, spec_min, range, fill_value, fbin;    // fbin: rfftfreq's 1 / (nperseg * (1 / fs))
  int n, nperseg, nstep, F, T;
};

struct SpecCoef { double t0f0, t0f1, t1f0, t1f1; };   // log-magnitudes at time l / l + 1 (t0 / t1), frequency q / q + 1 (f0 / f1)

// A coefficient source is an argument block derived from SpecOut with  window(w) -> a handle of window w  that holds
//   nframes         its frame count (0: get_spec returns zeros, utils.py:68-69; -1: NaN marker)
//   ftimes          its nframes frame times
//   coef(l, q)      the SpecCoef of knot interval (l, q)
// SpecArgs: the per-window scratch [window][frame][bin] the transform of spec.hip fills.
struct SpecScratchWindow {
  int nframes;
  const double* ftimes;
  const double* logmag;          // [frame][K]
  int K;
#ifdef __HIPCC__
  __device__ __forceinline__ SpecCoef coef(int l, int q) const {
    const double* c0 = logmag + (size_t)l * K + q;
    const double* c1 = c0 + K;
    return {c0[0], c0[1], c1[0], c1[1]};
  }
#endif
};

struct SpecArgs : SpecOut {
  const void* audio;
  const long long* file_off;
  const long long* file_len;
  const int* file_idx;
  const double* t1;
  const double* t2;
  const double* window;          // [nperseg]
  SpecMeta* meta;
  double* twiddle;               // [nperseg/2][2]: exp(-2 pi i k / nperseg), written by spec_prep_kernel's workgroup 0
  double* ftimes;                // [n][maxframes]: frame times of each window, written by spec_prep_kernel
  int* krange;                   // [2]: first / last frequency bin the target frequencies can touch (workgroup 0)
  double* logmag;                // [n][maxframes][nperseg/2 + 1]
  double scale;
  int maxframes, dtype, remove_dc;
#ifdef __HIPCC__
  __device__ __forceinline__ SpecScratchWindow window_of(int w) const {
    const int K = nperseg / 2 + 1;
    return {meta[w].nframes, ftimes + (size_t)w * maxframes, logmag + (size_t)w * maxframes * K, K};
  }
#endif
};

// spec.hip: STFT frames of max_samples samples; the shapes its kernels take; the bytes of the scratch regions
// spec_launch_frames fills (krange, meta, twiddle, ftimes, logmag, in the order ava_get_spec_batch lays them out); and
// spec_prep_kernel + the transform of every window's needed frames on stream st (AVA_OK or AVA_ELAUNCH).
int spec_frames_for(int max_samples, int nstep);
bool spec_shape_ok(int nperseg, int noverlap);
void spec_carve(SpecArgs& a, void* ws, int n, int max_samples, int nperseg, int noverlap);
int spec_launch_frames(const SpecArgs& a, hipStream_t st);

// The output half of an entry point's arguments: AVA_EINVAL for the ones ava_get_spec_batch and ava_warp_windows both
// refuse (null pointers, n, F, T, T > AVA_SPEC_TMAX, spec_max == spec_min, the quantile of normalize), else fills
// every field of o but vals (the caller's workspace) and returns AVA_OK.  Nothing is launched.
int spec_out_args(SpecOut& o, const double* target_times, const double* target_freqs, float* out, float* out_max, int n,
                  int F, int T, double fs, int nperseg, int noverlap, double spec_min, double spec_max, double fill_value,
                  int normalize, int q_lo, double q_gamma);

// rfftfreq's bin width 1 / (n d), d = 1 / fs: host IEEE arithmetic, the very operations of scipy.fft.rfftfreq
static inline double spec_fbin(int nperseg, double fs) { return 1.0 / ((double)nperseg * (1.0 / fs)); }

// first / last bin target frequencies in [mnf, mxf] can touch (+- 2 of slack), clamped to 0 .. nperseg / 2
__host__ __device__ __forceinline__ void spec_bin_range(double mnf, double mxf, double fbin, int nperseg, int* k0, int* k1) {
  const int K1 = nperseg / 2;
  const double b0 = floor(mnf / fbin) - 2.0, b1 = floor(mxf / fbin) + 3.0;
  *k0 = b0 > 0.0 ? (b0 < (double)K1 ? (int)b0 : K1) : 0;
  *k1 = b1 < (double)K1 ? (b1 > 0.0 ? (int)b1 : 0) : K1;
}

#ifdef __HIPCC__
// Knot interval l (frames l, l + 1; -1: outside the frame times or NaN -> fill value) and the two basis values of target
// time x over the nframes frame times ft (fpbspl: h0 = f (t[l+1] - x), h1 = f (x - t[l]), f = 1 / (t[l+1] - t[l])).
__device__ __forceinline__ void spec_time_basis(double x, const double* ft, int nframes, double fs, int nstep, int* lo,
                                                double* h0, double* h1) {
  const double xmin = ft[0], xmax = ft[nframes - 1];
  int l = -1;
  double hx0 = 0.0, hx1 = 0.0;
  if (!(x < xmin || x > xmax || !(x == x))) {
    l = (int)floor((x - xmin) * fs / (double)nstep);
    l = l < 0 ? 0 : (l > nframes - 2 ? nframes - 2 : l);
    while (l > 0 && x < ft[l]) --l;
    while (l < nframes - 2 && x >= ft[l + 1]) ++l;
    const double tl = ft[l], tr = ft[l + 1];
    const double fx = __ddiv_rn(1.0, __dsub_rn(tr, tl));
    hx0 = __dmul_rn(fx, __dsub_rn(tr, x));
    hx1 = __dmul_rn(fx, __dsub_rn(x, tl));
  }
  *lo = l; *h0 = hx0; *h1 = hx1;
}

// The same for target frequency y over the K bin frequencies k * val (val: spec_fbin)
__device__ __forceinline__ void spec_freq_basis(double y, double val, int K, int* qo, double* h0, double* h1) {
  const double ymax = __dmul_rn((double)(K - 1), val);
  int q = -1;
  double hy0 = 0.0, hy1 = 0.0;
  if (!(y < 0.0 || y > ymax || !(y == y))) {
    q = (int)floor(y / val);
    q = q < 0 ? 0 : (q > K - 2 ? K - 2 : q);
    while (q > 0 && y < __dmul_rn((double)q, val)) --q;
    while (q < K - 2 && y >= __dmul_rn((double)(q + 1), val)) ++q;
    const double yl = __dmul_rn((double)q, val), yr = __dmul_rn((double)(q + 1), val);
    const double fy = __ddiv_rn(1.0, __dsub_rn(yr, yl));
    hy0 = __dmul_rn(fy, __dsub_rn(yr, y));
    hy1 = __dmul_rn(fy, __dsub_rn(y, yl));
  }
  *qo = q; *h0 = hy0; *h1 = hy1;
}

// fpbisp: sum over x then y of (c * hx) * hy; cXY is the coefficient at time l + X, frequency q + Y
__device__ __forceinline__ double spec_bilinear(double c00, double c01, double c10, double c11, double hx0, double hx1,
                                                double hy0, double hy1) {
  double sp = 0.0;
  sp = __dadd_rn(sp, __dmul_rn(__dmul_rn(c00, hx0), hy0));
  sp = __dadd_rn(sp, __dmul_rn(__dmul_rn(c01, hx0), hy1));
  sp = __dadd_rn(sp, __dmul_rn(__dmul_rn(c10, hx1), hy0));
  sp = __dadd_rn(sp, __dmul_rn(__dmul_rn(c11, hx1), hy1));
  return sp;
}

// utils.py:101-103: (x - min) / (max - min), clip to [0, 1]
__device__ __forceinline__ double spec_scale_clip(double v, double spec_min, double range) {
  v = __dsub_rn(v, spec_min);
  v = __ddiv_rn(v, range);
  return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

// within_syll_normalize (utils.py:104-108) of one window by one workgroup of AVA_SPEC_NORM_T threads:
// spec -= np.quantile(spec, q); spec[spec < 0] = 0; spec /= max(spec) + EPSILON, from the n clipped fp64 values v into
// the fp32 o.  The quantile is numpy's default ('linear'): a[lo] + (a[lo+1] - a[lo]) * gamma with lo and
// gamma from the host (numpy's own expression for the virtual index), evaluated with numpy's two-sided lerp.  a[lo] is
// found by an MSB-first radix select over the bit patterns (the values are in [0, 1], so the unsigned order of the
// patterns is the numeric order; counts are integers: deterministic), a[lo+1] from one more counting pass.
__device__ __forceinline__ void spec_normalize_window(const double* v, float* o, int n, int q_lo, double q_gamma,
                                                      float* out_max) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long sh_prefix, sh_next;
  __shared__ unsigned sh_k, sh_le;
  __shared__ double sh_max[AVA_SPEC_NORM_T / 64];
  const int t = threadIdx.x;
  unsigned long long prefix = 0;
  unsigned k = (unsigned)q_lo;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (t < 256) hist[t] = 0;
    __syncthreads();
    const unsigned long long himask = shift == 56 ? 0ull : (~0ull << (shift + 8));
    for (int i = t; i < n; i += AVA_SPEC_NORM_T) {
      const unsigned long long key = (unsigned long long)__double_as_longlong(v[i]);
      if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255ull], 1u);
    }
    __syncthreads();
    if (t == 0) {
      unsigned c = 0, b = 0;
      for (; b < 256; ++b) {
        if (c + hist[b] > k) break;
        c += hist[b];
      }
      sh_prefix = prefix | ((unsigned long long)b << shift);
      sh_k = k - c;
    }
    __syncthreads();
    prefix = sh_prefix;
    k = sh_k;
    __syncthreads();
  }
  const double alo = __longlong_as_double((long long)prefix);
  // a[lo + 1]: alo again when more than lo + 1 values are <= alo, else the smallest value above it; and the maximum
  if (t == 0) { sh_le = 0; sh_next = ~0ull; }
  __syncthreads();
  unsigned le = 0;
  unsigned long long nxt = ~0ull;
  double mx = 0.0;
  for (int i = t; i < n; i += AVA_SPEC_NORM_T) {
    const double x = v[i];
    const unsigned long long key = (unsigned long long)__double_as_longlong(x);
    if (key <= prefix) ++le; else if (key < nxt) nxt = key;
    mx = x > mx ? x : mx;
  }
  atomicAdd(&sh_le, le);
  atomicMin(&sh_next, nxt);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) { const double y = __shfl_xor(mx, s, 64); mx = y > mx ? y : mx; }
  if ((t & 63) == 0) sh_max[t >> 6] = mx;
  __syncthreads();
  for (int i = 0; i < AVA_SPEC_NORM_T / 64; ++i) mx = sh_max[i] > mx ? sh_max[i] : mx;
  const double ahi = (sh_le >= (unsigned)q_lo + 2u || q_lo + 1 >= n) ? alo : __longlong_as_double((long long)sh_next);
  // numpy's _lerp: a + (b - a) * t, replaced by b - (b - a) * (1 - t) where t >= 0.5
  const double diff = __dsub_rn(ahi, alo);
  double qv = __dadd_rn(alo, __dmul_rn(diff, q_gamma));
  if (q_gamma >= 0.5) qv = __dsub_rn(ahi, __dmul_rn(diff, __dsub_rn(1.0, q_gamma)));
  double top = __dsub_rn(mx, qv);                                    // max of the shifted, floored spectrogram
  top = top < 0.0 ? 0.0 : top;
  const double den = __dadd_rn(top, AVA_SPEC_EPS);
  float fmax = 0.f;
  for (int i = t; i < n; i += AVA_SPEC_NORM_T) {
    double x = __dsub_rn(v[i], qv);
    x = x < 0.0 ? 0.0 : x;
    const float f = (float)__ddiv_rn(x, den);
    o[i] = f;
    fmax = f > fmax ? f : fmax;
  }
  if (out_max != nullptr && fmax > 0.f) atomicMax(reinterpret_cast<int*>(out_max), __float_as_int(fmax));
}

// utils.py:77-103 for the windows of coefficient source Src.  Linear B-spline evaluation in FITPACK's order (fpbspl,
// fpbisp: the functions above), then interp2d's out-of-bounds rule, then normalisation and clip.  A workgroup owns
// AVA_SPEC_ROWS frequency rows of one window: the knot interval and the two basis values of every target TIME are
// computed once per workgroup (LDS), those of a target FREQUENCY once per row visit, so a pixel costs four loads, the
// 4-term sum and the normalising division.  Consecutive threads take consecutive target times.
template <class Src>
__global__ __launch_bounds__(256) void spec_interp_kernel(const Src a) {
  __shared__ double chx0[AVA_SPEC_TMAX], chx1[AVA_SPEC_TMAX];
  __shared__ int cl[AVA_SPEC_TMAX];                                  // knot interval of column ti, -1: outside -> fill value
  __shared__ double rhy0[AVA_SPEC_ROWS], rhy1[AVA_SPEC_ROWS];
  __shared__ int rq[AVA_SPEC_ROWS];
  const int w = blockIdx.y, f0 = blockIdx.x * AVA_SPEC_ROWS, t = threadIdx.x;
  const auto win = a.window_of(w);
  const int rows = a.F - f0 < AVA_SPEC_ROWS ? a.F - f0 : AVA_SPEC_ROWS;
  float* obase = a.out + ((size_t)w * a.F + f0) * a.T;
  if (win.nframes <= 0) {                                            // np.zeros / the NaN marker
    const float z = win.nframes == 0 ? 0.f : __builtin_nanf("");
    for (int i = t; i < rows * a.T; i += 256) obase[i] = z;
    return;
  }
  const int K = a.nperseg / 2 + 1;                 // bin frequencies: rfftfreq(n, d) = arange(n/2 + 1) * (1 / (n d)), d = 1 / fs
  for (int ti = t; ti < a.T; ti += 256)
    spec_time_basis(a.target_times[(size_t)w * a.T + ti], win.ftimes, win.nframes, a.fs, a.nstep, &cl[ti], &chx0[ti], &chx1[ti]);
  if (t < rows) spec_freq_basis(a.target_freqs[f0 + t], a.fbin, K, &rq[t], &rhy0[t], &rhy1[t]);
  __syncthreads();
  float fmax = 0.f;
  for (int i = t; i < rows * a.T; i += 256) {
    const int r = i / a.T, ti = i - r * a.T;
    const int l = cl[ti], q = rq[r];
    double v;
    if (l < 0 || q < 0) {
      v = a.fill_value;
    } else {
      const SpecCoef c = win.coef(l, q);
      v = spec_bilinear(c.t0f0, c.t0f1, c.t1f0, c.t1f1, chx0[ti], chx1[ti], rhy0[r], rhy1[r]);
    }
    v = spec_scale_clip(v, a.spec_min, a.range);                       // utils.py:101-102
    if (a.normalize) {                                                 // utils.py:104-108 follow in spec_normalize_kernel
      a.vals[((size_t)w * a.F + f0) * a.T + i] = v;
    } else {
      const float vf = (float)v;
      obase[i] = vf;
      fmax = vf > fmax ? vf : fmax;
    }
  }
  if (a.out_max != nullptr && !a.normalize) {                          // one atomic per wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float y = __shfl_xor(fmax, o, 64); fmax = y > fmax ? y : fmax; }
    if ((t & 63) == 0 && fmax > 0.f) atomicMax(reinterpret_cast<int*>(a.out_max + w), __float_as_int(fmax));
  }
}

// within_syll_normalize (utils.py:104-108), one workgroup per window: spec_normalize_window
template <class Src>
__global__ __launch_bounds__(AVA_SPEC_NORM_T) void spec_normalize_kernel(const Src a) {
  const int w = blockIdx.x;
  if (a.window_of(w).nframes <= 0) return;                           // zeros (or the NaN marker) were written already
  const int n = a.F * a.T;
  spec_normalize_window(a.vals + (size_t)w * n, a.out + (size_t)w * n, n, a.q_lo, a.q_gamma,
                        a.out_max != nullptr ? a.out_max + w : nullptr);
}

// interpolate (+ normalise) the a.n windows of source a on stream st: AVA_OK or AVA_ELAUNCH
template <class Src>
static int spec_launch_out(const Src& a, hipStream_t st) {
  hipLaunchKernelGGL(spec_interp_kernel<Src>, dim3(ceil_div(a.F, AVA_SPEC_ROWS), a.n), dim3(256), 0, st, a);
  AVA_CHECK_LAUNCH();
  if (a.normalize) {
    hipLaunchKernelGGL(spec_normalize_kernel<Src>, dim3(a.n), dim3(AVA_SPEC_NORM_T), 0, st, a);
    AVA_CHECK_LAUNCH();
  }
  return AVA_OK;
}
#endif
