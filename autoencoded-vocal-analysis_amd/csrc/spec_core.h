// The arithmetic of get_spec (ava/preprocessing/utils.py:77-108) after the transform, shared by the shotgun
// spectrograms (spec.hip) and the warped windows out of the motif cache (warp_spec.hip,
// row f9): the linear B-spline basis of a target time / frequency in FITPACK's order, the four-term sum, interp2d's
// fill rule, the normalisation and clip, and within_syll_normalize.  Both units call these functions, so that a window
// cut from the cache and the same window transformed on its own are the same bits.  Also the argument block of
// spec.hip's kernels and the host launcher of its first two stages, which warp_spec.hip runs once per file.
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

struct SpecArgs {
  const void* audio;
  const long long* file_off;
  const long long* file_len;
  const int* file_idx;
  const double* t1;
  const double* t2;
  const double* target_times;    // [n][T]
  const double* target_freqs;    // [F]
  const double* window;          // [nperseg]
  SpecMeta* meta;
  double* twiddle;               // [nperseg/2][2]: exp(-2 pi i k / nperseg), written by spec_prep_kernel's workgroup 0
  double* ftimes;                // [n][maxframes]: frame times of each window, written by spec_prep_kernel
  int* krange;                   // [2]: first / last frequency bin the target frequencies can touch (workgroup 0)
  double* logmag;                // [n][maxframes][nperseg/2 + 1]
  float* out;                    // [n][F][T]
  float* out_max;                // [n] or null
  double* vals;                  // [n][F*T]: clipped fp64 spectrograms handed to spec_normalize_kernel (normalize only)
  double q_gamma;                // within_syll_normalize: np.quantile's interpolation weight ...
  int q_lo, normalize;           // ... between the order statistics q_lo and q_lo + 1 (0-based)
  double fs, scale, spec_min, range, fill_value, fbin;    // fbin: rfftfreq's 1 / (nperseg * (1 / fs))
  int n, maxframes, nperseg, nstep, F, T, dtype, remove_dc;
};

// spec.hip: STFT frames of max_samples samples; the shapes its kernels take; the bytes of the scratch regions
// spec_launch_frames fills (krange, meta, twiddle, ftimes, logmag, in the order ava_get_spec_batch lays them out); and
// spec_prep_kernel + the transform of every window's needed frames on stream st (AVA_OK or AVA_ELAUNCH).
int spec_frames_for(int max_samples, int nstep);
bool spec_shape_ok(int nperseg, int noverlap);
void spec_carve(SpecArgs& a, void* ws, int n, int max_samples, int nperseg, int noverlap);
int spec_launch_frames(const SpecArgs& a, hipStream_t st);

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
#endif
