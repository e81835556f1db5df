// The fp64 STFT frame shared by the shotgun spectrograms (spec.hip), the amplitude
// segmentation (segment.hip, row f5) and the template segmentation (template_seg.hip, row f6): scipy.signal.stft's
// Hann frames with zero boundary, the N-point transform of a real frame as an N/2-point complex FFT of the
// even/odd-interleaved samples (radix-2 decimation in time in LDS) + the split step, and the log-magnitude of the
// one-sided spectrum.  Each unit keeps its own twiddle source and its own use of the bins.
//
// The units are built with -ffp-contract=on, which fuses a product into an add only inside one source expression: the
// bits depend on how the arithmetic below is cut into expressions, so it stays cut exactly as it is.
#pragma once
#include <type_traits>
#include "common.h"

// audio_dtype codes of the C ABI (ava_hip.h: ava_get_spec_batch, ava_amp_trace)
enum { AVA_AUDIO_I16 = 0, AVA_AUDIO_I32 = 1, AVA_AUDIO_F32 = 2, AVA_AUDIO_F64 = 3 };

__device__ __forceinline__ double audio_at(const void* base, int dtype, long long i) {
  switch (dtype) {
    case AVA_AUDIO_I16: return (double)reinterpret_cast<const short*>(base)[i];
    case AVA_AUDIO_I32: return (double)reinterpret_cast<const int*>(base)[i];
    case AVA_AUDIO_F32: return (double)reinterpret_cast<const float*>(base)[i];
    default: return reinterpret_cast<const double*>(base)[i];
  }
}

// file of global frame g: the f with frame_off[f] <= g < frame_off[f + 1] (files without frames are never returned).
// Any [files + 1] table of ascending offsets works the same way (template_seg.hip looks workgroups up in its tile table).
__device__ __forceinline__ int stft_file_of(const long long* frame_off, int files, long long g) {
  int lo = 0, hi = files;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (frame_off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// Every LDS array of the transform is indexed through stft_pd(i) = i + i / 8: one pad double per eight spreads the
// power-of-two strides of the bit-reversed store, the butterflies and the twiddle look-ups over the banks (73 % of the
// LDS cycles of the unpadded kernel were bank conflicts).  stft_lds(H): doubles of one such array for indices < H.
__host__ __device__ constexpr int stft_pd(int i) { return i + (i >> 3); }
__host__ __device__ constexpr int stft_lds(int h) { return h + h / 8 + 1; }

// In-place N/2-point FFT of re / im, which hold the bit-reversed complex frame (the caller's barrier has made them
// visible), with twr / twi = exp(-2 pi i k / N), k < N/2.  Ends with a barrier.  NT threads.
template <int LOGN, int NT>
__device__ __forceinline__ void stft_fft(double* re, double* im, const double* twr, const double* twi) {
  constexpr int N = 1 << LOGN, H = N / 2, LOGH = LOGN - 1;
  const int t = threadIdx.x;
  // Two radix-2 stages (half = h, then 2 h) per pass over LDS: the four points i0 + {0, h, 2h, 3h} of a group are
  // combined in registers (same operations, same order as two separate stages; half the LDS traffic, which bounds
  // this kernel).  An odd stage count ends with one plain radix-2 pass.
  int st = 0;
#pragma unroll 1
  for (; st + 1 < LOGH; st += 2) {
    const int h = 1 << st;
    for (int b = t; b < H / 4; b += NT) {
      const int pos = b & (h - 1);
      const int i0 = ((b >> st) << (st + 2)) + pos, i1 = i0 + h, i2 = i1 + h, i3 = i2 + h;
      const int k1 = pos << (LOGN - 1 - st), k2 = pos << (LOGN - 2 - st);
      const double w1r = twr[stft_pd(k1)], w1i = twi[stft_pd(k1)], w2r = twr[stft_pd(k2)], w2i = twi[stft_pd(k2)];
      const double x1r = re[stft_pd(i1)], x1i = im[stft_pd(i1)], x3r = re[stft_pd(i3)], x3i = im[stft_pd(i3)];
      const double p1r = w1r * x1r - w1i * x1i, p1i = w1r * x1i + w1i * x1r;
      const double p3r = w1r * x3r - w1i * x3i, p3i = w1r * x3i + w1i * x3r;
      const double u0r = re[stft_pd(i0)], u0i = im[stft_pd(i0)], u2r = re[stft_pd(i2)], u2i = im[stft_pd(i2)];
      const double b0r = u0r + p1r, b0i = u0i + p1i, b1r = u0r - p1r, b1i = u0i - p1i;     // stage st
      const double b2r = u2r + p3r, b2i = u2i + p3i, b3r = u2r - p3r, b3i = u2i - p3i;
      const double q2r = w2r * b2r - w2i * b2i, q2i = w2r * b2i + w2i * b2r;               // stage st + 1: W^pos
      // twiddle of the pair (i1, i3) is W_{4h}^{pos + h} = exp(-2 pi i (pos + h) / (4 h)): entry k2 + N/4 of the table
      const double w3r = twr[stft_pd(k2 + H / 2)], w3i = twi[stft_pd(k2 + H / 2)];
      const double q3r = w3r * b3r - w3i * b3i, q3i = w3r * b3i + w3i * b3r;
      re[stft_pd(i0)] = b0r + q2r; im[stft_pd(i0)] = b0i + q2i;
      re[stft_pd(i2)] = b0r - q2r; im[stft_pd(i2)] = b0i - q2i;
      re[stft_pd(i1)] = b1r + q3r; im[stft_pd(i1)] = b1i + q3i;
      re[stft_pd(i3)] = b1r - q3r; im[stft_pd(i3)] = b1i - q3i;
    }
    __syncthreads();
  }
  if (st < LOGH) {
    const int half = 1 << st;
    for (int b = t; b < H / 2; b += NT) {
      const int pos = b & (half - 1);
      const int i0 = ((b >> st) << (st + 1)) + pos, i1 = i0 + half;
      const int tk = pos << (LOGN - 1 - st);               // exp(-2 pi i pos / (2 half)) in units of the N table
      const double wr = twr[stft_pd(tk)], wi = twi[stft_pd(tk)];
      const double xr = re[stft_pd(i1)], xi = im[stft_pd(i1)];
      const double pr = wr * xr - wi * xi, pi = wr * xi + wi * xr;
      const double ur = re[stft_pd(i0)], ui = im[stft_pd(i0)];
      re[stft_pd(i0)] = ur + pr; im[stft_pd(i0)] = ui + pi;
      re[stft_pd(i1)] = ur - pr; im[stft_pd(i1)] = ui - pi;
    }
    __syncthreads();
  }
}

struct StftBin { double re, im; };

// Bin k (0 <= k <= N/2) of the real frame from the transformed Z in re / im:
//   X_k = E_k + W_N^k O_k,  E_k = (Z_k + conj Z_{H-k}) / 2,  O_k = -i (Z_k - conj Z_{H-k}) / 2
template <int LOGN>
__device__ __forceinline__ StftBin stft_bin(int k, const double* re, const double* im, const double* twr,
                                            const double* twi) {
  constexpr int H = 1 << (LOGN - 1);
  const int ka = k & (H - 1), kb = (H - k) & (H - 1);
  const double zr = re[stft_pd(ka)], zi = im[stft_pd(ka)], cr = re[stft_pd(kb)], ci = -im[stft_pd(kb)];
  const double er = 0.5 * (zr + cr), ei = 0.5 * (zi + ci);
  const double dr = 0.5 * (zr - cr), di = 0.5 * (zi - ci);
  const double orr = di, oi = -dr;                                  // -i (dr + i di)
  const double wr = k == H ? -1.0 : twr[stft_pd(k)], wi = k == H ? 0.0 : twi[stft_pd(k)];
  return {er + (wr * orr - wi * oi), ei + (wr * oi + wi * orr)};
}

// log(|X| scale + eps).  |X|: no overflow / underflow guard needed at audio magnitudes (numpy's abs is hypot: same
// value to an ulp)
__device__ __forceinline__ double stft_logmag(StftBin x, double scale, double eps) {
  return log(__dadd_rn(__dmul_rn(sqrt(x.re * x.re + x.im * x.im), scale), eps));
}

// The frames first, first + stride, ... < end, one workgroup of NT threads; twr / twi hold the twiddles (written by
// the caller; the first barrier below publishes them).  frame(j) returns the sample reader of frame j:
// sample(p, live) is the input at offset p (-N/2 <= p < N/2) from the frame's centre, 0 outside the signal or when
// !live (read with an unconditional load at a clamped address).  Thread t owns the pairs (2 i, 2 i + 1), i = t + NT u,
// of every frame and fetches them one frame ahead.  Per frame: Hann window, bit-reversed store, stft_fft, then
// consume(j), which reads the bins it wants through stft_bin.
template <int LOGN, int NT, typename J, typename Frame, typename Consume>
__device__ __forceinline__ void stft_frames(J first, J end, J stride, const double* window, double* re, double* im,
                                            const double* twr, const double* twi, Frame frame, Consume consume) {
  constexpr int N = 1 << LOGN, H = N / 2, LOGH = LOGN - 1, U = H / NT > 0 ? H / NT : 1;
  const int t = threadIdx.x;
  double raw[U][2];
  auto fetch = [&](J j) {
    const auto sample = frame(j);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = t + NT * u;
#pragma unroll
      for (int e = 0; e < 2; ++e) raw[u][e] = sample(2ll * i + e - N / 2, i < H);   // 64-bit: int costs 8 VGPRs at N = 2048
    }
  };
  if (first < end) fetch(first);
  for (J j = first; j < end; j += stride) {
    __syncthreads();                                       // twiddles ready / previous frame's reads retired
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = t + NT * u;
      if (i < H) {
        const int r = (int)(__brev((unsigned)i) >> (32 - LOGH));
        re[stft_pd(r)] = __dmul_rn(raw[u][0], window[2 * i]);
        im[stft_pd(r)] = __dmul_rn(raw[u][1], window[2 * i + 1]);
      }
    }
    if (j + stride < end) fetch(j + stride);               // in flight under this frame's butterflies
    __syncthreads();
    stft_fft<LOGN, NT>(re, im, twr, twi);
    consume(j);
  }
}

// launch(std::integral_constant<int, LOGN>()) for nperseg = 2^LOGN, a power of two in 64..2048 (checked by the caller)
template <typename Launch>
static inline void stft_dispatch(int nperseg, Launch launch) {
  switch (nperseg) {
    case 64: launch(std::integral_constant<int, 6>()); break;
    case 128: launch(std::integral_constant<int, 7>()); break;
    case 256: launch(std::integral_constant<int, 8>()); break;
    case 512: launch(std::integral_constant<int, 9>()); break;
    case 1024: launch(std::integral_constant<int, 10>()); break;
    default: launch(std::integral_constant<int, 11>()); break;
  }
}
