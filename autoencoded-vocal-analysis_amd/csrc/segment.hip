// Amplitude segmentation on the device: the arithmetic of
// ava/segmenting/amplitude_segmentation.py:get_onsets_offsets for every recording of a DeviceAudio at once.
//
//   scipy.signal.stft of the whole file (hann, zero boundary, zero padded to whole hops, 'spectrum' scaling, no detrend),
//   bins [searchsorted(f, min_freq), searchsorted(f, max_freq)), clip((log(|X| + 1e-9) - min) / (max - min), 0, 1),
//   per frame  sum v  or  sum v e / (sum e + 1e-9), e = exp(v / temperature)
//                                          segmenting/utils.py:22-61, 400-404, amplitude_segmentation.py:63-66
//                                                                     band_stft_kernel    (workgroups stride over frames)
//   gaussian_filter(amps, smoothing_timescale / dt), mode 'reflect' inside each file, cast to the reference's dtype
//                                          amplitude_segmentation.py:67                  amp_smooth_kernel   (1 thread / frame)
//   local maxima above th_3                amplitude_segmentation.py:70-73               amp_maxima_kernel   (1 thread / frame)
//   nearest stop frame left and right of every maximum
//                                          amplitude_segmentation.py:79-99               amp_stops_kernel    (1 wave / maximum)
//
// The host receives O(#maxima) integers and runs the greedy chain and the duration filter (ava_amd/segment.py).
// band_stft_kernel in sum mode, with the spectrogram, is also the band stage of the template segmentation (row f6):
// ava_tpl_spec below; its correlation is template_seg.hip.
// The spectral arithmetic is fp64 (the transform of stft.h, shared with spec.hip); the trace is stored in the dtype the
// reference holds it in (float32 for int16 / float32 audio, float64 otherwise), and the decision kernels compare the
// values of THAT trace, promoted exactly to fp64, against thresholds the host has already rounded the way numpy would
// (a Python float compared with a float32 array is a float32).
#include "stft.h"

#define AVA_AMP_EPS 1e-9
#define AVA_AMP_T 256

struct BandArgs {
  const void* audio;
  const long long* file_off;     // [files] first sample of each file in `audio`
  const long long* file_len;     // [files] samples of each file
  const long long* frame_off;    // [files + 1] first global frame of each file; frame_off[files] = frames
  const double* window;          // [nperseg]
  double* raw;                   // [frames] per-frame band value: the sum, or the softmax-weighted value
  double* spec;                  // [k1 - k0][frames] band spectrogram or null
  double scale, spec_min, range, temperature;
  long long frames;
  int files, nperseg, nstep, k0, k1, dtype;
};

// One workgroup per frame, striding over all frames of all files: the shared transform of stft.h, then the band
// reduction in a fixed order (thread partial sums, then the waves' shuffles, then the four waves in order):
// deterministic.  SOFTMAX is a template parameter, not a flag: the sum-mode instances are spared the exp, the second
// reduction and their registers.
template <int LOGN, bool SOFTMAX>
__global__ __launch_bounds__(AVA_AMP_T) void band_stft_kernel(const BandArgs a) {
  constexpr int N = 1 << LOGN, H = N / 2;
  __shared__ double re[stft_lds(H)], im[stft_lds(H)];
  __shared__ double twr[stft_lds(H)], twi[stft_lds(H)];       // exp(-2 pi i k / N), k < N/2
  __shared__ double red[SOFTMAX ? 2 : 1][AVA_AMP_T / 64];
  const int t = threadIdx.x;
  for (int k = t; k < H; k += AVA_AMP_T) {
    double sn, cs;
    sincospi(-2.0 * (double)k / (double)N, &sn, &cs);
    twr[stft_pd(k)] = cs;
    twi[stft_pd(k)] = sn;
  }
  auto frame = [&](long long g) {                             // global frame g: a frame of its file
    const int f = stft_file_of(a.frame_off, a.files, g);
    const long long c = (g - a.frame_off[f]) * a.nstep, len = a.file_len[f], base = a.file_off[f];
    return [&a, c, len, base](long long p, bool live) {
      const long long idx = c + p;
      const bool in = live && idx >= 0 && idx < len;
      const double x = audio_at(a.audio, a.dtype, base + (in ? idx : 0));
      return in ? x : 0.0;
    };
  };
  auto band = [&](long long g) {                              // the kept bins k0 <= k < k1 (<= H)
    double s0 = 0.0, s1 = 0.0;
    for (int k = a.k0 + t; k < a.k1; k += AVA_AMP_T) {
      const double lg = stft_logmag(stft_bin<LOGN>(k, re, im, twr, twi), a.scale, AVA_AMP_EPS);
      double v = __ddiv_rn(__dsub_rn(lg, a.spec_min), a.range);
      v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
      if (a.spec != nullptr) a.spec[(size_t)(k - a.k0) * a.frames + g] = v;
      if constexpr (SOFTMAX) {
        const double e = exp(__ddiv_rn(v, a.temperature));
        s0 = fma(v, e, s0);
        s1 += e;
      } else {
        s0 += v;
      }
    }
    s0 = wave_sum_d(s0);
    if constexpr (SOFTMAX) s1 = wave_sum_d(s1);
    if ((t & 63) == 0) { red[0][t >> 6] = s0; if constexpr (SOFTMAX) red[1][t >> 6] = s1; }
    __syncthreads();
    if (t == 0) {
      double v0 = 0.0, v1 = 0.0;
#pragma unroll
      for (int w = 0; w < AVA_AMP_T / 64; ++w) { v0 += red[0][w]; if constexpr (SOFTMAX) v1 += red[1][w]; }
      a.raw[g] = SOFTMAX ? __ddiv_rn(v0, __dadd_rn(v1, AVA_AMP_EPS)) : v0;
    }
  };
  stft_frames<LOGN, AVA_AMP_T>((long long)blockIdx.x, a.frames, (long long)gridDim.x, a.window, re, im, twr, twi, frame,
                               band);
}

// scipy.ndimage.gaussian_filter on each file's trace: correlation with the 2 radius + 1 host-computed weights, mode
// 'reflect' (d c b a | a b c d | d c b a, repeated: period 2 T), fp64, then one rounding to the trace's dtype.
template <typename V>
__global__ __launch_bounds__(AVA_AMP_T) void amp_smooth_kernel(const double* raw, const long long* frame_off, int files,
                                                               long long frames, const double* w, int radius, V* out) {
  const long long g = (long long)blockIdx.x * AVA_AMP_T + threadIdx.x;
  if (g >= frames) return;
  const int f = stft_file_of(frame_off, files, g);
  const long long b = frame_off[f], T = frame_off[f + 1] - b, i = g - b, P = 2 * T;
  double s = 0.0;
  for (int k = -radius; k <= radius; ++k) {
    long long m = (i + k) % P;
    if (m < 0) m += P;
    if (m >= T) m = P - 1 - m;
    s = fma(w[k + radius], raw[b + m], s);
  }
  out[g] = (V)s;
}

// amplitude_segmentation.py:83-98's stop test at frame j >= 1 of a file of T frames: a[j] < th_1, or a[j] < th_2 and
// a[j] == min(a[j-1:j+2]) (the slice clipped at the file's end; a NaN in it makes the == false)
template <typename V>
__device__ __forceinline__ bool amp_is_stop(const V* a, long long b, long long T, long long j, double th1, double th2) {
  const double x = (double)a[b + j];
  if (x < th1) return true;
  if (!(x < th2)) return false;
  if (!((double)a[b + j - 1] >= x)) return false;
  if (j + 1 < T && !((double)a[b + j + 1] >= x)) return false;
  return true;
}

// amplitude_segmentation.py:70-73: 1 <= i <= T-2, a[i] > th_3, a[i] == max(a[i-1:i+2]).  The maxima of a wave are
// appended with one atomic per wave (their order in the list is not deterministic; the host sorts them).
template <typename V>
__global__ __launch_bounds__(AVA_AMP_T) void amp_maxima_kernel(const V* a, const long long* frame_off, int files,
                                                               long long frames, double th3,
                                                               unsigned long long* count, long long* maxima) {
  const long long g = (long long)blockIdx.x * AVA_AMP_T + threadIdx.x;
  bool is_max = false;
  if (g < frames) {
    const int f = stft_file_of(frame_off, files, g);
    const long long b = frame_off[f], T = frame_off[f + 1] - b, i = g - b;
    if (i >= 1 && i <= T - 2) {
      const double x = (double)a[g];
      is_max = x > th3 && (double)a[g - 1] <= x && (double)a[g + 1] <= x;
    }
  }
  const unsigned long long m = __ballot(is_max);
  if (m == 0) return;
  const int lane = threadIdx.x & 63;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(count, (unsigned long long)__popcll(m));
  base = __shfl(base, 0, 64);
  if (is_max) maxima[base + __popcll(m & ((1ull << lane) - 1ull))] = g;
}

// One wave per maximum: 64 candidate frames per step, the nearest stop is the lowest set lane of the ballot.
// left[e] / right[e]: frame index inside the file, or -1 when the search ends without a stop.
template <typename V>
__global__ __launch_bounds__(AVA_AMP_T) void amp_stops_kernel(const V* a, const long long* frame_off, int files,
                                                              double th1, double th2, const unsigned long long* count,
                                                              const long long* maxima, long long* left, long long* right) {
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * (AVA_AMP_T / 64);
  const long long n = (long long)*count;
  for (long long e = (long long)blockIdx.x * (AVA_AMP_T / 64) + (threadIdx.x >> 6); e < n; e += waves) {
    const long long g = maxima[e];
    const int f = stft_file_of(frame_off, files, g);
    const long long b = frame_off[f], T = frame_off[f + 1] - b, m = g - b;
    long long l = -1, r = -1;
    for (long long c = m - 1; c >= 1; c -= 64) {                // j = c, c-1, ..., down to 1
      const long long j = c - lane;
      const unsigned long long bal = __ballot(j >= 1 && amp_is_stop(a, b, T, j, th1, th2));
      if (bal != 0) { l = c - __builtin_ctzll(bal); break; }
    }
    for (long long c = m + 1; c <= T - 1; c += 64) {            // j = c, c+1, ..., up to T-1
      const long long j = c + lane;
      const unsigned long long bal = __ballot(j <= T - 1 && amp_is_stop(a, b, T, j, th1, th2));
      if (bal != 0) { r = c + __builtin_ctzll(bal); break; }
    }
    if (lane == 0) { left[e] = l; right[e] = r; }
  }
}

// The band stage of ava_amp_trace and ava_tpl_spec: AVA_EINVAL before any launch for a null pointer, no files or
// frames, an unsupported nperseg, noverlap >= nperseg, an empty band, an unknown audio dtype or a divisor `range` of 0
// (spec_min == spec_max for the segmenters, whose divisor is spec_max - spec_min); otherwise band_stft_kernel writes raw
// (and spec, if not null) on stream st.
static int band_stft(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                     const int64_t* frame_off, int files, int64_t frames, int nperseg, int noverlap,
                     const double* window, double scale, int k0, int k1, double spec_min, double range, bool softmax,
                     double temperature, double* raw, double* spec, hipStream_t st) {
  if (audio == nullptr || file_off == nullptr || file_len == nullptr || frame_off == nullptr || window == nullptr ||
      raw == nullptr)
    return AVA_EINVAL;
  if (files <= 0 || frames <= 0) return AVA_EINVAL;
  if (nperseg < 64 || nperseg > 2048 || (nperseg & (nperseg - 1)) != 0) return AVA_EINVAL;
  if (noverlap < 0 || noverlap >= nperseg) return AVA_EINVAL;
  if (k0 < 0 || k1 <= k0 || k1 > nperseg / 2 + 1) return AVA_EINVAL;             // empty band
  if (audio_dtype < AVA_AUDIO_I16 || audio_dtype > AVA_AUDIO_F64) return AVA_EINVAL;
  if (!(range != 0.0) || range != range) return AVA_EINVAL;
  BandArgs a;
  a.audio = audio;
  a.file_off = reinterpret_cast<const long long*>(file_off);
  a.file_len = reinterpret_cast<const long long*>(file_len);
  a.frame_off = reinterpret_cast<const long long*>(frame_off);
  a.window = window;
  a.raw = raw;
  a.spec = spec;
  a.scale = scale; a.spec_min = spec_min; a.range = range; a.temperature = temperature;
  a.frames = frames; a.files = files; a.nperseg = nperseg; a.nstep = nperseg - noverlap;
  a.k0 = k0; a.k1 = k1; a.dtype = audio_dtype;
  const int grid = frames < 4096 ? (int)frames : 4096;      // workgroups stride over the frames
  stft_dispatch(nperseg, [&](auto logn) {
    constexpr int LOGN = decltype(logn)::value;
    hipLaunchKernelGGL((softmax ? band_stft_kernel<LOGN, true> : band_stft_kernel<LOGN, false>), dim3(grid),
                       dim3(AVA_AMP_T), 0, st, a);
  });
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" size_t ava_amp_workspace_bytes(int64_t frames) {
  if (frames <= 0) return 0;
  return 256 + (size_t)frames * sizeof(double);
}

extern "C" int ava_amp_trace(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                             const int64_t* frame_off, int files, int64_t frames, int nperseg, int noverlap,
                             const double* window, double scale, int k0, int k1, double spec_min, double spec_max,
                             int softmax, double temperature, const double* gauss_w, int radius, int trace_f64,
                             void* trace, double* spec, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (gauss_w == nullptr || trace == nullptr || radius < 0) return AVA_EINVAL;
  if (softmax && !(temperature != 0.0)) return AVA_EINVAL;
  if (ws == nullptr || ws_bytes < ava_amp_workspace_bytes(frames)) return AVA_EINVAL;
  double* raw = reinterpret_cast<double*>(ava_align256(ws));
  hipStream_t st = to_stream(s);
  const int rc = band_stft(audio, audio_dtype, file_off, file_len, frame_off, files, frames, nperseg, noverlap, window,
                           scale, k0, k1, spec_min, spec_max - spec_min, softmax != 0, temperature, raw, spec, st);
  if (rc != AVA_OK) return rc;
  const long long* fo = reinterpret_cast<const long long*>(frame_off);
  const dim3 sgrid((unsigned)ceil_div64(frames, AVA_AMP_T));
  if (trace_f64)
    hipLaunchKernelGGL(amp_smooth_kernel<double>, sgrid, dim3(AVA_AMP_T), 0, st, raw, fo, files, frames, gauss_w,
                       radius, reinterpret_cast<double*>(trace));
  else
    hipLaunchKernelGGL(amp_smooth_kernel<float>, sgrid, dim3(AVA_AMP_T), 0, st, raw, fo, files, frames, gauss_w,
                       radius, reinterpret_cast<float*>(trace));
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// ava_amp_trace's band stage in sum mode, without smoothing: the spectrogram and the raw band sums
extern "C" int ava_tpl_spec(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                            const int64_t* frame_off, int files, int64_t frames, int nperseg, int noverlap,
                            const double* window, double scale, int k0, int k1, double spec_min, double spec_max,
                            double* spec, double* frame_sum, ava_stream_t s) {
  if (spec == nullptr) return AVA_EINVAL;
  return band_stft(audio, audio_dtype, file_off, file_len, frame_off, files, frames, nperseg, noverlap, window, scale,
                   k0, k1, spec_min, spec_max - spec_min, false, 1.0, frame_sum, spec, to_stream(s));
}

// The inputs of the time-warp fit (ava/models/utils.py:337-418, row f9): the same band stage with the divisor handed in,
// because _get_spec divides by spec_max_val - spec_min_val + 1e-9 where the segmenters divide by the plain difference.
// spec [k1 - k0][frames] and the per-frame band sums; the truncation to common shapes and the normalisation of each
// trace are the host's.
extern "C" int ava_warp_band_spec(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                                  const int64_t* frame_off, int files, int64_t frames, int nperseg, int noverlap,
                                  const double* window, double scale, int k0, int k1, double spec_min, double divisor,
                                  double* spec, double* frame_sum, ava_stream_t s) {
  if (spec == nullptr) return AVA_EINVAL;
  return band_stft(audio, audio_dtype, file_off, file_len, frame_off, files, frames, nperseg, noverlap, window, scale,
                   k0, k1, spec_min, divisor, false, 1.0, frame_sum, spec, to_stream(s));
}

extern "C" int ava_amp_decide(const void* trace, int trace_f64, const int64_t* frame_off, int files, int64_t frames,
                              double th1, double th2, double th3, uint64_t* count, int64_t* maxima, int64_t* left,
                              int64_t* right, int64_t capacity, ava_stream_t s) {
  if (trace == nullptr || frame_off == nullptr || count == nullptr || maxima == nullptr || left == nullptr ||
      right == nullptr)
    return AVA_EINVAL;
  if (files <= 0 || frames <= 0 || capacity < frames) return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  if (hipMemsetAsync(count, 0, sizeof(uint64_t), st) != hipSuccess) return AVA_ELAUNCH;
  const long long* fo = reinterpret_cast<const long long*>(frame_off);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count);
  long long* mx = reinterpret_cast<long long*>(maxima);
  long long* lf = reinterpret_cast<long long*>(left);
  long long* rt = reinterpret_cast<long long*>(right);
  const dim3 mgrid((unsigned)ceil_div64(frames, AVA_AMP_T));
  const long long want = ceil_div64(frames, AVA_AMP_T / 64);            // one wave per maximum at most
  const dim3 wgrid((unsigned)(want < 2048 ? want : 2048));
  if (trace_f64) {
    const double* a = reinterpret_cast<const double*>(trace);
    hipLaunchKernelGGL(amp_maxima_kernel<double>, mgrid, dim3(AVA_AMP_T), 0, st, a, fo, files, (long long)frames, th3, cnt, mx);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL(amp_stops_kernel<double>, wgrid, dim3(AVA_AMP_T), 0, st, a, fo, files, th1, th2, cnt, mx, lf, rt);
  } else {
    const float* a = reinterpret_cast<const float*>(trace);
    hipLaunchKernelGGL(amp_maxima_kernel<float>, mgrid, dim3(AVA_AMP_T), 0, st, a, fo, files, (long long)frames, th3, cnt, mx);
    AVA_CHECK_LAUNCH();
    hipLaunchKernelGGL(amp_stops_kernel<float>, wgrid, dim3(AVA_AMP_T), 0, st, a, fo, files, th1, th2, cnt, mx, lf, rt);
  }
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
