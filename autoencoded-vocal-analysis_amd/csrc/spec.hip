// Shotgun spectrograms on the device: get_spec of the reference
// (ava/preprocessing/utils.py:18-110) for a whole BATCH of windows whose audio already lives in HBM, as called by
// FixedWindowDataset.__getitem__ (ava/models/window_vae_dataset.py:189-256):
//
//   slice audio[max(0,s1):min(len,s2)], subtract its mean   utils.py:62-73      spec_prep_kernel   (1 workgroup / window)
//   scipy.signal.stft (hann, zero boundary, zero padded to whole hops, 'spectrum' scaling), log(|.| + 1e-12)
//                                                           utils.py:74-76      spec_stft_kernel   (1 workgroup / frame)
//   interp2d (bilinear on the (t, f) grid, fill outside), (x - min) / (max - min), clip to [0, 1]
//                                                           utils.py:77-103     spec_interp_kernel of spec_core.h (1 thread / pixel)
//
// Everything is fp64, as in the reference (int16 audio - float64 mean -> complex128 STFT): the log turns relative
// errors of small bins into absolute ones, and bins 100 dB under the frame's peak are above the clip floor.  The output
// is the fp32 [n, F, T] batch the VAE consumes (the reference converts with numpy_to_tensor, models/utils.py:444-446).
// Cost is irrelevant next to the train step: a batch of 256 windows is 7 k (finch: 512-point) to 38 k (mouse: 1024-point)
// FFTs, 0.3 to 2 GFLOP.  The frame times and bin frequencies are computed with the reference's own operation order
// (scipy's arange / fs - (nperseg/2) / fs + max(0, t1); rfftfreq's k * (1 / (n d))) and without contraction, so that
// the interval a target point falls into is decided by the same numbers.
#include "spec_core.h"

// frame time j of a window: scipy's  arange(nperseg/2, ..., hop) / fs - (nperseg/2) / fs, then utils.py:75's + max(0, t1)
__device__ __forceinline__ double frame_time(int j, const SpecArgs& a, double t_shift) {
  const double half = 0.5 * (double)a.nperseg;
  const double c = __ddiv_rn(half + (double)j * (double)a.nstep, a.fs);
  return __dadd_rn(__dsub_rn(c, __ddiv_rn(half, a.fs)), t_shift);
}

#define AVA_SPEC_PREP_T 1024
// utils.py:58-73: sample range of the window, the "too short" rule, the mean of the slice.  Fixed-order sum (thread
// strides, then a tree): deterministic; exact for integer audio (|sum| < 2^53), where it equals numpy's pairwise sum.
// int16 recordings (the usual wav) are read 8 samples per load.  Also: the range of frames the target times of this
// window can fall between, and (workgroup 0) the twiddle table of the transform.
__global__ __launch_bounds__(AVA_SPEC_PREP_T) void spec_prep_kernel(const SpecArgs a) {
  __shared__ double red[AVA_SPEC_PREP_T];
  __shared__ double tlo[64], thi[64];
  const int w = blockIdx.x, t = threadIdx.x;
  if (w == 0) {
    // power of two: exp(-2 pi i k / N) for k < N / 2 (k / N is exact); any other length: the whole circle, k < N, for the direct
    // transform (spec_dft_kernel), whose index (k n) mod N is exact -- only the quotient k / N is rounded, 1e-16 of the angle
    const int ntw = (a.nperseg & (a.nperseg - 1)) == 0 ? a.nperseg / 2 : a.nperseg;
    for (int k = t; k < ntw; k += AVA_SPEC_PREP_T) {
      double sn, cs;
      sincospi(-2.0 * (double)k / (double)a.nperseg, &sn, &cs);
      a.twiddle[2 * k] = cs;
      a.twiddle[2 * k + 1] = sn;
    }
  }
  if (w == 0 && t < 64) {                                       // bins the target frequencies lie between (+- 2 of slack)
    double mnf = 1e300, mxf = -1e300;
    for (int i = t; i < a.F; i += 64) {
      const double y = a.target_freqs[i];
      if (y < mnf) mnf = y;
      if (y > mxf) mxf = y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double m2 = __shfl_xor(mnf, o, 64), x2 = __shfl_xor(mxf, o, 64);
      mnf = m2 < mnf ? m2 : mnf;
      mxf = x2 > mxf ? x2 : mxf;
    }
    if (t == 0) {
      spec_bin_range(mnf, mxf, a.fbin, a.nperseg, &a.krange[0], &a.krange[1]);
    }
  }
  const long long len = a.file_len[a.file_idx[w]];
  const long long base = a.file_off[a.file_idx[w]];
  const double t1 = a.t1[w], t2 = a.t2[w];
  const long long s1 = (long long)rint(__dmul_rn(t1, a.fs));      // int(round(t1*fs)): round half to even
  const long long s2 = (long long)rint(__dmul_rn(t2, a.fs));
  const long long lo = s1 > 0 ? s1 : 0, hi = s2 < len ? s2 : len;
  const long long cnt = hi - lo;
  const bool valid = !(cnt < a.nperseg || s2 <= 0 || s1 >= len);
  double s = 0.0;
  if (valid && a.remove_dc) {
    const long long e0 = base + lo, e1 = e0 + cnt;
    if (a.dtype == AVA_AUDIO_I16) {
      const short* p = reinterpret_cast<const short*>(a.audio);
      long long a0 = (e0 + 7) & ~7ll, a1 = e1 & ~7ll;                 // 16-byte aligned body [a0, a1)
      if (a0 > a1) { a0 = e1; a1 = e1; }
      for (long long i = e0 + t; i < a0; i += AVA_SPEC_PREP_T) s += (double)p[i];
      const int4* p8 = reinterpret_cast<const int4*>(p + a0);
      const long long nv = (a1 - a0) >> 3;
      for (long long v = t; v < nv; v += AVA_SPEC_PREP_T) {
        const int4 q = p8[v];
        const int ws[4] = {q.x, q.y, q.z, q.w};
        int acc = 0;                                                   // 8 int16: exact in int32
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += (int)(short)(ws[u] & 0xffff) + (ws[u] >> 16);
        s += (double)acc;
      }
      for (long long i = a1 + t; i < e1; i += AVA_SPEC_PREP_T) s += (double)p[i];
    } else {
      for (long long i = e0 + t; i < e1; i += AVA_SPEC_PREP_T) s += audio_at(a.audio, a.dtype, i);
    }
  }
  red[t] = s;
  // smallest / largest target time of the window (NaNs ignored)
  double mn = 1e300, mx = -1e300;
  for (int i = t; i < a.T; i += AVA_SPEC_PREP_T) {
    const double x = a.target_times[(size_t)w * a.T + i];
    if (x < mn) mn = x;
    if (x > mx) mx = x;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double m2 = __shfl_xor(mn, o, 64), x2 = __shfl_xor(mx, o, 64);
    mn = m2 < mn ? m2 : mn;
    mx = x2 > mx ? x2 : mx;
  }
  if ((t & 63) == 0) { tlo[t >> 6] = mn; thi[t >> 6] = mx; }
  __syncthreads();
  for (int o = AVA_SPEC_PREP_T / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  {
    const int nfa = valid ? (int)((cnt + a.nstep - 1) / a.nstep) + 1 : 0;
    if (nfa <= a.maxframes)
      for (int j = t; j < nfa; j += AVA_SPEC_PREP_T) a.ftimes[(size_t)w * a.maxframes + j] = frame_time(j, a, t1 > 0.0 ? t1 : 0.0);
  }
  if (t == 0) {
    SpecMeta m;
    m.lo = base + lo;
    m.n = valid ? (int)cnt : 0;
    // boundary='zeros' adds nperseg/2 on both sides, padded=True fills up to a whole number of hops:
    // frames = ceil(n / hop) + 1
    int nf = valid ? (int)((cnt + a.nstep - 1) / a.nstep) + 1 : 0;
    if (nf > a.maxframes) nf = -1;                                 // caller's max_samples was too small: poisoned below
    m.nframes = nf;
    m.mean = (valid && a.remove_dc) ? red[0] / (double)cnt : 0.0;
    m.t_shift = t1 > 0.0 ? t1 : 0.0;
    for (int i = 1; i < AVA_SPEC_PREP_T / 64; ++i) {
      mn = tlo[i] < mn ? tlo[i] : mn;
      mx = thi[i] > mx ? thi[i] : mx;
    }
    // frames l, l+1 bracket a target time x when l = floor((x - t_0) fs / hop); two frames of slack either side
    int j0 = 0, j1 = nf - 1;
    if (nf > 0) {
      const double x0 = frame_time(0, a, m.t_shift), per = a.fs / (double)a.nstep;
      const double f0 = floor((mn - x0) * per) - 2.0, f1 = floor((mx - x0) * per) + 3.0;
      if (f0 > 0.0) j0 = f0 < (double)(nf - 1) ? (int)f0 : nf - 1;
      if (f1 < (double)(nf - 1)) j1 = f1 > 0.0 ? (int)f1 : 0;
    }
    m.j0 = j0; m.j1 = j1;
    a.meta[w] = m;
    if (a.out_max != nullptr) a.out_max[w] = 0.f;
  }
}

// Frames of one window (the shared transform of stft.h).  A workgroup walks the needed frames of its window with
// stride gridDim.x; the twiddle table is loaded once.
template <int LOGN>
__global__ __launch_bounds__(256) void spec_stft_kernel(const SpecArgs a) {
  constexpr int N = 1 << LOGN, H = N / 2;
  __shared__ double re[stft_lds(H)], im[stft_lds(H)];
  __shared__ double twr[stft_lds(H)], twi[stft_lds(H)];       // exp(-2 pi i k / N), k < N/2
  const int w = blockIdx.y, t = threadIdx.x;
  const SpecMeta m = a.meta[w];
  if (m.nframes <= 0 || m.j0 + (int)blockIdx.x > m.j1) return;
  for (int k = t; k < H; k += 256) {
    twr[stft_pd(k)] = a.twiddle[2 * k];
    twi[stft_pd(k)] = a.twiddle[2 * k + 1];
  }
  const int k0 = a.krange[0], k1 = a.krange[1];             // bins outside are never read by the interpolation
  auto frame = [&](int j) {                                   // frame j of the slice minus its mean
    const long long c = (long long)j * a.nstep;
    return [&a, &m, c](long long p, bool live) {
      const long long idx = c + p;
      const bool in = live && idx >= 0 && idx < m.n;
      const double x = audio_at(a.audio, a.dtype, m.lo + (in ? idx : 0));
      return in ? x - m.mean : 0.0;
    };
  };
  auto logmag = [&](int j) {
    double* dst = a.logmag + ((size_t)w * a.maxframes + j) * (H + 1);
    for (int k = k0 + t; k <= k1; k += 256)
      dst[k] = stft_logmag(stft_bin<LOGN>(k, re, im, twr, twi), a.scale, AVA_SPEC_EPS);
  };
  stft_frames<LOGN, 256>(m.j0 + (int)blockIdx.x, m.j1 + 1, (int)gridDim.x, a.window, re, im, twr, twi, frame, logmag);
}

// The same for a segment length that is NOT a power of two (the reference hands any nperseg to scipy.signal.stft,
// ava/preprocessing/utils.py:66-68; scipy's pocketfft takes any length): the one-sided spectrum by direct summation in fp64,
//   X_k = sum_n v_n exp(-2 pi i (k n mod N) / N),   v = (x - mean) * window,
// for the bins k0 .. k1 the interpolation can touch only.  The frame and the N twiddles live in LDS; a thread owns a bin and walks
// n with the table index advanced by k modulo N (exact integer arithmetic: no argument reduction error).  N^2 work instead of
// N log N -- 0.3 ms for a batch of 256 windows at N = 400 -- on a path whose power-of-two lengths (every example script of the
// reference uses 512 or 1024) keep the radix-2 kernel above.  Error of a direct sum: <= N eps sum |v|, as pocketfft's to a factor.
#define AVA_SPEC_DFT_MAXN 2048
__global__ __launch_bounds__(256) void spec_dft_kernel(const SpecArgs a) {
  __shared__ double v[AVA_SPEC_DFT_MAXN];
  __shared__ double twr[AVA_SPEC_DFT_MAXN], twi[AVA_SPEC_DFT_MAXN];
  const int w = blockIdx.y, t = threadIdx.x, N = a.nperseg, K1 = N / 2;
  const SpecMeta m = a.meta[w];
  if (m.nframes <= 0 || m.j0 + (int)blockIdx.x > m.j1) return;
  for (int k = t; k < N; k += 256) {
    twr[k] = a.twiddle[2 * k];
    twi[k] = a.twiddle[2 * k + 1];
  }
  const int k0 = a.krange[0], k1 = a.krange[1];
  for (int j = m.j0 + blockIdx.x; j <= m.j1; j += gridDim.x) {
    __syncthreads();                                       // twiddles ready / previous frame's reads retired
    for (int i = t; i < N; i += 256) {
      const long long idx = (long long)j * a.nstep + i - N / 2;              // position in the slice (zeros outside)
      const bool in = idx >= 0 && idx < m.n;
      const double x = audio_at(a.audio, a.dtype, m.lo + (in ? idx : 0));
      v[i] = in ? __dmul_rn(x - m.mean, a.window[i]) : 0.0;
    }
    __syncthreads();
    double* dst = a.logmag + ((size_t)w * a.maxframes + j) * (K1 + 1);
    for (int k = k0 + t; k <= k1; k += 256) {
      double xr = 0.0, xi = 0.0;
      int q = 0;                                           // (k n) mod N
      for (int n = 0; n < N; ++n) {
        const double vn = v[n];
        xr = fma(vn, twr[q], xr);
        xi = fma(vn, twi[q], xi);
        q += k;
        if (q >= N) q -= N;
      }
      dst[k] = stft_logmag({xr, xi}, a.scale, AVA_SPEC_EPS);
    }
  }
}

int spec_frames_for(int max_samples, int nstep) { return (max_samples + nstep - 1) / nstep + 1; }

bool spec_shape_ok(int nperseg, int noverlap) {
  if (nperseg < 64 || nperseg > 2048) return false;       // a power of two: radix-2 kernel; any other length: direct transform
  return noverlap >= 0 && noverlap < nperseg;
}

// bytes of krange, meta, twiddle, ftimes and logmag behind the 256-byte alignment slack
static size_t spec_frames_bytes(int n, int max_samples, int nperseg, int noverlap) {
  const size_t frames = (size_t)spec_frames_for(max_samples, nperseg - noverlap);
  return 256 + 16 + (((size_t)n * sizeof(SpecMeta) + 15) & ~(size_t)15) + (size_t)2 * nperseg * sizeof(double) +
         (size_t)n * frames * sizeof(double) + (size_t)n * frames * (size_t)(nperseg / 2 + 1) * sizeof(double);
}

extern "C" size_t ava_spec_workspace_bytes(int n, int max_samples, int nperseg, int noverlap, int F, int T, int normalize) {
  if (n <= 0 || max_samples <= 0 || F <= 0 || T <= 0 || !spec_shape_ok(nperseg, noverlap)) return 0;
  return spec_frames_bytes(n, max_samples, nperseg, noverlap) + (normalize ? (size_t)n * F * T * sizeof(double) : 0);
}

void spec_carve(SpecArgs& a, void* ws, int n, int max_samples, int nperseg, int noverlap) {
  char* base = ava_align256(ws);
  a.krange = reinterpret_cast<int*>(base);
  base += 16;
  a.meta = reinterpret_cast<SpecMeta*>(base);
  a.twiddle = reinterpret_cast<double*>(base + (((size_t)n * sizeof(SpecMeta) + 15) & ~(size_t)15));
  a.ftimes = a.twiddle + 2 * nperseg;                 // room for the whole circle (lengths that are not a power of two)
  a.logmag = a.ftimes + (size_t)n * spec_frames_for(max_samples, nperseg - noverlap);
  a.vals = a.logmag + (size_t)n * spec_frames_for(max_samples, nperseg - noverlap) * (size_t)(nperseg / 2 + 1);
}

int spec_launch_frames(const SpecArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(spec_prep_kernel, dim3(a.n), dim3(AVA_SPEC_PREP_T), 0, st, a);
  AVA_CHECK_LAUNCH();
  const dim3 fgrid(a.maxframes < 24 ? a.maxframes : 24, a.n);    // a workgroup strides over its window's needed frames
  if ((a.nperseg & (a.nperseg - 1)) != 0) hipLaunchKernelGGL(spec_dft_kernel, fgrid, dim3(256), 0, st, a);
  else stft_dispatch(a.nperseg, [&](auto logn) {
    hipLaunchKernelGGL(spec_stft_kernel<decltype(logn)::value>, fgrid, dim3(256), 0, st, a);
  });
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

int spec_out_args(SpecOut& o, const double* target_times, const double* target_freqs, float* out, float* out_max, int n,
                  int F, int T, double fs, int nperseg, int noverlap, double spec_min, double spec_max, double fill_value,
                  int normalize, int q_lo, double q_gamma) {
  if (target_times == nullptr || target_freqs == nullptr || out == nullptr) return AVA_EINVAL;
  if (n <= 0 || F <= 0 || T <= 0 || T > AVA_SPEC_TMAX) return AVA_EINVAL;
  if (!(spec_max != spec_min)) return AVA_EINVAL;
  if (normalize && (q_lo < 0 || q_lo >= F * T || !(q_gamma >= 0.0 && q_gamma <= 1.0))) return AVA_EINVAL;
  o.target_times = target_times; o.target_freqs = target_freqs; o.out = out; o.out_max = out_max; o.vals = nullptr;
  o.normalize = normalize ? 1 : 0; o.q_lo = q_lo; o.q_gamma = q_gamma;
  o.fs = fs; o.spec_min = spec_min; o.range = spec_max - spec_min; o.fill_value = fill_value;
  o.fbin = spec_fbin(nperseg, fs);
  o.n = n; o.nperseg = nperseg; o.nstep = nperseg - noverlap; o.F = F; o.T = T;
  return AVA_OK;
}

extern "C" int ava_get_spec_batch(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                                  const int32_t* file_idx, const double* t1, const double* t2, const double* target_times,
                                  int n, int max_samples, double fs, int nperseg, int noverlap, const double* window,
                                  double scale, const double* target_freqs, int F, int T, double spec_min, double spec_max,
                                  double fill_value, int remove_dc, int normalize, int q_lo, double q_gamma, float* out,
                                  float* out_max, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (audio == nullptr || file_off == nullptr || file_len == nullptr || file_idx == nullptr || t1 == nullptr ||
      t2 == nullptr || window == nullptr)
    return AVA_EINVAL;
  if (max_samples <= 0 || !(fs > 0.0) || !spec_shape_ok(nperseg, noverlap)) return AVA_EINVAL;
  if (audio_dtype < AVA_AUDIO_I16 || audio_dtype > AVA_AUDIO_F64) return AVA_EINVAL;
  SpecArgs a;
  const int rc = spec_out_args(a, target_times, target_freqs, out, out_max, n, F, T, fs, nperseg, noverlap, spec_min,
                               spec_max, fill_value, normalize, q_lo, q_gamma);
  if (rc != AVA_OK) return rc;
  if (ws == nullptr || ws_bytes < ava_spec_workspace_bytes(n, max_samples, nperseg, noverlap, F, T, normalize)) return AVA_EWORKSPACE;
  a.audio = audio; a.file_off = reinterpret_cast<const long long*>(file_off);
  a.file_len = reinterpret_cast<const long long*>(file_len); a.file_idx = file_idx;
  a.t1 = t1; a.t2 = t2; a.window = window;
  spec_carve(a, ws, n, max_samples, nperseg, noverlap);
  a.scale = scale; a.maxframes = spec_frames_for(max_samples, a.nstep);
  a.dtype = audio_dtype; a.remove_dc = remove_dc;
  hipStream_t st = to_stream(s);
  const int frc = spec_launch_frames(a, st);
  return frc != AVA_OK ? frc : spec_launch_out(a, st);
}
