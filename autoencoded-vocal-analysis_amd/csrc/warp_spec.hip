// Time-warped shotgun windows on the device: WarpedWindowDataset.__getitem__ of the
// reference (ava/models/window_vae_dataset.py:589-640) calls get_spec(0.0, template_dur, audio[file], ..., target_times)
// for EVERY window, i.e. transforms the whole motif and interpolates num_time_bins columns out of it.  The slice, its
// mean and its log-spectrogram are the same for every window of a file, so they are made once:
//
//   ava_warp_cache_build   per file: the slice [0, min(len, round(template_dur fs))), the "too short" rule, the mean, every
//                          STFT frame, log(|.| + 1e-12)     spec_prep_kernel + spec_stft_kernel / spec_dft_kernel of spec.hip,
//                          run with one "window" per file (spec_launch_frames), then
//                          warp_pack_kernel: [file][bin][frame] for the bins the target frequencies can touch
//   ava_warp_windows       per batch: warp_interp_kernel (1 workgroup / 16 rows of a window), interpolation straight out
//                          of the cache under each window's own target times; warp_normalize_kernel if asked for
//
// No arithmetic is restated here: the frames are spec.hip's kernels, and the interpolation, the fill rule, the
// normalisation, the clip and within_syll_normalize are the functions of spec_core.h that spec.hip's kernels call, on
// the same fp64 inputs.  A window out of the cache is therefore bit-identical to ava_get_spec_batch(0, template_dur) on
// the same target times.
#include "spec_core.h"

struct WarpLayout {                // the cache: [nframes int[files]] [ftimes double[files][maxframes]] [logmag]
  int max_samples, maxframes, fstride, k0, nb;
  size_t off_ftimes, off_logmag, bytes;      // offsets behind the 256-byte alignment of the caller's pointer
};

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

static bool warp_layout(int files, double template_dur, double fs, int nperseg, int noverlap, double fmin, double fmax,
                        WarpLayout* L) {
  if (files <= 0 || files > 65535 || !(fs > 0.0) || !(template_dur > 0.0) || !spec_shape_ok(nperseg, noverlap)) return false;
  if (!(fmin <= fmax)) return false;
  const double s2 = rint(template_dur * fs);               // int(round(t2 * fs)), utils.py:59
  if (!(s2 >= 1.0 && s2 < 2147483647.0)) return false;
  L->max_samples = (int)s2;
  L->maxframes = spec_frames_for(L->max_samples, nperseg - noverlap);
  L->fstride = (L->maxframes + 15) & ~15;                  // rows start on 128-byte lines
  int k1;
  spec_bin_range(fmin, fmax, spec_fbin(nperseg, fs), nperseg, &L->k0, &k1);
  L->nb = k1 - L->k0 + 1;
  if (L->nb < 2) return false;
  L->off_ftimes = up256((size_t)files * sizeof(int));
  L->off_logmag = L->off_ftimes + up256((size_t)files * L->maxframes * sizeof(double));
  L->bytes = 256 + L->off_logmag + (size_t)files * L->nb * L->fstride * sizeof(double);
  return true;
}

static inline char* align256(const void* p) {
  char* base = reinterpret_cast<char*>(const_cast<void*>(p));
  return base + ((256 - (reinterpret_cast<uintptr_t>(base) & 255)) & 255);
}

// the per-"window" inputs of spec_prep_kernel for one window per file: the whole motif, every frame, every bin in range
__global__ __launch_bounds__(256) void warp_args_kernel(int files, double template_dur, double fmin, double fmax,
                                                        int* file_idx, double* t1, double* t2, double* tt, double* tf) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f == 0) { tf[0] = fmin; tf[1] = fmax; }
  if (f >= files) return;
  file_idx[f] = f;
  t1[f] = 0.0;
  t2[f] = template_dur;
  tt[2 * f] = -1e300;                                       // every frame is needed
  tt[2 * f + 1] = 1e300;
}

// [file][frame][K] of spec.hip's scratch -> [file][bin - k0][frame] of the cache (zeros behind a file's last frame)
__global__ __launch_bounds__(256) void warp_pack_kernel(const SpecMeta* meta, const double* ftimes, const double* logmag,
                                                        int files, int maxframes, int fstride, int K, int k0, int nb,
                                                        int* c_nframes, double* c_ftimes, double* c_logmag) {
  const int f = blockIdx.y, t = threadIdx.x;
  if (f >= files) return;
  const int nf = meta[f].nframes;
  if (blockIdx.x == 0) {
    if (t == 0) c_nframes[f] = nf;
    for (int j = t; j < maxframes; j += 256) c_ftimes[(size_t)f * maxframes + j] = j < nf ? ftimes[(size_t)f * maxframes + j] : 0.0;
  }
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    double* dst = c_logmag + ((size_t)f * nb + b) * fstride;
    const int k = k0 + b;
    for (int j = t; j < fstride; j += 256)
      dst[j] = (j < nf && k < K) ? logmag[((size_t)f * maxframes + j) * K + k] : 0.0;
  }
}

struct WarpArgs {
  const int* c_nframes;          // the cache
  const double* c_ftimes;
  const double* c_logmag;
  const int* file_idx;           // [n]
  const double* target_times;    // [n][T]
  const double* target_freqs;    // [F]
  float* out;                    // [n][F][T]
  double* vals;                  // [n][F*T] (normalize only)
  double fs, spec_min, range, fill_value, fbin, q_gamma;
  int n, files, maxframes, fstride, k0, nb, nperseg, nstep, F, T, normalize, q_lo;
};

// frames of window w's file: 0 where get_spec returns zeros (utils.py:68-69), -1 for a file index out of range
__device__ __forceinline__ int warp_nframes(const WarpArgs& a, int w, int* file) {
  const int f = a.file_idx[w];
  *file = f;
  return (f < 0 || f >= a.files) ? -1 : a.c_nframes[f];
}

// spec_interp_kernel's grid and tables over the cache: a workgroup owns AVA_SPEC_ROWS frequency rows of one window; the
// knot interval and basis values of every target time are computed once per workgroup into LDS.  Consecutive threads
// take consecutive target times, whose frames l are equal or adjacent: the four coefficient loads of a wave fall in two
// rows [bin q], [bin q + 1] of the cache, contiguous along frames.
__global__ __launch_bounds__(256) void warp_interp_kernel(const WarpArgs a) {
  __shared__ double chx0[AVA_SPEC_TMAX], chx1[AVA_SPEC_TMAX];
  __shared__ int cl[AVA_SPEC_TMAX];
  __shared__ double rhy0[AVA_SPEC_ROWS], rhy1[AVA_SPEC_ROWS];
  __shared__ int rq[AVA_SPEC_ROWS];
  const int w = blockIdx.y, f0 = blockIdx.x * AVA_SPEC_ROWS, t = threadIdx.x;
  int file;
  const int nf = warp_nframes(a, w, &file);
  const int rows = a.F - f0 < AVA_SPEC_ROWS ? a.F - f0 : AVA_SPEC_ROWS;
  float* obase = a.out + ((size_t)w * a.F + f0) * a.T;
  if (nf <= 0) {
    const float z = nf == 0 ? 0.f : __builtin_nanf("");
    for (int i = t; i < rows * a.T; i += 256) obase[i] = z;
    return;
  }
  const int K = a.nperseg / 2 + 1;
  const double* ft = a.c_ftimes + (size_t)file * a.maxframes;
  for (int ti = t; ti < a.T; ti += 256)
    spec_time_basis(a.target_times[(size_t)w * a.T + ti], ft, nf, a.fs, a.nstep, &cl[ti], &chx0[ti], &chx1[ti]);
  if (t < rows) spec_freq_basis(a.target_freqs[f0 + t], a.fbin, K, &rq[t], &rhy0[t], &rhy1[t]);
  __syncthreads();
  const double* cfile = a.c_logmag + (size_t)file * a.nb * a.fstride;
  for (int i = t; i < rows * a.T; i += 256) {
    const int r = i / a.T, ti = i - r * a.T;
    const int l = cl[ti], q = rq[r];
    double v;
    if (l < 0 || q < 0) {
      v = a.fill_value;
    } else {
      int b = q - a.k0;                                     // inside [0, nb - 2] by the slack of spec_bin_range
      b = b < 0 ? 0 : (b > a.nb - 2 ? a.nb - 2 : b);
      const double* c0 = cfile + (size_t)b * a.fstride + l;                      // [freq q][time l]
      const double* c1 = c0 + a.fstride;                                         // [freq q + 1][time l]
      v = spec_bilinear(c0[0], c1[0], c0[1], c1[1], chx0[ti], chx1[ti], rhy0[r], rhy1[r]);
    }
    v = spec_scale_clip(v, a.spec_min, a.range);
    if (a.normalize) a.vals[((size_t)w * a.F + f0) * a.T + i] = v;
    else obase[i] = (float)v;
  }
}

__global__ __launch_bounds__(AVA_SPEC_NORM_T) void warp_normalize_kernel(const WarpArgs a) {
  const int w = blockIdx.x;
  int file;
  if (warp_nframes(a, w, &file) <= 0) return;               // zeros (or the NaN marker) were written already
  const int n = a.F * a.T;
  spec_normalize_window(a.vals + (size_t)w * n, a.out + (size_t)w * n, n, a.q_lo, a.q_gamma, nullptr);
}

extern "C" size_t ava_warp_cache_bytes(int files, double template_dur, double fs, int nperseg, int noverlap, double fmin,
                                       double fmax) {
  WarpLayout L;
  return warp_layout(files, template_dur, fs, nperseg, noverlap, fmin, fmax, &L) ? L.bytes : 0;
}

// scratch of the build: the per-file arguments, then the regions spec_launch_frames fills
static size_t warp_args_bytes(int files) {
  return up256((size_t)files * sizeof(int)) + 2 * up256((size_t)files * sizeof(double)) +
         up256((size_t)2 * files * sizeof(double)) + 256;
}

extern "C" size_t ava_warp_cache_workspace_bytes(int files, double template_dur, double fs, int nperseg, int noverlap) {
  WarpLayout L;
  if (!warp_layout(files, template_dur, fs, nperseg, noverlap, 0.0, 0.0, &L)) return 0;
  return 256 + warp_args_bytes(files) + ava_spec_workspace_bytes(files, L.max_samples, nperseg, noverlap, 2, 2, 0);
}

extern "C" int ava_warp_cache_build(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                                    int files, double template_dur, double fs, int nperseg, int noverlap,
                                    const double* window, double scale, double fmin, double fmax, int remove_dc,
                                    void* cache, size_t cache_bytes, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (audio == nullptr || file_off == nullptr || file_len == nullptr || window == nullptr || cache == nullptr) return AVA_EINVAL;
  if (audio_dtype < AVA_AUDIO_I16 || audio_dtype > AVA_AUDIO_F64) return AVA_EINVAL;
  WarpLayout L;
  if (!warp_layout(files, template_dur, fs, nperseg, noverlap, fmin, fmax, &L)) return AVA_EINVAL;
  if (cache_bytes < L.bytes) return AVA_EWORKSPACE;
  if (ws == nullptr || ws_bytes < ava_warp_cache_workspace_bytes(files, template_dur, fs, nperseg, noverlap)) return AVA_EWORKSPACE;
  char* base = align256(ws);
  int* file_idx = reinterpret_cast<int*>(base);
  base += up256((size_t)files * sizeof(int));
  double* t1 = reinterpret_cast<double*>(base);
  base += up256((size_t)files * sizeof(double));
  double* t2 = reinterpret_cast<double*>(base);
  base += up256((size_t)files * sizeof(double));
  double* tt = reinterpret_cast<double*>(base);
  base += up256((size_t)2 * files * sizeof(double));
  double* tf = reinterpret_cast<double*>(base);
  base += 256;
  hipStream_t st = to_stream(s);
  hipLaunchKernelGGL(warp_args_kernel, dim3(ceil_div(files, 256)), dim3(256), 0, st, files, template_dur, fmin, fmax, file_idx,
                     t1, t2, tt, tf);
  AVA_CHECK_LAUNCH();
  SpecArgs a;
  a.audio = audio; a.file_off = reinterpret_cast<const long long*>(file_off);
  a.file_len = reinterpret_cast<const long long*>(file_len); a.file_idx = file_idx;
  a.t1 = t1; a.t2 = t2; a.target_times = tt; a.target_freqs = tf; a.window = window;
  spec_carve(a, base, files, L.max_samples, nperseg, noverlap);
  a.vals = nullptr; a.out = nullptr; a.out_max = nullptr;
  a.normalize = 0; a.q_lo = 0; a.q_gamma = 0.0;
  a.fs = fs; a.scale = scale; a.spec_min = 0.0; a.range = 1.0; a.fill_value = 0.0;
  a.fbin = spec_fbin(nperseg, fs);
  a.n = files; a.nperseg = nperseg; a.nstep = nperseg - noverlap; a.maxframes = L.maxframes;
  a.F = 2; a.T = 2; a.dtype = audio_dtype; a.remove_dc = remove_dc;
  const int rc = spec_launch_frames(a, st);
  if (rc != AVA_OK) return rc;
  char* c = align256(cache);
  hipLaunchKernelGGL(warp_pack_kernel, dim3(L.nb < 64 ? L.nb : 64, files), dim3(256), 0, st, a.meta, a.ftimes, a.logmag, files,
                     L.maxframes, L.fstride, nperseg / 2 + 1, L.k0, L.nb, reinterpret_cast<int*>(c),
                     reinterpret_cast<double*>(c + L.off_ftimes), reinterpret_cast<double*>(c + L.off_logmag));
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" size_t ava_warp_windows_workspace_bytes(int n, int F, int T, int normalize) {
  if (n <= 0 || F <= 0 || T <= 0) return 0;
  return 256 + (normalize ? (size_t)n * F * T * sizeof(double) : 0);
}

extern "C" int ava_warp_windows(const void* cache, size_t cache_bytes, int files, double template_dur, double fs,
                                int nperseg, int noverlap, double fmin, double fmax, const int32_t* file_idx,
                                const double* target_times, int n, const double* target_freqs, int F, int T,
                                double spec_min, double spec_max, double fill_value, int normalize, int q_lo,
                                double q_gamma, float* out, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (cache == nullptr || file_idx == nullptr || target_times == nullptr || target_freqs == nullptr || out == nullptr)
    return AVA_EINVAL;
  if (n <= 0 || F <= 0 || T <= 0 || T > AVA_SPEC_TMAX) return AVA_EINVAL;
  if (!(spec_max != spec_min)) return AVA_EINVAL;
  if (normalize && (q_lo < 0 || q_lo >= F * T || !(q_gamma >= 0.0 && q_gamma <= 1.0))) return AVA_EINVAL;
  WarpLayout L;
  if (!warp_layout(files, template_dur, fs, nperseg, noverlap, fmin, fmax, &L)) return AVA_EINVAL;
  if (cache_bytes < L.bytes) return AVA_EWORKSPACE;
  if (normalize && (ws == nullptr || ws_bytes < ava_warp_windows_workspace_bytes(n, F, T, 1))) return AVA_EWORKSPACE;
  const char* c = align256(cache);
  WarpArgs a;
  a.c_nframes = reinterpret_cast<const int*>(c);
  a.c_ftimes = reinterpret_cast<const double*>(c + L.off_ftimes);
  a.c_logmag = reinterpret_cast<const double*>(c + L.off_logmag);
  a.file_idx = file_idx; a.target_times = target_times; a.target_freqs = target_freqs;
  a.out = out;
  a.vals = normalize ? reinterpret_cast<double*>(align256(ws)) : nullptr;
  a.fs = fs; a.spec_min = spec_min; a.range = spec_max - spec_min; a.fill_value = fill_value;
  a.fbin = spec_fbin(nperseg, fs); a.q_gamma = q_gamma;
  a.n = n; a.files = files; a.maxframes = L.maxframes; a.fstride = L.fstride; a.k0 = L.k0; a.nb = L.nb;
  a.nperseg = nperseg; a.nstep = nperseg - noverlap; a.F = F; a.T = T; a.normalize = normalize ? 1 : 0; a.q_lo = q_lo;
  hipStream_t st = to_stream(s);
  hipLaunchKernelGGL(warp_interp_kernel, dim3(ceil_div(F, AVA_SPEC_ROWS), n), dim3(256), 0, st, a);
  AVA_CHECK_LAUNCH();
  if (normalize) {
    hipLaunchKernelGGL(warp_normalize_kernel, dim3(n), dim3(AVA_SPEC_NORM_T), 0, st, a);
    AVA_CHECK_LAUNCH();
  }
  return AVA_OK;
}
