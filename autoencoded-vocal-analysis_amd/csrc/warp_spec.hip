// Time-warped shotgun windows on the device: WarpedWindowDataset.__getitem__ of the
// reference (ava/models/window_vae_dataset.py:589-640) calls get_spec(0.0, template_dur, audio[file], ..., target_times)
// for EVERY window, i.e. transforms the whole motif and interpolates num_time_bins columns out of it.  The slice, its
// mean and its log-spectrogram are the same for every window of a file, so they are made once:
//
//   ava_warp_cache_build   per file: the slice [0, min(len, round(template_dur fs))), the "too short" rule, the mean, every
//                          STFT frame, log(|.| + 1e-12)     spec_prep_kernel + spec_stft_kernel / spec_dft_kernel of spec.hip,
//                          run with one "window" per file (spec_launch_frames), then
//                          warp_pack_kernel: [file][bin][frame] for the bins the target frequencies can touch
//   ava_warp_windows       per batch: spec_interp_kernel of spec_core.h (1 workgroup / 16 rows of a window) with the
//                          cache as its coefficient source, under each window's own target times; spec_normalize_kernel
//                          if asked for
//
// No arithmetic and no kernel of the window path is restated here: the frames are spec.hip's kernels, and the
// interpolation and normalisation are the kernels ava_get_spec_batch launches, reading [file][bin][frame] out of the
// cache instead of [window][frame][bin] out of the scratch.  A window out of the cache is therefore bit-identical to
// ava_get_spec_batch(0, template_dur) on the same target times.
#include "spec_core.h"

struct WarpLayout {                // the cache: [nframes int[files]] [ftimes double[files][maxframes]] [logmag]
  int max_samples, maxframes, fstride, k0, nb;
  size_t off_ftimes, off_logmag, bytes;      // offsets behind the 256-byte alignment of the caller's pointer
};

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
  L->off_ftimes = ava_up256((size_t)files * sizeof(int));
  L->off_logmag = L->off_ftimes + ava_up256((size_t)files * L->maxframes * sizeof(double));
  L->bytes = 256 + L->off_logmag + (size_t)files * L->nb * L->fstride * sizeof(double);
  return true;
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

// The cache as a coefficient source of spec_interp_kernel (spec_core.h).  Consecutive threads take consecutive target
// times, whose frames l are equal or adjacent: the four coefficient loads of a wave fall in two rows [bin q], [bin q + 1]
// of the cache, contiguous along frames.
struct WarpCacheWindow {
  int nframes;
  const double* ftimes;
  const double* logmag;          // [bin - k0][fstride] of the window's file
  int fstride, k0, nb;
  __device__ __forceinline__ SpecCoef coef(int l, int q) const {
    int b = q - k0;                                         // inside [0, nb - 2] by the slack of spec_bin_range
    b = b < 0 ? 0 : (b > nb - 2 ? nb - 2 : b);
    const double* c0 = logmag + (size_t)b * fstride + l;
    const double* c1 = c0 + fstride;
    return {c0[0], c1[0], c0[1], c1[1]};
  }
};

struct WarpArgs : SpecOut {
  const int* c_nframes;          // the cache
  const double* c_ftimes;
  const double* c_logmag;
  const int* file_idx;           // [n]
  int files, maxframes, fstride, k0, nb;
  // frames of window w's file: 0 where get_spec returns zeros (utils.py:68-69), -1 for a file index out of range
  __device__ __forceinline__ WarpCacheWindow window_of(int w) const {
    const int f = file_idx[w];
    if (f < 0 || f >= files) return {-1, nullptr, nullptr, fstride, k0, nb};
    return {c_nframes[f], c_ftimes + (size_t)f * maxframes, c_logmag + (size_t)f * nb * fstride, fstride, k0, nb};
  }
};

extern "C" size_t ava_warp_cache_bytes(int files, double template_dur, double fs, int nperseg, int noverlap, double fmin,
                                       double fmax) {
  WarpLayout L;
  return warp_layout(files, template_dur, fs, nperseg, noverlap, fmin, fmax, &L) ? L.bytes : 0;
}

// scratch of the build: the per-file arguments, then the regions spec_launch_frames fills
static size_t warp_args_bytes(int files) {
  return ava_up256((size_t)files * sizeof(int)) + 2 * ava_up256((size_t)files * sizeof(double)) +
         ava_up256((size_t)2 * files * sizeof(double)) + 256;
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
  char* base = ava_align256(ws);
  int* file_idx = reinterpret_cast<int*>(base);
  base += ava_up256((size_t)files * sizeof(int));
  double* t1 = reinterpret_cast<double*>(base);
  base += ava_up256((size_t)files * sizeof(double));
  double* t2 = reinterpret_cast<double*>(base);
  base += ava_up256((size_t)files * sizeof(double));
  double* tt = reinterpret_cast<double*>(base);
  base += ava_up256((size_t)2 * files * sizeof(double));
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
  char* c = ava_align256(cache);
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

extern "C" int ava_warp_cache_layout(int files, double template_dur, double fs, int nperseg, int noverlap, double fmin,
                                     double fmax, int64_t out[6]) {
  WarpLayout L;
  if (out == nullptr || !warp_layout(files, template_dur, fs, nperseg, noverlap, fmin, fmax, &L)) return AVA_EINVAL;
  out[0] = L.maxframes; out[1] = L.fstride; out[2] = L.k0; out[3] = L.nb;
  out[4] = (int64_t)L.off_ftimes; out[5] = (int64_t)L.off_logmag;
  return AVA_OK;
}

extern "C" int ava_warp_windows(const void* cache, size_t cache_bytes, int files, double template_dur, double fs,
                                int nperseg, int noverlap, double fmin, double fmax, const int32_t* file_idx,
                                const double* target_times, int n, const double* target_freqs, int F, int T,
                                double spec_min, double spec_max, double fill_value, int normalize, int q_lo,
                                double q_gamma, float* out, void* ws, size_t ws_bytes, ava_stream_t s) {
  if (cache == nullptr || file_idx == nullptr) return AVA_EINVAL;
  WarpArgs a;
  const int rc = spec_out_args(a, target_times, target_freqs, out, nullptr, n, F, T, fs, nperseg, noverlap, spec_min,
                               spec_max, fill_value, normalize, q_lo, q_gamma);
  if (rc != AVA_OK) return rc;
  WarpLayout L;
  if (!warp_layout(files, template_dur, fs, nperseg, noverlap, fmin, fmax, &L)) return AVA_EINVAL;
  if (cache_bytes < L.bytes) return AVA_EWORKSPACE;
  if (normalize && (ws == nullptr || ws_bytes < ava_warp_windows_workspace_bytes(n, F, T, 1))) return AVA_EWORKSPACE;
  const char* c = ava_align256(cache);
  a.c_nframes = reinterpret_cast<const int*>(c);
  a.c_ftimes = reinterpret_cast<const double*>(c + L.off_ftimes);
  a.c_logmag = reinterpret_cast<const double*>(c + L.off_logmag);
  a.file_idx = file_idx;
  a.vals = normalize ? reinterpret_cast<double*>(ava_align256(ws)) : nullptr;
  a.files = files; a.maxframes = L.maxframes; a.fstride = L.fstride; a.k0 = L.k0; a.nb = L.nb;
  return spec_launch_out(a, to_stream(s));
}
