// Template segmentation on the device: the arithmetic core of
// ava/segmenting/template_segmentation.py:_segment_file for every recording of a DeviceAudio at once.
//
//   _get_spec (lines 758-790, = segmenting/utils.py:get_spec): scipy.signal.stft of the whole file (hann, zero boundary,
//   zero padded to whole hops, 'spectrum' scaling), bins [searchsorted(f, min_freq), searchsorted(f, max_freq)),
//   clip((log(|X| + 1e-9) - min) / (max - min), 0, 1); plus the sum of every frame over the band
//                                                                   tpl_spec_kernel   (workgroups stride over frames)
//   the normalised cross-correlation (lines 240-245) of file f at lags i = 0 .. n_f - L - 1:
//     mu_i = sum_{t<L} framesum[i + t] / (F L)                      tpl_mean_kernel   (1 thread / lag)
//     N_i  = sum_{k<F, t<L} T[k, t] (S[k, i + t] - mu_i),  Q_i = sum (S[k, i + t] - mu_i)^2,  r_i = N_i / (Q_i + 1e-9)
//                                                                   tpl_xcorr_kernel  (1 workgroup / tile of lags)
//
// The reference's quirks stay: n_f - L lags (not n_f - L + 1), and r divides by the sum of squares, not its root.
// Every product uses S - mu_i (centred): a patch that is all 0.0 or all 1.0 gives exactly 0, as in the reference,
// although the template's own sum is not zero.  All arithmetic is fp64.  Each lag's sums run in one fixed order
// (bin chunk, frame chunk, bin, frame), the same wherever the lag sits in its tile and whichever files share the
// launch: the trace is bit-reproducible.  The host (ava_amd/template_segmentation.py) runs the threshold, the maxima
// and _clean_max_indices on the trace.
#include "stft.h"

#define AVA_TPL_EPS 1e-9
#define AVA_TPL_T 256            // threads of the spectrogram and mean kernels

// Correlation tiles.  A workgroup of XT threads owns TILE = XT * R consecutive lags of one
// file; thread x owns lags R x .. R x + R - 1, so every spectrogram value it reads from LDS serves R lags (a sliding
// window of R registers).  Per step the workgroup stages KC bins x LC frames of the template and the KC x (TILE + LC - 1)
// spectrogram values those lags need.  LDS row layout: frame p of a row at [p % R][p / R], so that the R-strided
// reads of a wave hit consecutive doubles (ds_read_b64 conflict-free); WR = (TILE + LC) / R + 4 makes the staging
// stores conflict-free as well (WR % 16 == 4).
#define AVA_TPL_XT 128
#define AVA_TPL_R 4
#define AVA_TPL_TILE (AVA_TPL_XT * AVA_TPL_R)
#define AVA_TPL_KC 4
#define AVA_TPL_LC 64
#define AVA_TPL_WR ((AVA_TPL_TILE + AVA_TPL_LC) / AVA_TPL_R + 4)
static_assert(AVA_TPL_LC % AVA_TPL_R == 0, "frame chunks hold whole register windows");
static_assert(AVA_TPL_WR % 16 == 4, "conflict-free staging stores");

struct TplSpecArgs {
  const void* audio;
  const long long* file_off;     // [files] first sample of each file in `audio`
  const long long* file_len;     // [files] samples of each file
  const long long* frame_off;    // [files + 1] first global frame of each file; frame_off[files] = frames
  const double* window;          // [nperseg]
  double* spec;                  // [k1 - k0][frames] band spectrogram
  double* frame_sum;             // [frames] sum of spec over the band
  double scale, spec_min, range;
  long long frames;
  int files, nstep, k0, k1, dtype;
};

// One workgroup per frame, striding over all frames of all files: the shared transform of stft.h, the clipped band
// values, and their sum in a fixed order (thread partial sums, the waves' shuffles, the four waves in order).
template <int LOGN>
__global__ __launch_bounds__(AVA_TPL_T) void tpl_spec_kernel(const TplSpecArgs a) {
  constexpr int N = 1 << LOGN, H = N / 2;
  __shared__ double re[stft_lds(H)], im[stft_lds(H)];
  __shared__ double twr[stft_lds(H)], twi[stft_lds(H)];       // exp(-2 pi i k / N), k < N/2
  __shared__ double red[AVA_TPL_T / 64];
  const int t = threadIdx.x;
  for (int k = t; k < H; k += AVA_TPL_T) {
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
    double s = 0.0;
    for (int k = a.k0 + t; k < a.k1; k += AVA_TPL_T) {
      const double lg = stft_logmag(stft_bin<LOGN>(k, re, im, twr, twi), a.scale, AVA_TPL_EPS);
      double v = __ddiv_rn(__dsub_rn(lg, a.spec_min), a.range);
      v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
      a.spec[(size_t)(k - a.k0) * a.frames + g] = v;
      s += v;
    }
    s = wave_sum_d(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
      double v = 0.0;
#pragma unroll
      for (int w = 0; w < AVA_TPL_T / 64; ++w) v += red[w];
      a.frame_sum[g] = v;
    }
  };
  stft_frames<LOGN, AVA_TPL_T>((long long)blockIdx.x, a.frames, (long long)gridDim.x, a.window, re, im, twr, twi, frame,
                               band);
}

struct TplXcorrArgs {
  const double* spec;            // [F][frames]
  const double* frame_sum;       // [frames]
  const long long* frame_off;    // [files + 1]
  const long long* lag_off;      // [files + 1] first global lag of each file; lag_off[files] = lags
  const long long* tile_off;     // [files + 1] first tile of each file; tile_off[files] = tiles
  const double* tmpl;            // [F][L]
  double* mu;                    // [lags] (workspace)
  double* trace;                 // [lags]
  long long frames, lags;
  int files, F, L;
};

// lags of file f: what lag_off grants, never more than n_f - L (so that no window reads past its file)
__device__ __forceinline__ long long tpl_lags_of(const TplXcorrArgs& a, int f) {
  const long long n = a.lag_off[f + 1] - a.lag_off[f], cap = a.frame_off[f + 1] - a.frame_off[f] - a.L;
  return n < cap ? n : cap;
}

// mu of every lag: its L frame sums in order, over F L
__global__ __launch_bounds__(AVA_TPL_T) void tpl_mean_kernel(const TplXcorrArgs a) {
  const long long l = (long long)blockIdx.x * AVA_TPL_T + threadIdx.x;
  if (l >= a.lags) return;
  const int f = stft_file_of(a.lag_off, a.files, l);
  const long long i = l - a.lag_off[f];
  if (i >= tpl_lags_of(a, f)) return;
  const double* fs = a.frame_sum + a.frame_off[f] + i;
  double s = 0.0;
  for (int t = 0; t < a.L; ++t) s += fs[t];
  a.mu[l] = __ddiv_rn(s, (double)a.F * (double)a.L);
}

__global__ __launch_bounds__(AVA_TPL_XT) void tpl_xcorr_kernel(const TplXcorrArgs a) {
  constexpr int R = AVA_TPL_R, KC = AVA_TPL_KC, LC = AVA_TPL_LC, WR = AVA_TPL_WR;
  __shared__ double sl[KC][R][WR];
  __shared__ double tl[KC][LC];
  const int x = threadIdx.x;
  const int f = stft_file_of(a.tile_off, a.files, (long long)blockIdx.x);
  const long long i0 = ((long long)blockIdx.x - a.tile_off[f]) * AVA_TPL_TILE;   // first lag of the tile in its file
  const long long nl = tpl_lags_of(a, f) - i0;
  if (nl <= 0) return;                                                           // (uniform)
  const int nt = nl < AVA_TPL_TILE ? (int)nl : AVA_TPL_TILE;                     // lags of this tile
  const long long g0 = a.frame_off[f] + i0, l0 = a.lag_off[f] + i0;              // its first frame, first global lag
  const int r0 = x * R;
  double mu[R], num[R], den[R], w[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    mu[j] = r0 + j < nt ? a.mu[l0 + r0 + j] : 0.0;
    num[j] = 0.0;
    den[j] = 0.0;
  }
  for (int kc = 0; kc < a.F; kc += KC) {
    const int kn = a.F - kc < KC ? a.F - kc : KC;
    for (int t0 = 0; t0 < a.L; t0 += LC) {
      const int lc = a.L - t0 < LC ? a.L - t0 : LC;
      const int width = nt + lc - 1;                                             // frames g0 + t0 + p, p < width
      __syncthreads();                                                           // the previous chunk's reads are done
      for (int e = x; e < KC * LC; e += AVA_TPL_XT) {
        const int kk = e / LC, t = e % LC;
        tl[kk][t] = kk < kn && t < lc ? a.tmpl[(size_t)(kc + kk) * a.L + t0 + t] : 0.0;
      }
      for (int kk = 0; kk < kn; ++kk) {
        const double* row = a.spec + (size_t)(kc + kk) * a.frames + g0 + t0;
        for (int p = x; p < width; p += AVA_TPL_XT) sl[kk][p % R][p / R] = row[p];
      }
      __syncthreads();
      for (int kk = 0; kk < kn; ++kk) {
        // w[q % R] holds the value at frame r0 + q (relative to the chunk); lag r0 + j at step s reads frame r0 + j + s
#pragma unroll
        for (int j = 0; j < R - 1; ++j) w[j] = sl[kk][j][x];
        for (int t = 0; t < lc; t += R) {
#pragma unroll
          for (int u = 0; u < R; ++u) {
            if (t + u < lc) {                                                    // (uniform)
              const int c = t + u + R - 1;
              w[(u + R - 1) % R] = sl[kk][(u + R - 1) % R][x + c / R];
              const double tv = tl[kk][t + u];
#pragma unroll
              for (int j = 0; j < R; ++j) {
                const double d = w[(u + j) % R] - mu[j];
                num[j] = fma(tv, d, num[j]);
                den[j] = fma(d, d, den[j]);
              }
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < R; ++j)
    if (r0 + j < nt) a.trace[l0 + r0 + j] = __ddiv_rn(num[j], __dadd_rn(den[j], AVA_TPL_EPS));
}

extern "C" size_t ava_tpl_workspace_bytes(int64_t lags) {
  if (lags <= 0) return 0;
  return 256 + (size_t)lags * sizeof(double);
}

extern "C" int ava_tpl_tile_lags(void) { return AVA_TPL_TILE; }

extern "C" int ava_tpl_spec(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                            const int64_t* frame_off, int files, int64_t frames, int nperseg, int noverlap,
                            const double* window, double scale, int k0, int k1, double spec_min, double spec_max,
                            double* spec, double* frame_sum, ava_stream_t s) {
  if (audio == nullptr || file_off == nullptr || file_len == nullptr || frame_off == nullptr || window == nullptr ||
      spec == nullptr || frame_sum == nullptr)
    return AVA_EINVAL;
  if (files <= 0 || frames <= 0) return AVA_EINVAL;
  if (nperseg < 64 || nperseg > 2048 || (nperseg & (nperseg - 1)) != 0) return AVA_EINVAL;
  if (noverlap < 0 || noverlap >= nperseg) return AVA_EINVAL;
  if (k0 < 0 || k1 <= k0 || k1 > nperseg / 2 + 1) return AVA_EINVAL;             // empty band
  if (audio_dtype < AVA_AUDIO_I16 || audio_dtype > AVA_AUDIO_F64) return AVA_EINVAL;
  if (!(spec_max != spec_min)) return AVA_EINVAL;
  TplSpecArgs a;
  a.audio = audio;
  a.file_off = reinterpret_cast<const long long*>(file_off);
  a.file_len = reinterpret_cast<const long long*>(file_len);
  a.frame_off = reinterpret_cast<const long long*>(frame_off);
  a.window = window;
  a.spec = spec;
  a.frame_sum = frame_sum;
  a.scale = scale; a.spec_min = spec_min; a.range = spec_max - spec_min;
  a.frames = frames; a.files = files; a.nstep = nperseg - noverlap;
  a.k0 = k0; a.k1 = k1; a.dtype = audio_dtype;
  const int grid = frames < 4096 ? (int)frames : 4096;      // workgroups stride over the frames
  stft_dispatch(nperseg, [&](auto logn) {
    hipLaunchKernelGGL(tpl_spec_kernel<decltype(logn)::value>, dim3(grid), dim3(AVA_TPL_T), 0, to_stream(s), a);
  });
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_tpl_xcorr(const double* spec, const double* frame_sum, int F, int64_t frames,
                             const int64_t* frame_off, const int64_t* lag_off, const int64_t* tile_off, int files,
                             int64_t lags, int64_t tiles, const double* tmpl, int template_F, int L, double* trace,
                             void* ws, size_t ws_bytes, ava_stream_t s) {
  if (spec == nullptr || frame_sum == nullptr || frame_off == nullptr || lag_off == nullptr || tile_off == nullptr ||
      tmpl == nullptr || trace == nullptr)
    return AVA_EINVAL;
  if (F <= 0 || L <= 0 || template_F != F || files <= 0 || frames <= 0 || lags <= 0 || tiles <= 0) return AVA_EINVAL;
  if (tiles > 0x7fffffffll || lags > frames) return AVA_EINVAL;
  if (ws == nullptr || ws_bytes < ava_tpl_workspace_bytes(lags)) return AVA_EINVAL;
  TplXcorrArgs a;
  a.spec = spec;
  a.frame_sum = frame_sum;
  a.frame_off = reinterpret_cast<const long long*>(frame_off);
  a.lag_off = reinterpret_cast<const long long*>(lag_off);
  a.tile_off = reinterpret_cast<const long long*>(tile_off);
  a.tmpl = tmpl;
  char* base = reinterpret_cast<char*>(ws);
  base += (256 - (reinterpret_cast<uintptr_t>(base) & 255)) & 255;
  a.mu = reinterpret_cast<double*>(base);
  a.trace = trace;
  a.frames = frames; a.lags = lags; a.files = files; a.F = F; a.L = L;
  hipStream_t st = to_stream(s);
  hipLaunchKernelGGL(tpl_mean_kernel, dim3((unsigned)ceil_div64(lags, AVA_TPL_T)), dim3(AVA_TPL_T), 0, st, a);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(tpl_xcorr_kernel, dim3((unsigned)tiles), dim3(AVA_TPL_XT), 0, st, a);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
