// Template segmentation on the device: the arithmetic core of
// ava/segmenting/template_segmentation.py:_segment_file for every recording of a DeviceAudio at once.
//
//   _get_spec (lines 758-790, = segmenting/utils.py:get_spec): the band spectrogram of the whole file and the sum of
//   every frame over the band: the amplitude segmentation's band stage in sum mode (ava_tpl_spec, segment.hip)
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
#define AVA_TPL_T 256            // threads of the mean kernel

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
  a.mu = reinterpret_cast<double*>(ava_align256(ws));
  a.trace = trace;
  a.frames = frames; a.lags = lags; a.files = files; a.F = F; a.L = L;
  hipStream_t st = to_stream(s);
  hipLaunchKernelGGL(tpl_mean_kernel, dim3((unsigned)ceil_div64(lags, AVA_TPL_T)), dim3(AVA_TPL_T), 0, st, a);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(tpl_xcorr_kernel, dim3((unsigned)tiles), dim3(AVA_TPL_XT), 0, st, a);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
