// Permutation test for MMD^2: the null distribution of the reference's unbiased
// estimator (`_estimate_mmd2`, ava/plotting/mmd_plots.py:255-296; Gretton et al. 2012, section 5) under random
// re-splits of the pooled sample, and the count behind the p-value.  The reference has no such test; the model is
// DESIGN.md section 1 row f18, the statistic of a split is the reference's term_1 + term_2 - term_3 (:277-295).
//
// A problem is one pair of index lists (n1 and n2 rows of latent); its pool is their concatenation, positions
// j = 0 .. n - 1.  Split 0 is the caller's own (positions 0 .. n1 - 1 are set 1); in split p >= 1 set 1 is the n1
// positions with the smallest (key, j), key = ava_mix64(j, salt), salt = ((seed + pair) mod 2^32) 2^32 + p.
//
// Three kernels per chunk [p0, p1) of splits, all problems of a table at once:
//   membership  a workgroup per (problem, split): the n1-th smallest key by an 8-pass radix select (256-bin LDS
//               histograms over keys recomputed in every pass: no key array in memory), then one byte per position,
//               1 = set 1.  Ties in the key would go to the smaller j (the hash is a bijection of j, so there are none).
//   statistic   with K0 the pool's kernel matrix exp(A d^2), diagonal zeroed, and S the n x columns 0/1 matrix of the
//               chunk, a workgroup owns (problem, 64 pool rows, 64 columns) and walks the pool's 64-row column tiles:
//               the tile of K0 from sqd_stage_rows / sqd_accumulate (the bits of mmd_tile_sum's distances), through
//               LDS into the fragment layout of corr_mfma_stage as the A operand, the bytes as 0.0 / 1.0 as the B
//               operand: Y = K0 S for its rows on the fp64 matrix cores.  K0 is never stored.  From Y, per column,
//               a = sum_{i in S} Y_i (twice the within-set sum of the marked set) and cross = sum_{i not in S} Y_i:
//               both direct sums of positive values.
//   finalize    fixed-order sums of a and cross over the row tiles, the three terms, the statistic; then the count
//               #{p >= 1 : stat_p >= stat_0}.
// The pool total T = sum K0 is column 0 of every chunk, an all-ones column (its a).  The within-set sum of the
// unmarked set is (T - a - 2 cross) / 2, which cancels when that set is the small one.  So the columns of S mark the
// SMALLER of the two sets (the membership byte, flipped when n1 > n2) and the finalize kernel swaps the roles back.
//
// Order contract: a column's Y_i takes its k in one ascending walk of 4-wide MFMA steps from pool position 0; a and
// cross sum a thread's rows ascending, then the four row groups of a wave as (g0 + g1) + (g2 + g3), then the waves as
// (w0 + w1) + (w2 + w3), then the row tiles ascending.  None of this looks at the column's place.  So a column's values
// depend on the latent rows, sigma and its membership vector only -- never on its place in a tile, on the chunk it
// fell in or on the other columns -- and two runs give the same bits.
//
// Caps: pool n1 + n2 <= 2^24 rows, 2^23 problems, p1 <= 2^31 - 1, 2^20 splits per chunk, problems x splits of a chunk
// <= 2^31 - 1 (the finalize launch has a thread for each).
#include "common.h"
#include "sqdist_tile.h"
#include "corr_tile.h"

#define MP_T SQD_T              // pool rows of a tile, and the k of one step of the product
#define MP_COLS 64              // columns (splits) of a workgroup of the statistic kernel
#define MP_ROW 8                // int64 of a table row: {o1, o2, n1, n2, pair, first position, first row tile, 0}
#define MP_CHUNK (1 << 20)      // workgroups per launch
#define MP_MAX_N (1 << 24)
#define MP_MAX_PROBLEMS (1 << 23)
#define MP_MAX_CHUNK_COLS (1 << 20)
#define MP_PANEL (MP_T * CORR_LD)                         // doubles of one 16-wide k panel of 64 rows
#define MP_LDS_BYTES (2 * (MP_T / CORR_KC) * MP_PANEL * sizeof(double))

static_assert(MP_T == 64 && MP_COLS == 64 && CORR_KC == 16, "the thread maps below are written for these");
static_assert(2 * SQD_T * SQD_LD <= (MP_T / CORR_KC) * MP_PANEL, "the distance stages alias the K0 panels");

__global__ __launch_bounds__(256) void mmd_perm_member_kernel(const int64_t* __restrict__ table, int cols, int64_t p0,
                                                              uint64_t seed, int64_t n_total, int64_t g0,
                                                              uint8_t* __restrict__ mem) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t sel[3];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t g = g0 + blockIdx.x;
  const int64_t prob = g / cols;
  const int q = (int)(g - prob * cols);
  const int64_t* row = table + (size_t)prob * MP_ROW;
  const int n1 = (int)row[2], n = n1 + (int)row[3];
  const uint64_t p = (uint64_t)(p0 + q);
  uint8_t* out = mem + (size_t)q * n_total + row[5];
  if (p == 0) {                          // the caller's own split
    for (int j = t; j < n; j += 256) out[j] = j < n1;
    return;
  }
  const uint64_t salt = (((seed + (uint64_t)row[4]) & 0xffffffffull) << 32) + p;
  uint64_t prefix = 0;                   // the leading bytes of the n1-th smallest key found so far
  uint32_t k = (uint32_t)n1;             // its rank (from 1) among the keys that share them
  uint32_t n_eq = 0;
  for (int b = 0; b < 8; ++b) {
    const int shift = 56 - 8 * b;
    hist[t] = 0;
    __syncthreads();
    for (int j = t; j < n; j += 256) {
      const uint64_t key = ava_mix64((uint64_t)j, salt);
      if (b == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    const uint32_t c = hist[t];
    uint32_t v = c;                      // inclusive scan over the 256 bins
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    for (int ww = 0; ww < w; ++ww) v += wsum[ww];
    if (v - c < k && k <= v) {           // the one bin the rank falls in
      sel[0] = (uint32_t)t;
      sel[1] = k - (v - c);
      sel[2] = c;
    }
    __syncthreads();
    prefix = (prefix << 8) | sel[0];
    k = sel[1];
    n_eq = sel[2];
    __syncthreads();
  }
  // set 1: the keys below the n1-th smallest, and of the n_eq positions that hold it the k with the smallest j
  for (int j = t; j < n; j += 256) {
    const uint64_t key = ava_mix64((uint64_t)j, salt);
    bool in = key < prefix;
    if (key == prefix) {
      in = true;
      if (k < n_eq) {
        uint32_t before = 0;
        for (int jj = 0; jj < j; ++jj) before += ava_mix64((uint64_t)jj, salt) == prefix;
        in = before < k;
      }
    }
    out[j] = in;
  }
}

// the table row whose row tiles include tile gt: column 6 is strictly increasing (every problem has a tile)
__device__ __forceinline__ int mp_find_problem(const int64_t* __restrict__ table, int n_problems, int64_t gt) {
  int lo = 0, hi = n_problems;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[(size_t)mid * MP_ROW + 6] <= gt) lo = mid; else hi = mid;
  }
  return lo;
}

// partials: [row tile of the whole table][cols + 1][2] = {a, cross}; column 0 is the all-ones column, column 1 + q
// split p0 + q.  ptiles = ceil((cols + 1) / 64).
__global__ __launch_bounds__(256) void mmd_perm_stat_kernel(const double* __restrict__ L, int z,
                                                            const int64_t* __restrict__ idx,
                                                            const int64_t* __restrict__ table, int n_problems, int cols,
                                                            int ptiles, int64_t n_total, double A, int64_t g0,
                                                            const uint8_t* __restrict__ mem,
                                                            double* __restrict__ partials) {
  extern __shared__ __align__(16) double sm[];
  __shared__ int64_t xrow[MP_T], yrow[MP_T];
  __shared__ double red[4][MP_COLS][2];
  double* ks = sm;                                   // [4][64][17]: K0 tile, panel s = columns 16 s .. 16 s + 15
  double* ss = sm + (MP_T / CORR_KC) * MP_PANEL;     // [4][64][17]: S tile, row = column of S, panel s likewise
  double* xs = sm;                                   // [64][33] and [64][33]: the distance stages, over ks
  double* ys = sm + SQD_T * SQD_LD;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int ty = t >> 4, tx = t & 15;
  const int64_t g = g0 + blockIdx.x;
  const int64_t gt = g / ptiles;
  const int pt = (int)(g - gt * ptiles);
  const int64_t* row = table + (size_t)mp_find_problem(table, n_problems, gt) * MP_ROW;
  const int64_t o1 = row[0], o2 = row[1];
  const int n1 = (int)row[2], n2 = (int)row[3], n = n1 + n2;
  const int rt = (int)(gt - row[6]);
  const int i0 = rt * MP_T;
  const uint8_t flip = n1 > n2;                      // the bytes mark set 1, the columns of S the smaller set
  const uint8_t* pm = mem + row[5];
  const int n_tiles = (n + MP_T - 1) / MP_T;
  if (t < MP_T) {
    const int gi = i0 + t;
    xrow[t] = gi < n ? (gi < n1 ? idx[o1 + gi] : idx[o2 + gi - n1]) : -1;
  }
  corr_d4 acc[1][4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[0][b] = (corr_d4){0.0, 0.0, 0.0, 0.0};

  for (int ct = 0; ct < n_tiles; ++ct) {
    const int j0 = ct * MP_T;
    __syncthreads();                                 // the MFMAs of the tile before have read ks and ss
    if (t < MP_T) {
      const int gj = j0 + t;
      yrow[t] = gj < n ? (gj < n1 ? idx[o1 + gj] : idx[o2 + gj - n1]) : -1;
    }
    {
      const int c = t >> 2, s = t & 3;               // column c of the tile, positions 16 s .. 16 s + 15
      const int ec = pt * MP_COLS + c;
      double* dst = ss + s * MP_PANEL + c * CORR_LD;
      const uint8_t* src = pm + (size_t)(ec > 0 ? ec - 1 : 0) * n_total;
#pragma unroll
      for (int kk = 0; kk < CORR_KC; ++kk) {
        const int pos = j0 + CORR_KC * s + kk;
        double v = 0.0;
        if (ec <= cols && pos < n) v = ec == 0 ? 1.0 : (double)(uint8_t)(src[pos] ^ flip);
        dst[kk] = v;
      }
    }
    double d2[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) d2[i][j] = 0.0;
    for (int k0 = 0; k0 < z; k0 += SQD_KC) {
      __syncthreads();                               // yrow is there; the stage before has been read
      sqd_stage_rows(xs, ys, L, xrow, yrow, z, k0, t);
      __syncthreads();
      sqd_accumulate(xs, ys, SQD_LD, z - k0 < SQD_KC ? z - k0 : SQD_KC, ty, tx, d2);
    }
    __syncthreads();                                 // xs / ys have been read: ks may overwrite them
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gi = i0 + ty + 16 * i, gj = j0 + tx + 16 * j;
        ks[j * MP_PANEL + (ty + 16 * i) * CORR_LD + tx] = (gi < n && gj < n && gi != gj) ? exp(A * d2[i][j]) : 0.0;
      }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < MP_T / CORR_KC; ++s)
      corr_mfma_stage<1, 4>(ks + s * MP_PANEL, ss + s * MP_PANEL, 16 * w, 0, lane, acc);
  }

  // acc[0][b][reg] = Y[row 16 w + (lane >> 4) + 4 reg][column 16 b + (lane & 15)]
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int ec = pt * MP_COLS + 16 * b + (lane & 15);
    const uint8_t* src = pm + (size_t)(ec > 0 ? ec - 1 : 0) * n_total;
    double sa = 0.0, sc = 0.0;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int gi = i0 + 16 * w + (lane >> 4) + 4 * reg;
      if (ec <= cols && gi < n) {
        const bool in = ec == 0 || (uint8_t)(src[gi] ^ flip) != 0;
        if (in) sa += acc[0][b][reg]; else sc += acc[0][b][reg];
      }
    }
    sa += __shfl_xor(sa, 16, 64);
    sc += __shfl_xor(sc, 16, 64);
    sa += __shfl_xor(sa, 32, 64);
    sc += __shfl_xor(sc, 32, 64);
    if (lane < 16) {
      red[w][16 * b + lane][0] = sa;
      red[w][16 * b + lane][1] = sc;
    }
  }
  __syncthreads();
  if (t < MP_COLS) {
    const int ec = pt * MP_COLS + t;
    if (ec <= cols) {
      double* dst = partials + ((size_t)gt * (cols + 1) + ec) * 2;
      dst[0] = (red[0][t][0] + red[1][t][0]) + (red[2][t][0] + red[3][t][0]);
      dst[1] = (red[0][t][1] + red[1][t][1]) + (red[2][t][1] + red[3][t][1]);
    }
  }
}

// one thread per (problem, split of the chunk): terms [problems][cols][3] = the reference's term_1, term_2, term_3 of the
// split, stats [problems][cols] = term_1 + term_2 - term_3.  With m the marked (smaller) set and M the other one:
// a / 2 and (T - a - 2 cross) / 2 are their sums over i < j, cross the sum over the pairs between them.
__global__ __launch_bounds__(256) void mmd_perm_finalize_kernel(const double* __restrict__ partials,
                                                                const int64_t* __restrict__ table, int cols,
                                                                int64_t n_items, double* __restrict__ terms,
                                                                double* __restrict__ stats) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_items) return;
  const int64_t prob = e / cols;
  const int q = (int)(e - prob * cols);
  const int64_t* row = table + (size_t)prob * MP_ROW;
  const int n1 = (int)row[2], n2 = (int)row[3];
  const int64_t tiles = row[MP_ROW + 6] - row[6];
  const double* base = partials + (size_t)row[6] * (cols + 1) * 2;
  double tot = 0.0, a = 0.0, c = 0.0;
  for (int64_t r = 0; r < tiles; ++r) {
    const double* pr = base + (size_t)r * (cols + 1) * 2;
    tot += pr[0];
    a += pr[2 * (q + 1)];
    c += pr[2 * (q + 1) + 1];
  }
  const double m = n1 <= n2 ? n1 : n2, M = n1 <= n2 ? n2 : n1;
  const double rest = (tot - a) - 2.0 * c;
  const double tm = (0.5 * a) * (2.0 / (m * (m - 1.0)));
  const double tM = (0.5 * rest) * (2.0 / (M * (M - 1.0)));
  const double t3 = c * (2.0 / ((double)n1 * n2));
  const double t1 = n1 <= n2 ? tm : tM, t2 = n1 <= n2 ? tM : tm;
  terms[e * 3 + 0] = t1;
  terms[e * 3 + 1] = t2;
  terms[e * 3 + 2] = t3;
  stats[e] = t1 + t2 - t3;
}

// one workgroup per problem: counts[problem] (+)= #{q : p0 + q >= 1, stats[q] >= stat_0}.  The chunk that starts at
// p0 = 0 holds stat_0 (split 0), stores it in stat0[problem] for the later chunks and starts the count.
__global__ __launch_bounds__(256) void mmd_perm_count_kernel(const double* __restrict__ stats, int cols, int64_t p0,
                                                             double* __restrict__ stat0, int64_t* __restrict__ counts) {
  __shared__ int red[4];
  const int t = threadIdx.x;
  const double* s = stats + (size_t)blockIdx.x * cols;
  const double s0 = p0 == 0 ? s[0] : stat0[blockIdx.x];
  int c = 0;
  for (int q = t; q < cols; q += 256) c += (p0 + q >= 1) && (s[q] >= s0);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((t & 63) == 0) red[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    const int64_t total = (red[0] + red[1]) + (red[2] + red[3]);
    if (p0 == 0) {
      stat0[blockIdx.x] = s0;
      counts[blockIdx.x] = total;
    } else {
      counts[blockIdx.x] += total;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// walks the n_problems + 1 HOST rows; n_idx < 0: the index list's length is not known (sizing only)
static bool mp_table_ok(const int64_t* table, int n_problems, int64_t n_idx, int64_t* n_total, int64_t* n_tiles) {
  if (table == nullptr || n_problems < 1 || n_problems > MP_MAX_PROBLEMS) return false;
  int64_t pos = 0, tiles = 0;
  for (int i = 0; i <= n_problems; ++i) {
    const int64_t* row = table + (size_t)i * MP_ROW;
    if (row[5] != pos || row[6] != tiles) return false;
    if (i == n_problems) break;
    const int64_t o1 = row[0], o2 = row[1], n1 = row[2], n2 = row[3];
    if (n1 < 2 || n2 < 2 || n1 + n2 > MP_MAX_N || o1 < 0 || o2 < 0 || row[4] < 0) return false;
    if (n_idx >= 0 && (o1 + n1 > n_idx || o2 + n2 > n_idx)) return false;
    pos += n1 + n2;
    tiles += (n1 + n2 + MP_T - 1) / MP_T;
  }
  *n_total = pos;
  *n_tiles = tiles;
  return true;
}

static bool mp_range_ok(int64_t p0, int64_t p1, int n_problems) {
  return p0 >= 0 && p1 > p0 && p1 <= 0x7fffffff && p1 - p0 <= MP_MAX_CHUNK_COLS &&
         (p1 - p0) * (int64_t)n_problems <= 0x7fffffff;
}

extern "C" int ava_mmd2_perm_tile(void) { return MP_COLS; }

extern "C" size_t ava_mmd2_perm_workspace_bytes(const int64_t* table, int n_problems, int n_splits) {
  int64_t n_total, n_tiles;
  if (!mp_range_ok(0, n_splits, n_problems) || !mp_table_ok(table, n_problems, -1, &n_total, &n_tiles)) return 0;
  return (size_t)n_tiles * (size_t)(n_splits + 1) * 2 * sizeof(double) + 256;
}

static int mp_launch_membership(const int64_t* table_dev, int n_problems, int64_t p0, int cols, uint64_t seed,
                                int64_t n_total, uint8_t* membership, hipStream_t st) {
  const int64_t total = (int64_t)n_problems * cols;
  for (int64_t g0 = 0; g0 < total; g0 += MP_CHUNK) {
    const int64_t left = total - g0;
    const int grid = (int)(left < MP_CHUNK ? left : MP_CHUNK);
    hipLaunchKernelGGL(mmd_perm_member_kernel, dim3(grid), dim3(256), 0, st, table_dev, cols, p0, seed, n_total, g0,
                       membership);
    AVA_CHECK_LAUNCH();
  }
  return AVA_OK;
}

extern "C" int ava_mmd2_perm_membership(const int64_t* table, const int64_t* table_dev, int n_problems, int64_t p0,
                                        int64_t p1, uint64_t seed, uint8_t* membership, ava_stream_t s) {
  int64_t n_total, n_tiles;
  if (table_dev == nullptr || membership == nullptr || !mp_range_ok(p0, p1, n_problems) ||
      !mp_table_ok(table, n_problems, -1, &n_total, &n_tiles))
    return AVA_EINVAL;
  return mp_launch_membership(table_dev, n_problems, p0, (int)(p1 - p0), seed, n_total, membership, to_stream(s));
}

extern "C" int ava_mmd2_perm(const double* latent, int z, const int64_t* idx, int64_t n_idx, const int64_t* table,
                             const int64_t* table_dev, int n_problems, int64_t p0, int64_t p1, uint64_t seed,
                             double sigma, uint8_t* membership, double* terms, double* stats, double* stat0,
                             int64_t* counts, void* ws, size_t ws_bytes, ava_stream_t s) {
  int64_t n_total, n_tiles;
  if (latent == nullptr || idx == nullptr || table_dev == nullptr || membership == nullptr || terms == nullptr ||
      stats == nullptr || stat0 == nullptr || counts == nullptr || ws == nullptr || z < 1 || z > 128 || n_idx < 0 ||
      !(sigma > 0.0) || !mp_range_ok(p0, p1, n_problems) || !mp_table_ok(table, n_problems, n_idx, &n_total, &n_tiles))
    return AVA_EINVAL;
  const int cols = (int)(p1 - p0);
  if (ws_bytes < (size_t)n_tiles * (size_t)(cols + 1) * 2 * sizeof(double) + 256) return AVA_EWORKSPACE;
  hipStream_t st = to_stream(s);
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&mmd_perm_stat_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)MP_LDS_BYTES) != hipSuccess)
      return AVA_ELAUNCH;
    attr = true;
  }
  int rc = mp_launch_membership(table_dev, n_problems, p0, cols, seed, n_total, membership, st);
  if (rc != AVA_OK) return rc;
  double* partials = reinterpret_cast<double*>(ava_align256(ws));
  const double A = -0.5 / (sigma * sigma);
  const int ptiles = (cols + 1 + MP_COLS - 1) / MP_COLS;
  const int64_t total = n_tiles * ptiles;
  for (int64_t g0 = 0; g0 < total; g0 += MP_CHUNK) {
    const int64_t left = total - g0;
    const int grid = (int)(left < MP_CHUNK ? left : MP_CHUNK);
    hipLaunchKernelGGL(mmd_perm_stat_kernel, dim3(grid), dim3(256), MP_LDS_BYTES, st, latent, z, idx, table_dev,
                       n_problems, cols, ptiles, n_total, A, g0, membership, partials);
    AVA_CHECK_LAUNCH();
  }
  const int64_t n_items = (int64_t)n_problems * cols;            // <= 2^31 - 1: at most 2^23 workgroups
  hipLaunchKernelGGL(mmd_perm_finalize_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st, partials,
                     table_dev, cols, n_items, terms, stats);
  AVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(mmd_perm_count_kernel, dim3(n_problems), dim3(256), 0, st, stats, cols, p0, stat0, counts);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
