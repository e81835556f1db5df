// Cross-validated k-nearest-neighbour prediction from latent rows (the specification is
// scikit-learn 1.7's neighbors/_classification.py, _regression.py and _base.py::_get_weights under
// cross_val_predict with a PredefinedSplit).  All arithmetic is fp64; no kernel uses atomics and every sum runs in one
// fixed order, so every result is bit-reproducible and independent of the launch shape.
//
// masked kNN  the k nearest rows of every row among the rows of OTHER folds: pj_knn_kernel's walk (64 queries per
//             workgroup, the fp64 direct-difference tile of sqdist_tile.h, one folding thread per query, the lists of
//             knn_list.h in dynamic LDS) with the candidates of every query, the tile's references of other folds, staged
//             in LDS as a 64-bit mask.  A reference tile whose rows all share the one fold of all the workgroup's queries
//             holds no candidate and is skipped before anything is staged.  The order contract of sqdist_tile.h gives
//             every pair the bits it has in pj_knn_kernel, and the strict (distance, index) order makes the list for
//             k' < k a prefix of the list for k: one pass at the largest k serves every fold and every k of a sweep.
// vote        one wavefront per query row; lane s holds the class and the weight of list slot s.  A running sum over the
//             slots in ascending order gives every lane the score of its own class at every k of the sweep (lanes of one
//             class hold the same bits), and a butterfly takes the arg-max by (score descending, class ascending).
// proba       the class scores of one k, summed in slot order and divided by the sum of the weights (0 counts as 1).
// regress     one thread per (query, output) walks the list once and writes num / den at every k of the sweep.
// Weights: 1, or 1 / distance, except in a row whose slot 0 is at distance 0, where they are (distance == 0).
#include <limits.h>

#include "common.h"
#include "knn_list.h"
#include "sqdist_tile.h"

#define KP_MAX_SWEEP 16
#define KP_MAX_CLASSES 4096
#define KP_MAX_OUT 256

// rows [q0, q0 + nq) of the table: the k nearest of the n rows X to query row q among the rows r with
// fold[r] != fold[q], ordered by (distance, index).
// Folds: lane l of every wave holds the fold of query qb + l and of the tile's reference r0 + l in registers (the next
// tile's are in flight while this one is formed), so every wave decides the skip alone and alike.  For a tile that is
// not skipped wave w turns the folds into the candidate masks of its queries 16 w .. 16 w + 15 (bit c: reference
// r0 + c exists and is of another fold; one ballot per query) and stages them in LDS after sqd_tile's opening barrier
// (every thread is past the fold before) and before the two barriers that precede the fold, which walks the runs of
// set bits: no barrier beyond pj_knn_kernel's.
// LDS: 33 792 B static for the staging buffers / the 64 x 64 distance tile, 512 B of candidate masks and 768 k B of
// dynamic lists: 83 456 B at k = 64, of the 160 KiB a workgroup may use.
template <typename T>
__global__ __launch_bounds__(256) void kp_knn_masked_kernel(const T* __restrict__ X, const int* __restrict__ fold,
                                                            int n, int d, int k, int q0, int nq,
                                                            int64_t* __restrict__ out_idx,
                                                            double* __restrict__ out_dist) {
  __shared__ double stage[2 * SQD_T * SQD_LD];      // xs | ys while staging, then the 64 x 64 distance tile
  __shared__ uint64_t cand[SQD_T];                  // candidate mask of every query for the tile at hand
  extern __shared__ double lists[];                 // k x 64 distances, then k x 64 int indices
  double* xs = stage;
  double* ys = stage + SQD_T * SQD_LD;
  double* dt = stage;
  double* ld = lists;
  int* li = reinterpret_cast<int*>(lists + (size_t)k * SQD_T);
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15, lane = t & 63, w = t >> 6;
  const int qb = q0 + blockIdx.x * SQD_T;            // first query row of this workgroup: qb < qe
  const int qe = q0 + nq;
  for (int s = t; s < k * SQD_T; s += 256) {
    ld[s] = 0.0;
    li[s] = -1;
  }
  // rows that do not exist carry the fold of query qb: they can never keep a tile from being skipped
  const int f0 = fold[qb];
  const int fq = qb + lane < qe ? fold[qb + lane] : f0;
  const bool one_fold = __all(fq == f0);             // all this workgroup's queries are of fold f0
  int fr_next = lane < n ? fold[lane] : f0;
  for (int r0 = 0; r0 < n; r0 += SQD_T) {
    const int fr = fr_next;
    fr_next = r0 + SQD_T + lane < n ? fold[r0 + SQD_T + lane] : f0;
    // the same registers in every wave: the branch is uniform over the workgroup, and no LDS is touched before it
    if (one_fold && __all(fr == f0)) continue;
    double acc[4][4];
    sqd_tile(xs, ys, X, qb, qe, X, r0, n, d, t, acc);  // opens with a barrier: the tile before is folded, cand is free
    uint64_t mine = 0;
    for (int j = 0; j < SQD_T / 4; ++j) {
      const int fj = __shfl(fq, 16 * w + j, 64);      // by every lane: a shuffle reads active lanes only
      const uint64_t m = __ballot(r0 + lane < n && fr != fj);
      if (lane == j) mine = m;
    }
    if (lane < SQD_T / 4) cand[16 * w + lane] = mine;
    __syncthreads();                                 // staging reads done: the tile reuses the buffer
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dt[(ty + 16 * i) * PJ_DLD + tx + 16 * j] = sqrt(acc[i][j]);
    __syncthreads();
    if (t < SQD_T && qb + t < qe) {
      // the candidates are the maximal runs of references of other folds, each folded in reference order
      uint64_t m = cand[t];
      while (m != 0) {
        const int c = __builtin_ctzll(m);
        const uint64_t rest = ~(m >> c);             // its lowest set bit ends the run that starts at c
        const int len = rest != 0 ? __builtin_ctzll(rest) : SQD_T;
        pj_fold_tile(dt + t * PJ_DLD + c, r0 + c, len, qb + t, 0, k, ld, li, t);
        m = c + len < SQD_T ? m & (~(uint64_t)0 << (c + len)) : 0;
      }
    }
  }
  __syncthreads();
  if (t < SQD_T && qb + t < qe) pj_write_list((size_t)(qb + t - q0), qb + t, k, 0, ld, li, t, out_idx, out_dist);
}

// sklearn's _get_weights for slot distance dd of a row whose slot 0 is at d0 (the list is sorted: a row has a zero
// distance exactly when slot 0 has)
__device__ __forceinline__ double kp_weight(double dd, double d0, int weighted) {
  if (!weighted) return 1.0;
  if (d0 == 0.0) return dd == 0.0 ? 1.0 : 0.0;
  return 1.0 / dd;
}

// out[a][q] = the class of query q at the a-th k of the sweep; bit k - 1 of sweep is set for every k of it.  One
// wavefront per query: after slot s the running sum of lane l <= s is the score of lane l's class over slots 0 .. s,
// plain adds from 0.0 in slot order.
__global__ __launch_bounds__(256) void kp_vote_kernel(const int64_t* __restrict__ idx, const double* __restrict__ dist,
                                                      int nq, int kmax, const int* __restrict__ y, uint64_t sweep,
                                                      int kend, int weighted, int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;                               // a whole wavefront
  const size_t o = (size_t)q * kmax;
  const double d0 = dist[o];
  int label = INT_MAX;
  double w = 0.0;
  if (lane < kend && idx[o + lane] >= 0) {           // an empty slot (the table's caller rules it out) has no vote
    label = y[idx[o + lane]];
    w = kp_weight(dist[o + lane], d0, weighted);
  }
  double score = 0.0;
  int a = 0;
  for (int s = 0; s < kend; ++s) {
    const int ls = __shfl(label, s, 64);
    const double ws = __shfl(w, s, 64);
    if (ls == label) score += ws;
    if ((sweep >> s) & 1) {
      double bs = lane <= s ? score : -1.0;          // scores are >= 0
      int bl = lane <= s ? label : INT_MAX;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(bs, off, 64);
        const int ol = __shfl_xor(bl, off, 64);
        if (os > bs || (os == bs && ol < bl)) {
          bs = os;
          bl = ol;
        }
      }
      if (lane == 0) out[(size_t)a * nq + q] = bl;
      ++a;
    }
  }
}

// out[q][c] = the share of class c in the weights of the k slots of query q (a [nq][k] table): one workgroup per query,
// the scores in LDS, one thread adding them in slot order
__global__ __launch_bounds__(256) void kp_proba_kernel(const int64_t* __restrict__ idx, const double* __restrict__ dist,
                                                       int k, const int* __restrict__ y, int n_classes, int weighted,
                                                       double* __restrict__ out) {
  extern __shared__ double score[];                  // n_classes
  __shared__ double total;
  const int t = threadIdx.x;
  const size_t o = (size_t)blockIdx.x * k;
  for (int c = t; c < n_classes; c += 256) score[c] = 0.0;
  __syncthreads();
  if (t == 0) {
    const double d0 = dist[o];
    double sum = 0.0;
    for (int s = 0; s < k; ++s) {
      const double w = kp_weight(dist[o + s], d0, weighted);
      const int c = idx[o + s] >= 0 ? y[idx[o + s]] : -1;
      if (c >= 0 && c < n_classes) score[c] += w;
      sum += w;
    }
    total = sum == 0.0 ? 1.0 : sum;
  }
  __syncthreads();
  for (int c = t; c < n_classes; c += 256) out[(size_t)blockIdx.x * n_classes + c] = score[c] / total;
}

// out[a][q][t] = num / den of output t of query q at the a-th k of the sweep (bits of sweep as in kp_vote_kernel)
__global__ __launch_bounds__(256) void kp_regress_kernel(const int64_t* __restrict__ idx,
                                                         const double* __restrict__ dist, int nq, int kmax,
                                                         const double* __restrict__ Y, int n_out, uint64_t sweep,
                                                         int kend, int weighted, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)nq * n_out) return;
  const int64_t q = e / n_out;
  const int t = (int)(e % n_out);
  const size_t o = (size_t)q * kmax;
  const double d0 = dist[o];
  double num = 0.0, den = 0.0;
  int a = 0;
  for (int s = 0; s < kend; ++s) {
    if (idx[o + s] >= 0) {                           // an empty slot (the table's caller rules it out) counts for nothing
      const double w = kp_weight(dist[o + s], d0, weighted);
      num = fma(w, Y[(size_t)idx[o + s] * n_out + t], num);
      den += w;
    }
    if ((sweep >> s) & 1) {
      out[((size_t)a * nq + q) * n_out + t] = num / den;
      ++a;
    }
  }
}

extern "C" int ava_kp_knn_masked(const void* x, int dtype, int n, int d, int k, const int* fold, int q0, int nq,
                                 int64_t* out_idx, double* out_dist, ava_stream_t s) {
  if (x == nullptr || fold == nullptr || out_idx == nullptr || out_dist == nullptr || (dtype != 0 && dtype != 1) ||
      n < 1 || n > (1 << 30) || d < 1 || d > 65536 || k < 1 || k > PJ_MAX_K || k > n || q0 < 0 || nq < 1 ||
      (int64_t)q0 + nq > n)
    return AVA_EINVAL;
  const size_t lds = (size_t)k * SQD_T * (sizeof(double) + sizeof(int));
  if (dtype == 0)
    hipLaunchKernelGGL(kp_knn_masked_kernel<float>, dim3(ceil_div(nq, SQD_T)), dim3(256), lds, to_stream(s),
                       reinterpret_cast<const float*>(x), fold, n, d, k, q0, nq, out_idx, out_dist);
  else
    hipLaunchKernelGGL(kp_knn_masked_kernel<double>, dim3(ceil_div(nq, SQD_T)), dim3(256), lds, to_stream(s),
                       reinterpret_cast<const double*>(x), fold, n, d, k, q0, nq, out_idx, out_dist);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// the sweep as a bit set; false unless 1 <= ks[0] < ks[1] < .. <= kmax
static bool kp_sweep_bits(const int* ks, int n_k, int kmax, uint64_t* bits) {
  if (ks == nullptr || n_k < 1 || n_k > KP_MAX_SWEEP || kmax < 1 || kmax > PJ_MAX_K) return false;
  *bits = 0;
  for (int a = 0; a < n_k; ++a) {
    if (ks[a] < 1 || ks[a] > kmax || (a > 0 && ks[a] <= ks[a - 1])) return false;
    *bits |= (uint64_t)1 << (ks[a] - 1);
  }
  return true;
}

extern "C" int ava_kp_max_sweep(void) { return KP_MAX_SWEEP; }
extern "C" int ava_kp_max_classes(void) { return KP_MAX_CLASSES; }
extern "C" int ava_kp_max_outputs(void) { return KP_MAX_OUT; }

extern "C" int ava_kp_vote(const int64_t* idx, const double* dist, int nq, int kmax, const int* y, const int* ks,
                           int n_k, int weighted, int* out_pred, ava_stream_t s) {
  uint64_t bits;
  if (idx == nullptr || dist == nullptr || y == nullptr || out_pred == nullptr || nq < 1 ||
      (weighted != 0 && weighted != 1) || !kp_sweep_bits(ks, n_k, kmax, &bits))
    return AVA_EINVAL;
  hipLaunchKernelGGL(kp_vote_kernel, dim3(ceil_div(nq, 4)), dim3(256), 0, to_stream(s), idx, dist, nq, kmax, y, bits,
                     ks[n_k - 1], weighted, out_pred);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_kp_proba(const int64_t* idx, const double* dist, int nq, int k, const int* y, int n_classes,
                            int weighted, double* out, ava_stream_t s) {
  if (idx == nullptr || dist == nullptr || y == nullptr || out == nullptr || nq < 1 || k < 1 || k > PJ_MAX_K ||
      n_classes < 1 || n_classes > KP_MAX_CLASSES || (weighted != 0 && weighted != 1))
    return AVA_EINVAL;
  hipLaunchKernelGGL(kp_proba_kernel, dim3(nq), dim3(256), (size_t)n_classes * sizeof(double), to_stream(s), idx, dist,
                     k, y, n_classes, weighted, out);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

extern "C" int ava_kp_regress(const int64_t* idx, const double* dist, int nq, int kmax, const double* Y, int n_out,
                              const int* ks, int n_k, int weighted, double* out, ava_stream_t s) {
  uint64_t bits;
  if (idx == nullptr || dist == nullptr || Y == nullptr || out == nullptr || nq < 1 || n_out < 1 ||
      n_out > KP_MAX_OUT || (weighted != 0 && weighted != 1) || !kp_sweep_bits(ks, n_k, kmax, &bits))
    return AVA_EINVAL;
  const int64_t blocks = ceil_div64((int64_t)nq * n_out, 256);
  if (blocks > INT_MAX) return AVA_EINVAL;
  hipLaunchKernelGGL(kp_regress_kernel, dim3((unsigned)blocks), dim3(256), 0, to_stream(s), idx, dist, nq, kmax, Y,
                     n_out, bits, ks[n_k - 1], weighted, out);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
