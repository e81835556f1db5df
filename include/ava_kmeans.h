/* The k-means part of the C ABI of libava_hip.so (row f25; csrc/kmeans.hip).  Included by ava_hip.h, which declares
 * ava_stream_t and the AVA_* return codes; mirrored one to one by ava_amd/_lib.py (KM_SIGNATURES).
 *
 * ---- Lloyd k-means with k-means++ seeding (scikit-learn 1.7 cluster/_kmeans.py: _kmeans_plusplus, _tolerance,
 * _kmeans_single_lloyd; _k_means_common.pyx: _relocate_empty_clusters_dense, _inertia_dense) -------------------------------
 * x [n][d] (dtype 0 = float32, 1 = float64; device) is converted on load; everything else is fp64.  Every (row, centre)
 * and (row, row) distance has the bits ava_pair_sqdist gives the pair.  Nothing uses floating-point atomics: every sum
 * over rows is taken inside chunks of ava_km_chunk_rows() = 2048 rows in ascending row order and the chunk partials are
 * added in ascending chunk order, so the same inputs give the same bits on every run, for float32 and float64 copies of
 * the same values.  1 <= n <= 2^31 - 64, 1 <= d <= ava_km_max_d() = 128, 1 <= k <= ava_km_max_k() = 256; a fit also
 * needs k <= n.  Nothing allocates or synchronises; every pointer is a device pointer.
 * ws: ava_km_workspace_bytes(n, d, k) bytes (0 for an unsupported shape); ava_km_pp_step and ava_km_variance accept the
 *   size for k = 1.
 *
 * ava_km_assign: labels [n] int = the nearest of the centres [k][d] of every row, the lowest index on a tie; d2 [n] the
 *   squared distance to it; inertia [1] (may be null) = sum d2 in the chunk order.
 * ava_km_update: one M-step from labels [n] int (a label outside [0, k) is in no cluster): counts [k] int64 and
 *   centres [k][d] = the sum of the rows of the cluster in the chunk order / its count, zeros for an empty cluster.
 * ava_km_fit: iterations [it0, it0 + n_iters) of sklearn's Lloyd loop on centres [k][d] (in and out): assign, new centres
 *   (an empty cluster takes the row farthest from its own centre; several empty clusters in ascending id take the rows in
 *   the order (d2 descending, row ascending); the row leaves its old cluster's sum and count), shift = sum_k |c_new -
 *   c_old|^2; the loop stops when no label changed (strict), else when shift <= tol * mean_var[0].  labels [n] int must
 *   hold -1 before iteration 0; labels and d2 [n] are those of the last assignment that ran, made at the centres BEFORE
 *   that iteration's update.  ctl [>= 3 + it0 + n_iters] int, zeroed before iteration 0: ctl[0] = 1 after a strict stop,
 *   ctl[1] the number of iterations that ran, ctl[2 + it] whether the loop had stopped before iteration it: the launches
 *   of a stopped iteration return at once, so iterations are enqueued in blocks between reads of ctl.  shift [1] (may be
 *   null): the shift of the last iteration that ran.  mean_var [1]: ava_km_variance's out[0].
 * ava_km_pp_start: closest [n] = the squared distance of every row to row `first` (sklearn's first centre).
 * ava_km_pp_step: one further centre of sklearn's _kmeans_plusplus.  rand [n_trials] are the caller's uniform draws,
 *   1 <= n_trials <= 8.  The candidates are searchsorted(scan, rand * potential) clipped to n - 1, scan the inclusive
 *   sums of closest (sequential inside the chunks, the ascending chunk offsets added), potential its last entry; the
 *   candidate whose min(closest, d2(candidate, .)) has the least sum (chunk order; the first on a tie) is written to
 *   out_idx [1] int, its sum to out_pot [1], and closest becomes that minimum.
 * ava_km_variance: out [1 + d]: out[1 + j] = mean_n (x_nj - mean_j)^2 with both means in the chunk order, out[0] their
 *   ascending sum / d (np.mean(np.var(x, axis=0)), the factor of sklearn's _tolerance).
 * ava_km_transform: out [n][k] = the euclidean distance of every row to every centre (the square root of the tile).
 *
 * All return AVA_EINVAL before any launch for null pointers, an unknown dtype or an unsupported shape, AVA_EWORKSPACE
 * for a workspace that is too small. */
#ifndef AVA_KMEANS_H
#define AVA_KMEANS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int ava_km_max_d(void);
int ava_km_max_k(void);
int ava_km_chunk_rows(void);
size_t ava_km_workspace_bytes(int n, int d, int k);
int ava_km_assign(const void* x, int dtype, int n, int d, int k, const double* centres, int* labels, double* d2,
                  double* inertia, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_km_update(const void* x, int dtype, int n, int d, int k, const int* labels, double* centres, int64_t* counts,
                  void* ws, size_t ws_bytes, ava_stream_t s);
int ava_km_fit(const void* x, int dtype, int n, int d, int k, double* centres, int* labels, double* d2, double tol,
               const double* mean_var, int it0, int n_iters, int* ctl, double* shift, void* ws, size_t ws_bytes,
               ava_stream_t s);
int ava_km_pp_start(const void* x, int dtype, int n, int d, int first, double* closest, ava_stream_t s);
int ava_km_pp_step(const void* x, int dtype, int n, int d, int n_trials, const double* rand, double* closest, int* out_idx,
                   double* out_pot, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_km_variance(const void* x, int dtype, int n, int d, double* out, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_km_transform(const void* x, int dtype, int n, int d, int k, const double* centres, double* out, ava_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* AVA_KMEANS_H */
