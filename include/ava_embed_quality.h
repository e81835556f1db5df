/* Trustworthiness, continuity and preserved neighbours of an embedding (row f26; csrc/embed_quality.hip).  Included by
 * ava_hip.h, inside its extern "C" block and after its typedefs; mirrored by _lib.EQ_SIGNATURES.
 *
 * n rows are given in two spaces, X [n][d] and Y [n][e], float32 (dtype 0) or float64 (dtype 1), read into fp64.  d2 is
 * the squared euclidean distance of csrc/sqdist_tile.h (direct differences, one fma per feature, features ascending),
 * and (d2(i, l), l) comes before (d2(i, j), j) when d2(i, l) < d2(i, j), or when they are equal and l < j: a strict total
 * order, so every count below is a function of the data alone.
 *   rank        r(i, j) = 1 + #{ l != i : (d2(i, l), l) before (d2(i, j), j) }, j != i: 1 .. n - 1
 *   penalty     P(k) = sum_i sum_{s < k} max(0, r_X(i, N^Y(i)[s]) - k), N^Y(i) row i's neighbours in Y in the order
 *               (the columns 1 .. of ava_pj_knn's table).  Trustworthiness is 1 - P(k) 2 / (n k (2 n - 3 k - 1)),
 *               continuity the same with the spaces exchanged.
 *   overlap     |N_k^X(i) and N_k^Y(i)|; its mean over rows, divided by k, is Q_NX(k).
 * All results are integers, summed as integers: they do not depend on the launch shape, and no kernel uses a
 * floating-point atomic.  ks [n_k] (host) is a sweep of k with 1 <= ks[a] <= m and n_k <= ava_eq_max_sweep() = 16, in
 * any order; one table at m = max(ks) serves all of it, since the list for k' < k is a prefix of the list for k.
 *
 * ava_eq_ranks: rank [n][m] int = r(i, tgt[i][s]) among the rows of x.  tgt [n][m] int64 (device) may repeat a row and
 *   need not hold neighbours.  AVA_EINVAL unless 1 <= m <= ava_eq_max_targets() = 63, 2 <= n < 2^31 - 64,
 *   1 <= d <= 65536 and every target is in [0, n) and is not its own row: the targets are checked on the device first,
 *   and the call waits for that answer.  col_splits workgroups share the reference rows of every 64-row query tile and
 *   add their counts into the table (0: enough of them to fill the device; more than there are tiles: one per tile);
 *   the table is the same for every value.  ws: ava_eq_workspace_bytes(n, m) bytes (0 for an unsupported shape).
 * ava_eq_penalties: pen [n][n_k] int64 = sum_{s < ks[a]} max(0, rank[i][s] - ks[a]) and totals [n_k] int64, their sums
 *   over the rows.
 * ava_eq_overlap: overlap [n][n_k] int = #{ (s, t) : a[i][s] == b[i][t], s < ks[a], t < ks[a] } of two tables [n][m]
 *   int64 (entries below 0 match nothing) and totals [n_k] int64, their sums over the rows. */
int ava_eq_max_targets(void);
int ava_eq_max_sweep(void);
size_t ava_eq_workspace_bytes(int n, int m);
int ava_eq_ranks(const void* x, int dtype, int n, int d, const int64_t* tgt, int m, int col_splits, int* rank, void* ws,
                 size_t ws_bytes, ava_stream_t s);
int ava_eq_penalties(const int* rank, int n, int m, const int* ks, int n_k, int64_t* pen, int64_t* totals,
                     ava_stream_t s);
int ava_eq_overlap(const int64_t* a, const int64_t* b, int n, int m, const int* ks, int n_k, int* overlap,
                   int64_t* totals, ava_stream_t s);
