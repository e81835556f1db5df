/* Connected components and a symmetric eigensolver over a sparse graph (row f27; csrc/spectral.hip).  Included by
 * ava_hip.h, inside its extern "C" block and after its typedefs; mirrored by _lib.SP_SIGNATURES.
 *
 * The graph is a symmetric CSR of n rows: indptr [n + 1] int64 with indptr[0] = 0 and indptr[n] = nnz, col [nnz] int32
 * (sorted within a row), val [nnz] fp64, all on the device.  Everything is fp64.  A stored diagonal entry is ignored
 * everywhere, and so is a stored zero.  Every entry point that follows the graph first checks it on the device
 * (indptr ascending within [0, nnz], every col in [0, n)) and waits for that answer: AVA_EINVAL before anything reads
 * through an index.
 *   deg[i]   = sum over j != i of val[i][j]; dd[i] = sqrt(deg[i]), or 1 where deg[i] = 0 (an isolated row)
 *   M        = D^-1/2 A D^-1/2 with the diagonal excluded = I - L_sym: y[i] = (sum_j val[i][j] (x[j] / dd[j])) / dd[i],
 *              the divisions as multiplications by 1 / dd
 * A row's sum is taken by 16 lanes, lane l over the row's entries l, l + 16, ... ascending, and the 16 partial sums by
 * a butterfly; sums over rows go over chunks of ava_sp_chunk_rows() = 1024 rows (a lane over the rows lane + 64 k of the
 * chunk ascending, the 64 lanes by a butterfly) and the chunks are added ascending (a squared norm: blocks of 256 rows,
 * added by a fixed tree).  No sum depends on the launch shape and no kernel uses a floating-point atomic, so two runs
 * give the same bits.
 *
 * The basis is [capacity][n] fp64, vector v at basis + v n: nlock locked vectors first, then the Lanczos vectors.
 * ws: ava_sp_workspace_bytes(n, capacity) bytes (0 for an unsupported shape) serve every entry point.
 *
 * ava_sp_components: labels [n] int (device): components numbered in the order of their smallest row; *count (host):
 *   how many.  Min-label propagation with pointer jumping; the call waits for the device after every round.
 * ava_sp_degrees: deg [n], dd [n].
 * ava_sp_apply: y = M x; x and y [n] must not overlap.
 * ava_sp_null_vectors: basis[c] = dd o [labels == c] normalised, c < k: the null space of L_sym, one vector per
 *   component (e_i for an isolated row).
 * ava_sp_start: basis[nlock] = the vector u01(mix64(row, seed)) - 1/2, orthogonalised twice against basis[0 .. nlock) and
 *   normalised; norm [1] (device) its length before that.  A length <= breakdown gives the zero vector.
 * ava_sp_lanczos: steps j0 <= j < j1 with no host synchronisation between them.  Step j: w = M basis[nlock + j]; twice
 *   h = B^T w, w -= B h over B = basis[0 .. nlock + j]; alpha[j] = the two coefficients of basis[nlock + j] added,
 *   beta[j] = |w|, basis[nlock + j + 1] = w / beta[j] (the zero vector where beta[j] <= breakdown).  alpha, beta [j1]
 *   on the device.  AVA_EINVAL unless 0 <= j0 <= j1 and nlock + j1 + 1 <= capacity <= ava_sp_max_basis().
 * ava_sp_rotate: basis[0 .. keep) <- sum_c basis[c] S[c][.] over c < ncv, c ascending; S [ncv][keep] on the device,
 *   1 <= keep <= ncv <= capacity.  Tiles of ava_sp_rotate_tile() = 8 output vectors.
 * n <= ava_sp_max_n() = 2^30. */
int ava_sp_max_n(void);
int ava_sp_max_basis(void);
int ava_sp_chunk_rows(void);
int ava_sp_rotate_tile(void);
size_t ava_sp_workspace_bytes(int n, int capacity);
int ava_sp_components(const int64_t* indptr, const int* col, const double* val, int n, int64_t nnz, int* labels,
                      int* count, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_sp_degrees(const int64_t* indptr, const int* col, const double* val, int n, int64_t nnz, double* deg,
                   double* dd, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_sp_apply(const int64_t* indptr, const int* col, const double* val, const double* dd, int n, int64_t nnz,
                 const double* x, double* y, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_sp_null_vectors(const int* labels, const double* dd, int n, int k, double* basis, int capacity, void* ws,
                        size_t ws_bytes, ava_stream_t s);
int ava_sp_start(double* basis, int n, int capacity, int nlock, uint64_t seed, double breakdown, double* norm,
                 void* ws, size_t ws_bytes, ava_stream_t s);
int ava_sp_lanczos(const int64_t* indptr, const int* col, const double* val, const double* dd, int n, int64_t nnz,
                   double* basis, int capacity, int nlock, int j0, int j1, double breakdown, double* alpha,
                   double* beta, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_sp_rotate(double* basis, int n, int capacity, int ncv, int keep, const double* S, void* ws, size_t ws_bytes,
                  ava_stream_t s);
