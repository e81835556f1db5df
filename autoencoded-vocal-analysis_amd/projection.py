"""UMAP and PCA projections of latent means on the device: DataContainer's ``'latent_mean_umap'`` and
``'latent_mean_pca'`` fields (``ava/data/data_container.py:514-551``).

  ``UMAP``            ``umap.UMAP(n_components=2, n_neighbors=20, min_dist=0.1, metric='euclidean', random_state=42)``
                      with umap-learn 0.5 semantics: exact kNN, bandwidths and memberships, and every layout epoch in
                      ``csrc/projection.hip``; the fuzzy union, the schedule, ``(a, b)`` and the init on the host
  ``pca_projection``  ``PCA(n_components, copy=False, random_state=42).fit_transform(X)`` through sklearn's
                      ``covariance_eigh`` path: device column sums and Gram matrix, host ``eigh``, device projection
  ``TransformableUMAP``  ``UMAP`` that also keeps its float32 training rows on the device (N x d x 4 bytes of HBM: about
                      0.65 GB for the 10 000 spectrograms of ~16 000 bins that ``refine_segments`` fits) and embeds
                      new rows with ``transform``: query kNN, bipartite memberships, weighted-mean start positions and a
                      layout that moves only the new points, all in ``csrc/projection.hip``
                      ``TransformableUMAP(metric='correlation')`` is ``umap.UMAP(metric='correlation')``: the kNN of
                      ``fit`` and ``transform`` under the correlation distance (``pj_knn_corr_kernel``, the centred
                      dot products on the fp64 matrix cores), the rows' means and sums of squares kept beside the rows
  ``install``         points ``DataContainer._make_latent_mean_umap_projection`` / ``_make_latent_mean_pca_projection``
                      here

Deviations from umap-learn, on purpose (INTEGRATION.md lists them too):

* the kNN search is exact for every N, ordered by (distance, index), the row itself first; umap-learn uses NN-descent
  for N >= 4096 and an unstable argsort of float32 distances below that;
* distances, bandwidths and positions are fp64; the embedding is returned as float32;
* each layout epoch is one synchronous update from the previous epoch's positions (umap-learn moves one edge at a
  time); the tail move of edge (v, j) is applied through the reverse edge (j, v), which the symmetric graph holds with
  the same weight and schedule; negative samples come from a counter-based hash, and a negative sample at distance 0
  moves nothing;
* a disconnected graph, or an ``eigsh`` that fails, falls back to the random init with a warning (umap-learn lays
  the components out with a meta-embedding);
* ``UMAP.transform`` (new points) is not supported: ``UMAP.fit`` keeps no training rows.  ``TransformableUMAP`` does,
  and its ``transform`` follows umap-learn 0.5's with the same deviations: the query kNN is exact and ordered by
  (distance, index) (umap-learn searches its NN-descent index), everything is fp64 (umap-learn initialises and lays
  out in float32), the negative samples come from the counter-based hash salted by
  ``RandomState(transform_seed).randint(2**31 - 1)``, and a negative sample at distance 0 moves nothing.  The moves
  are applied edge by edge, as umap-learn applies them, in slot order;
* ``metric='correlation'`` is accepted by ``TransformableUMAP`` only (``UMAP`` keeps refusing it; every other metric
  is ``NotImplementedError`` in both).  The distance is fp64 ``1 - c`` with ``c`` clipped to [-1, 1] (umap-learn's
  numba ``correlation`` works in float32 and does not clip).  Zero-variance rows follow what umap-learn's
  ``correlation`` does as far as it was recalled when this was written: 0.0 between two constant rows, 1.0 between a
  constant row and any other, a row being constant when its centred sum of squares is exactly 0.  That rule was
  recalled from memory and not checked against umap-learn, which was not installed where this was written.

There is no CPU fallback: the kernels need the MI355X.
"""
import warnings

import numpy as np
import scipy.sparse
import torch

from . import _lib, _rows

__all__ = ["UMAP", "TransformableUMAP", "pca_projection", "install", "knn", "knn_query", "smooth_knn",
           "smooth_knn_bipartite", "transform_init", "transform_layout", "fuzzy_union", "find_ab_params",
           "epochs_per_sample", "init_embedding", "Layout", "MAX_K", "MAX_DIM", "MAX_PCA_DIM"]

MAX_K = 64                 # n_neighbors the kNN kernel keeps per row (the row itself included)
MAX_DIM = 65536            # row length of the kNN kernel (as neighbors.MAX_DIM)
MAX_PCA_DIM = 512          # row length of the Gram kernel
MAX_NEG = 16               # negative samples per edge and epoch the layout kernel draws at most
MAX_NEGATIVE_SAMPLE_RATE = 7   # keeps n_neg <= 2 rate + 1 <= 16


def _device():
    return _lib.device("projection")


def _as_rows(X, dtype=None):
    """``X`` as a contiguous 2-D device tensor of ``dtype`` (numpy arrays and host tensors are uploaded); without
    ``dtype`` float32 / float64 inputs are read as they are, everything else as float64."""
    t = X.detach() if torch.is_tensor(X) else np.asarray(X)
    if dtype is None:
        t = _rows.native(t)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("expected a non-empty 2-D array, got shape %s" % (tuple(t.shape),))
    t = _rows.upload(t, _device(), dtype)
    if not _rows.is_finite(t):
        raise ValueError("input contains NaN or infinity")
    return t


METRICS = ('euclidean', 'correlation')     # of knn / knn_query


def _check_metric(metric):
    if metric not in METRICS:
        raise NotImplementedError("metric must be one of %r, got %r" % (METRICS, metric))


def _row_stats_device(xd):
    """``[n, 2]`` float64 on the device: the fp64 mean and the centred sum of squares of every row
    (``ava_pj_row_stats``), what the correlation kNN needs of either operand"""
    n, d = int(xd.shape[0]), int(xd.shape[1])
    if d > MAX_DIM or n >= 2 ** 31:
        raise ValueError("unsupported shape [%d, %d]" % (n, d))
    stats = torch.empty((n, 2), dtype=torch.float64, device=xd.device)
    _lib.check(_lib.load().ava_pj_row_stats(xd.data_ptr(), _lib.dtype_code(xd), n, d, stats.data_ptr(), _lib.stream()),
               "ava_pj_row_stats")
    return stats


def _knn_device(xd, k, chunk_rows=None, qd=None, metric='euclidean', xstat=None):
    """the kNN table of the rows of ``qd`` among the rows of ``xd``; without ``qd`` of ``xd``'s own rows, the row itself
    first (``ava_pj_knn``).  ``metric='correlation'`` goes to ``ava_pj_knn_corr``; ``xstat`` are ``xd``'s row
    statistics if the caller keeps them."""
    _check_metric(metric)
    m, n, d = int((xd if qd is None else qd).shape[0]), int(xd.shape[0]), int(xd.shape[1])
    if qd is not None and int(qd.shape[1]) != d:
        raise ValueError("queries have %d columns, references %d" % (int(qd.shape[1]), d))
    if qd is not None and qd.dtype != xd.dtype:
        raise ValueError("queries and references must have one dtype")
    if not 1 <= k <= min(MAX_K, n):
        raise ValueError("k must be in [1, min(%d, n)], got %d" % (MAX_K, k))
    if d > MAX_DIM or n >= 2 ** 31 or m >= 2 ** 31:
        raise ValueError("unsupported shape [%d, %d]" % (n, d) if qd is None else
                         "unsupported shapes [%d, %d], [%d, %d]" % (m, d, n, d))
    if chunk_rows is None:
        chunk_rows = m
    elif int(chunk_rows) != chunk_rows or chunk_rows < 1:
        raise ValueError("chunk_rows must be a positive integer")
    chunk_rows = min(int(chunk_rows), m)
    lib = _lib.load()
    idx = torch.empty((m, k), dtype=torch.int64, device=xd.device)
    dist = torch.empty((m, k), dtype=torch.float64, device=xd.device)
    st = _lib.stream()
    corr, code = metric == 'correlation', _lib.dtype_code(xd)
    if corr:
        if xstat is None:
            xstat = _row_stats_device(xd)
        if tuple(xstat.shape) != (n, 2) or xstat.dtype != torch.float64 or not xstat.is_contiguous():
            raise ValueError("the row statistics must be a contiguous float64 [%d, 2]" % n)
        qstat = None if qd is None else _row_stats_device(qd)
    for q0 in range(0, m, chunk_rows):
        nq = min(chunk_rows, m - q0)
        out = (k, q0, nq, idx[q0:].data_ptr(), dist[q0:].data_ptr(), st)
        if corr and qd is None:
            _lib.check(lib.ava_pj_knn_corr(xd.data_ptr(), code, xstat.data_ptr(), n, d, *out), "ava_pj_knn_corr")
        elif corr:
            _lib.check(lib.ava_pj_knn_corr_query(qd.data_ptr(), xd.data_ptr(), code, qstat.data_ptr(), xstat.data_ptr(),
                                                 m, n, d, *out), "ava_pj_knn_corr_query")
        elif qd is None:
            _lib.check(lib.ava_pj_knn(xd.data_ptr(), code, n, d, *out), "ava_pj_knn")
        else:
            _lib.check(lib.ava_pj_knn_query(qd.data_ptr(), xd.data_ptr(), code, m, n, d, *out), "ava_pj_knn_query")
    return idx, dist


def _knn_query_device(qd, xd, k, chunk_rows=None, metric='euclidean', xstat=None):
    return _knn_device(xd, k, chunk_rows, qd, metric, xstat)


def knn(X, k, chunk_rows=None, metric='euclidean'):
    """Exact kNN of every row of ``X`` among its rows (fp64 from the given values): ``(idx int64 [n, k],
    dist float64 [n, k])``.  Column 0 is the row itself at distance 0, then the ``k - 1`` nearest other rows ordered
    by (distance, index).  ``chunk_rows`` query rows go to one launch; the result does not depend on it.

    ``metric`` is ``'euclidean'`` or ``'correlation'`` (anything else: ``NotImplementedError``).  The correlation
    distance is ``1 - c``, ``c`` the cosine of the two centred rows clipped to [-1, 1]; a row is constant when its
    centred sum of squares is exactly 0, and then the distance is 0 to another constant row and 1 to any other, so
    every distance is finite."""
    _check_metric(metric)
    xd = _as_rows(X)
    idx, dist = _knn_device(xd, int(k), chunk_rows, metric=metric)
    return idx.cpu().numpy(), dist.cpu().numpy()


def knn_query(Q, X, k, chunk_rows=None, metric='euclidean'):
    """Exact kNN of every row of ``Q`` among the rows of ``X`` (fp64 from the given values, the arithmetic and the
    metrics of ``knn``): ``(idx int64 [m, k], dist float64 [m, k])`` ordered by (distance, index).  No row is
    excluded: under the euclidean metric a query that is a copy of reference row ``r`` gets ``(r, 0.0)`` first.  ``Q``
    is read in the dtype of ``X``.  ``chunk_rows`` query rows go to one launch; the result does not depend on it."""
    _check_metric(metric)
    xd = _as_rows(X)
    qd = _as_rows(Q, xd.dtype)
    idx, dist = _knn_query_device(qd, xd, int(k), chunk_rows, metric)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _smooth_device(idx, dist, local_connectivity, bipartite=False):
    n, k = int(idx.shape[0]), int(idx.shape[1])
    lib = _lib.load()
    mean = torch.empty(1, dtype=torch.float64, device=idx.device)
    sigma = torch.empty(n, dtype=torch.float64, device=idx.device)
    rho = torch.empty_like(sigma)
    w = torch.empty((n, k), dtype=torch.float64, device=idx.device)
    fn = lib.ava_pj_smooth_bipartite if bipartite else lib.ava_pj_smooth
    _lib.check(fn(dist.data_ptr(), idx.data_ptr(), n, k, float(local_connectivity), mean.data_ptr(),
                  sigma.data_ptr(), rho.data_ptr(), w.data_ptr(), _lib.stream()),
               "ava_pj_smooth_bipartite" if bipartite else "ava_pj_smooth")
    return sigma, rho, w


def _upload_table(idx, dist):
    dev = _device()
    idx = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
    dist = torch.as_tensor(np.ascontiguousarray(dist, dtype=np.float64)).to(dev)
    if idx.dim() != 2 or idx.shape != dist.shape or idx.shape[0] < 1 or not 1 <= idx.shape[1] <= MAX_K:
        raise ValueError("idx and dist must both be [n, k] with k <= %d" % MAX_K)
    return idx, dist


def smooth_knn(idx, dist, local_connectivity=1.0):
    """umap's ``smooth_knn_dist`` and ``compute_membership_strengths`` of a kNN table (as ``knn`` returns it), on the
    device: ``(sigma [n], rho [n], w [n, k])`` float64 numpy arrays."""
    idx, dist = _upload_table(idx, dist)
    sigma, rho, w = _smooth_device(idx, dist, local_connectivity)
    return sigma.cpu().numpy(), rho.cpu().numpy(), w.cpu().numpy()


def smooth_knn_bipartite(idx, dist, local_connectivity=0.0):
    """``smooth_knn`` for a query table (as ``knn_query`` returns it), umap's ``compute_membership_strengths(...,
    bipartite=True)``: no weight is zeroed where ``idx`` equals the row number.  ``transform`` passes
    ``max(0, local_connectivity - 1)``."""
    if not local_connectivity >= 0.0:
        raise ValueError("local_connectivity must be >= 0")
    idx, dist = _upload_table(idx, dist)
    sigma, rho, w = _smooth_device(idx, dist, local_connectivity, bipartite=True)
    return sigma.cpu().numpy(), rho.cpu().numpy(), w.cpu().numpy()


def fuzzy_union(idx, w, n, set_op_mix_ratio=1.0):
    """The fuzzy simplicial set of umap's ``fuzzy_simplicial_set``: ``A + A^T - A o A^T`` (mixed with ``A o A^T`` by
    ``set_op_mix_ratio``) of the membership matrix ``A[i, idx[i, j]] = w[i, j]``, zeros eliminated: a scipy CSR
    matrix with sorted indices."""
    k = idx.shape[1]
    A = scipy.sparse.coo_matrix((np.asarray(w, dtype=np.float64).ravel(),
                                 (np.repeat(np.arange(n), k), np.asarray(idx).ravel())), shape=(n, n)).tocsr()
    A.eliminate_zeros()
    At = A.transpose().tocsr()
    prod = A.multiply(At)
    G = set_op_mix_ratio * (A + At - prod) + (1.0 - set_op_mix_ratio) * prod
    G = scipy.sparse.csr_matrix(G)
    G.eliminate_zeros()
    G.sort_indices()
    return G


def find_ab_params(spread=1.0, min_dist=0.1):
    """umap's ``find_ab_params``: fit ``1 / (1 + a x^(2b))`` to the target membership curve."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def epochs_per_sample(weights, n_epochs):
    """umap's ``make_epochs_per_sample``: ``n_epochs / (n_epochs * w / max w)``, -1 where that count is 0."""
    result = -1.0 * np.ones(weights.shape[0], dtype=np.float64)
    n_samples = n_epochs * (weights / weights.max())
    result[n_samples > 0] = float(n_epochs) / np.float64(n_samples[n_samples > 0])
    return result


def _spectral(graph):
    """Eigenvectors 1 and 2 of the normalised Laplacian (umap's ``spectral_layout`` for a connected graph), or None
    (with a warning) when the graph is disconnected or ``eigsh`` fails."""
    from scipy.sparse.csgraph import connected_components
    from scipy.sparse.linalg import eigsh, ArpackError
    n = graph.shape[0]
    n_comp, _ = connected_components(graph)
    if n_comp > 1:
        warnings.warn("the graph has %d connected components: using the random init" % n_comp)
        return None
    diag = np.asarray(graph.sum(axis=0))
    I = scipy.sparse.identity(n, dtype=np.float64)
    D = scipy.sparse.spdiags(1.0 / np.sqrt(diag), 0, n, n)
    L = I - D * graph * D
    try:
        vals, vecs = eigsh(L, 3, which="SM", ncv=max(7, int(np.sqrt(n))), tol=1e-4, v0=np.ones(n), maxiter=n * 5)
    except (ArpackError, ValueError) as e:
        warnings.warn("the spectral init failed (%s): using the random init" % e)
        return None
    order = np.argsort(vals)[1:3]
    return vecs[:, order]


def _spectral_device(graph, tol=1e-4, maxiter=None):
    """``_spectral`` with the components and the eigensolver of ``ava_amd.spectral`` on the device: the same result
    up to ``tol`` and the sign of each vector, None (with the same warnings) in the same cases"""
    from . import spectral as _sp
    try:
        n_comp, Y = _sp.umap_eigenvectors(graph, tol=tol, maxiter=maxiter)
    except _sp.SpectralConvergenceError as e:
        warnings.warn("the spectral init failed (%s): using the random init" % e)
        return None
    if Y is None:
        warnings.warn("the graph has %d connected components: using the random init" % n_comp)
    return Y


def init_embedding(graph, init, rs, eigen_solver='scipy', tol=1e-4, maxiter=None):
    """The initial positions (float64 ``[n, 2]``) drawn from ``rs`` (a ``np.random.RandomState``): ``'spectral'``
    (max |.| scaled to 10, plus ``rs.normal(scale=1e-4)``; the random init if that is impossible) or ``'random'``
    (``rs.uniform(-10, 10)``), then every column rescaled to [0, 10].  ``eigen_solver``: ``'scipy'`` (ARPACK on the host)
    or ``'device'`` (``ava_amd.spectral``, residual at most ``tol`` within ``maxiter`` operator applications)."""
    if eigen_solver not in ('scipy', 'device'):
        raise ValueError("eigen_solver must be 'scipy' or 'device', got %r" % (eigen_solver,))
    n = graph.shape[0]
    Y = None
    if init == 'spectral':
        Y = _spectral(graph) if eigen_solver == 'scipy' else _spectral_device(graph, tol, maxiter)
    if Y is not None:
        Y = Y * (10.0 / np.abs(Y).max()) + rs.normal(scale=0.0001, size=[n, 2])
    else:
        Y = rs.uniform(low=-10.0, high=10.0, size=(n, 2))
    lo, hi = Y.min(0), Y.max(0)
    return 10.0 * (Y - lo) / (hi - lo)


class Layout:
    """Device state of the SGD layout over a pruned symmetric CSR ``graph``: positions, per-edge schedules and the
    two sample counters.  ``run(e0, e1)`` enqueues epochs ``[e0, e1)`` with no host synchronisation in between;
    ``positions()`` returns the fp64 positions as numpy."""

    def __init__(self, graph, Y0, n_epochs, a, b, gamma=1.0, learning_rate=1.0, negative_sample_rate=5, salt=0):
        dev = _device()
        n = graph.shape[0]
        self.n, self.nnz, self.n_epochs = n, int(graph.nnz), int(n_epochs)
        self.a, self.b, self.gamma, self.learning_rate = float(a), float(b), float(gamma), float(learning_rate)
        self.salt = int(salt)
        eps = epochs_per_sample(graph.data, self.n_epochs) if self.nnz else np.zeros(0)
        epn = eps / negative_sample_rate

        def up(a, dtype):
            return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(dev)
        self.indptr = up(graph.indptr, np.int64)
        self.col = up(graph.indices, np.int32)
        self.eps, self.epn = up(eps, np.float64), up(epn, np.float64)
        self.next_s, self.next_n = self.eps.clone(), self.epn.clone()
        self.y = up(Y0, np.float64).reshape(n, 2).contiguous()
        self.y_tmp = torch.empty_like(self.y)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.epoch = 0

    def run(self, e0=None, e1=None):
        e0 = self.epoch if e0 is None else int(e0)
        e1 = self.n_epochs if e1 is None else int(e1)
        if e0 != self.epoch or not e0 <= e1 <= self.n_epochs:
            raise ValueError("epochs [%d, %d) do not continue from epoch %d of %d" % (e0, e1, self.epoch,
                                                                                    self.n_epochs))
        if e1 > e0 and self.nnz:
            lib = _lib.load()
            _lib.check(lib.ava_pj_layout(self.y.data_ptr(), self.y_tmp.data_ptr(), self.indptr.data_ptr(),
                                         self.col.data_ptr(), self.eps.data_ptr(), self.epn.data_ptr(),
                                         self.next_s.data_ptr(), self.next_n.data_ptr(), self.n, self.nnz, e0, e1,
                                         self.n_epochs, self.learning_rate, self.a, self.b, self.gamma, self.salt,
                                         self.flag.data_ptr(), _lib.stream()), "ava_pj_layout")
        self.epoch = e1
        return self

    def positions(self):
        if int(self.flag.item()):
            raise _lib.AvaHipError("an edge needed more than %d negative samples in one epoch" % MAX_NEG)
        return self.y.cpu().numpy()


def _transform_init_device(w, idx, emb):
    m, k = int(idx.shape[0]), int(idx.shape[1])
    lib = _lib.load()
    wn = torch.empty((m, k), dtype=torch.float64, device=idx.device)
    y0 = torch.empty((m, 2), dtype=torch.float64, device=idx.device)
    _lib.check(lib.ava_pj_transform_init(w.data_ptr(), idx.data_ptr(), emb.data_ptr(), m, k, wn.data_ptr(),
                                         y0.data_ptr(), _lib.stream()), "ava_pj_transform_init")
    return wn, y0


def _transform_layout_device(y, emb, idx, eps, epn, n_epochs, a, b, gamma, learning_rate, salt, epochs=None):
    """moves ``y`` [m, 2] (device, in place); ``eps`` / ``epn`` [k, m] slot-major device tensors"""
    m, k = int(idx.shape[0]), int(idx.shape[1])
    epochs = int(n_epochs) if epochs is None else int(epochs)
    if not 0 <= epochs <= n_epochs:
        raise ValueError("epochs must be in [0, n_epochs]")
    flag = torch.zeros(1, dtype=torch.int32, device=y.device)
    lib = _lib.load()
    _lib.check(lib.ava_pj_transform_layout(y.data_ptr(), emb.data_ptr(), idx.data_ptr(), eps.data_ptr(),
                                           epn.data_ptr(), m, k, int(emb.shape[0]), epochs, int(n_epochs),
                                           float(learning_rate), float(a), float(b), float(gamma), int(salt),
                                           flag.data_ptr(), _lib.stream()), "ava_pj_transform_layout")
    return flag


def _upload_neighbours(idx, w, emb):
    dev = _device()
    idx = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
    w = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    emb = torch.as_tensor(np.ascontiguousarray(emb, dtype=np.float64)).to(dev)
    if idx.dim() != 2 or idx.shape != w.shape or idx.shape[0] < 1 or not 1 <= idx.shape[1] <= MAX_K:
        raise ValueError("idx and the weights must both be [m, k] with k <= %d" % MAX_K)
    if emb.dim() != 2 or emb.shape[1] != 2 or emb.shape[0] < 1:
        raise ValueError("the training embedding must be [n, 2]")
    if int(idx.min()) < 0 or int(idx.max()) >= emb.shape[0]:
        raise ValueError("idx must lie in [0, %d)" % emb.shape[0])
    return idx, w, emb


def transform_init(idx, w, embedding):
    """sklearn's ``normalize(w, norm='l1')`` (rows summed left to right, a row of sum 0 stays 0) and umap's
    ``init_transform``: ``(wn [m, k], Y0 [m, 2])`` float64, ``Y0[i] = sum_s wn[i, s] embedding[idx[i, s]]`` in slot
    order, on the device."""
    idx, w, emb = _upload_neighbours(idx, w, embedding)
    wn, y0 = _transform_init_device(w, idx, emb)
    return wn.cpu().numpy(), y0.cpu().numpy()


def transform_schedule(w, n_epochs, negative_sample_rate=5):
    """``(eps, epn)`` [m, k]: umap's ``make_epochs_per_sample`` of the slots that survive ``w < w.max() / n_epochs``
    (the maximum of the whole batch), -1 for the pruned ones, and ``eps / negative_sample_rate``"""
    w = np.asarray(w, dtype=np.float64)
    eps = np.full(w.shape, -1.0)
    keep = ~(w < w.max() / float(n_epochs)) & (w != 0.0)
    if keep.any():
        eps[keep] = epochs_per_sample(w[keep], n_epochs)
    return eps, eps / negative_sample_rate


def transform_layout(Y0, embedding, idx, eps, epn, n_epochs, a, b, salt, epochs=None, gamma=1.0, learning_rate=1.0):
    """``epochs`` (default all) of ``n_epochs`` of the transform layout from ``Y0`` [m, 2] against the fixed
    ``embedding`` [n, 2], on the device, one launch: ``(Y float64 [m, 2], flagged)``.  ``eps`` / ``epn`` [m, k] as
    ``transform_schedule`` returns them; ``flagged`` tells whether a slot was due more than 16 negative samples in one
    epoch (it drew 16)."""
    idx, eps, emb = _upload_neighbours(idx, eps, embedding)
    epn = torch.as_tensor(np.ascontiguousarray(epn, dtype=np.float64)).to(idx.device)
    y = torch.as_tensor(np.ascontiguousarray(Y0, dtype=np.float64)).to(idx.device)
    if epn.shape != eps.shape or y.shape != (idx.shape[0], 2):
        raise ValueError("epn must be [m, k] and Y0 [m, 2]")
    if int(n_epochs) < 1:
        raise ValueError("n_epochs must be positive")
    flag = _transform_layout_device(y, emb, idx, eps.t().contiguous(), epn.t().contiguous(), int(n_epochs), a, b, gamma,
                                    learning_rate, salt, epochs)
    return y.cpu().numpy(), bool(int(flag.item()))


class UMAP:
    """``umap.UMAP`` for ``n_components=2`` and ``metric='euclidean'`` with the hot path on the device (see the
    module docstring for the deviations).  ``fit_transform(X)`` returns float32 ``[N, 2]``."""

    def __init__(self, n_components=2, n_neighbors=20, min_dist=0.1, metric='euclidean', random_state=42,
                 n_epochs=None, init='spectral', spread=1.0, learning_rate=1.0, repulsion_strength=1.0,
                 negative_sample_rate=5, set_op_mix_ratio=1.0, local_connectivity=1.0, eigen_solver='scipy'):
        self.n_components = n_components
        self.n_neighbors = n_neighbors
        self.min_dist = min_dist
        self.metric = metric
        self.random_state = random_state
        self.n_epochs = n_epochs
        self.init = init
        self.spread = spread
        self.learning_rate = learning_rate
        self.repulsion_strength = repulsion_strength
        self.negative_sample_rate = negative_sample_rate
        self.set_op_mix_ratio = set_op_mix_ratio
        self.local_connectivity = local_connectivity
        self.eigen_solver = eigen_solver     # of the spectral init: 'scipy' (host ARPACK) or 'device' (ava_amd.spectral)

    METRICS = ('euclidean',)                # the metrics _validate accepts

    def _validate(self):
        if self.n_components != 2:
            raise NotImplementedError("only n_components=2 is supported, got %r" % (self.n_components,))
        if self.metric not in self.METRICS:
            raise NotImplementedError("%s supports metric in %r, got %r"
                                      % (type(self).__name__, self.METRICS, self.metric))
        if int(self.n_neighbors) != self.n_neighbors or not 2 <= self.n_neighbors <= MAX_K:
            raise ValueError("n_neighbors must be an integer in [2, %d], got %r" % (MAX_K, self.n_neighbors))
        if self.init not in ('spectral', 'random'):
            raise ValueError("init must be 'spectral' or 'random', got %r" % (self.init,))
        if getattr(self, 'eigen_solver', 'scipy') not in ('scipy', 'device'):
            raise ValueError("eigen_solver must be 'scipy' or 'device', got %r" % (self.eigen_solver,))
        if self.n_epochs is not None and (int(self.n_epochs) != self.n_epochs or self.n_epochs < 1):
            raise ValueError("n_epochs must be a positive integer or None, got %r" % (self.n_epochs,))
        if (int(self.negative_sample_rate) != self.negative_sample_rate or
                not 1 <= self.negative_sample_rate <= MAX_NEGATIVE_SAMPLE_RATE):
            raise ValueError("negative_sample_rate must be an integer in [1, %d], got %r"
                             % (MAX_NEGATIVE_SAMPLE_RATE, self.negative_sample_rate))
        if not 0.0 <= self.set_op_mix_ratio <= 1.0:
            raise ValueError("set_op_mix_ratio must be in [0, 1]")
        if not self.min_dist <= self.spread or self.min_dist < 0.0:
            raise ValueError("min_dist must be in [0, spread]")
        if self.local_connectivity < 0.0:
            raise ValueError("local_connectivity must be >= 0")

    def fit(self, X):
        self._validate()
        x32 = _as_rows(X, torch.float32)                 # umap's check_array(dtype=np.float32)
        n = int(x32.shape[0])
        if n == 1:
            self.embedding_ = np.zeros((1, 2), dtype=np.float32)
            self.graph_ = scipy.sparse.csr_matrix((1, 1), dtype=np.float64)
            self.sigmas_, self.rhos_ = np.zeros(1), np.zeros(1)
            self.a_, self.b_ = find_ab_params(self.spread, self.min_dist)
            self._n_neighbors = 1
            return self
        k = int(self.n_neighbors)
        if n <= k:
            warnings.warn("n_neighbors is larger than the dataset size; truncating to X.shape[0] - 1")
            k = n - 1
        self._n_neighbors = k
        idx, dist = self._fit_knn(x32, k)
        sigma, rho, w = _smooth_device(idx, dist, self.local_connectivity)
        self.graph_ = fuzzy_union(idx.cpu().numpy(), w.cpu().numpy(), n, self.set_op_mix_ratio)
        self.sigmas_, self.rhos_ = sigma.cpu().numpy(), rho.cpu().numpy()
        self.a_, self.b_ = find_ab_params(self.spread, self.min_dist)
        n_epochs = int(self.n_epochs) if self.n_epochs is not None else (500 if n <= 10000 else 200)
        graph = self.graph_.copy()
        if graph.nnz:
            graph.data[graph.data < graph.data.max() / float(n_epochs)] = 0.0
            graph.eliminate_zeros()
        rs = self.random_state if isinstance(self.random_state, np.random.RandomState) else \
            np.random.RandomState(self.random_state)
        Y0 = init_embedding(graph, self.init, rs, getattr(self, 'eigen_solver', 'scipy'))
        salt = rs.randint(2 ** 31 - 1)
        lay = Layout(graph, Y0, n_epochs, self.a_, self.b_, self.repulsion_strength, self.learning_rate,
                     self.negative_sample_rate, salt)
        self.embedding_ = lay.run().positions().astype(np.float32)
        return self

    def _fit_knn(self, x32, k):
        return _knn_device(x32, k)

    def fit_transform(self, X, y=None):
        return self.fit(X).embedding_

    def transform(self, X):
        raise NotImplementedError("UMAP.transform (embedding new points) is not supported")


class TransformableUMAP(UMAP):
    """``UMAP`` that can embed new rows: ``fit`` additionally keeps the float32 training rows on the device (N x d x 4
    bytes of HBM for as long as the object lives; 10 000 rows of 16 000 bins are 0.64 GB), beside ``embedding_``,
    ``a_`` and ``b_``; ``transform(X)`` follows umap-learn 0.5's ``transform`` (see the module docstring for the
    deviations) and returns float32 ``[m, 2]``.  ``transform_seed`` is umap-learn's argument of that name.

    ``metric='correlation'`` (what ``template_segmentation.clean_collected_segments`` fits) runs the kNN of ``fit`` and
    of ``transform`` under the correlation distance of ``knn``; the training rows' statistics (``N x 2`` doubles) stay
    on the device beside the rows.  Everything after the kNN works in the embedding plane and is the same.

    Pickling drops the device tensors: the pickle holds a host copy of the training rows, uploaded again by the first
    ``transform`` after loading, which also recomputes the statistics."""

    METRICS = ('euclidean', 'correlation')

    def __init__(self, n_components=2, n_neighbors=20, min_dist=0.1, metric='euclidean', random_state=42,
                 n_epochs=None, init='spectral', spread=1.0, learning_rate=1.0, repulsion_strength=1.0,
                 negative_sample_rate=5, set_op_mix_ratio=1.0, local_connectivity=1.0, transform_seed=42,
                 eigen_solver='scipy'):
        super().__init__(n_components, n_neighbors, min_dist, metric, random_state, n_epochs, init, spread,
                         learning_rate, repulsion_strength, negative_sample_rate, set_op_mix_ratio, local_connectivity,
                         eigen_solver)
        self.transform_seed = transform_seed
        self._train_rows = None          # float32 [N, d] on the device
        self._train_stats = None         # float64 [N, 2] on the device: the rows' statistics (metric='correlation')
        self._train_host = None          # the rows as numpy, only after unpickling and until the next transform

    def fit(self, X):
        self._validate()
        x32 = _as_rows(X, torch.float32)
        self._train_stats = None
        super().fit(x32)
        # _as_rows hands a tensor that is already float32, contiguous and on the device back as it is: keep a copy,
        # so that the caller may overwrite its own
        self._train_rows = x32.clone() if torch.is_tensor(X) and x32.data_ptr() == X.data_ptr() else x32
        self._train_host = None
        return self

    def _fit_knn(self, x32, k):
        if self.metric == 'correlation':
            self._train_stats = _row_stats_device(x32)
        return _knn_device(x32, k, metric=self.metric, xstat=self._train_stats)

    def __getstate__(self):
        state = dict(self.__dict__)
        rows = state.pop('_train_rows', None)
        if rows is not None:
            state['_train_host'] = rows.cpu().numpy()
        state['_train_rows'] = None
        state['_train_stats'] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    def _rows(self):
        if self._train_rows is None:
            if self._train_host is None:
                raise ValueError("transform needs a fitted TransformableUMAP: call fit first")
            self._train_rows = _as_rows(self._train_host, torch.float32)
            self._train_host = None
        if self.metric == 'correlation' and self.__dict__.get('_train_stats') is None:
            self._train_stats = _row_stats_device(self._train_rows)
        return self._train_rows

    def transform(self, X):
        if self._train_rows is None and self._train_host is None:
            raise ValueError("transform needs a fitted TransformableUMAP: call fit first")
        shape = tuple(X.shape) if torch.is_tensor(X) else np.shape(X)
        if len(shape) == 2 and shape[0] == 0:
            raise ValueError("transform needs at least one row")
        d = int(self._train_host.shape[1] if self._train_rows is None else self._train_rows.shape[1])
        if len(shape) == 2 and shape[1] != d:
            raise ValueError("X has %d columns, the training rows have %d" % (shape[1], d))
        q32 = _as_rows(X, torch.float32)
        train = self._rows()
        m, n = int(q32.shape[0]), int(train.shape[0])
        idx, dist = _knn_query_device(q32, train, int(self._n_neighbors), metric=self.metric,
                                      xstat=self.__dict__.get('_train_stats'))
        _, _, w = _smooth_device(idx, dist, max(0.0, self.local_connectivity - 1.0), bipartite=True)
        emb = torch.from_numpy(np.ascontiguousarray(self.embedding_, dtype=np.float64)).to(q32.device)
        _, y = _transform_init_device(w, idx, emb)        # from the weights of all slots: pruning comes after
        if self.n_epochs is None:
            n_epochs = 100 if m <= 10000 else 30
        else:
            n_epochs = int(self.n_epochs // 3)
        if n_epochs > 0:
            eps, epn = transform_schedule(w.cpu().numpy(), n_epochs, self.negative_sample_rate)
            salt = np.random.RandomState(self.transform_seed).randint(2 ** 31 - 1)

            def up(a):
                return torch.from_numpy(np.ascontiguousarray(a.T)).to(q32.device)
            flag = _transform_layout_device(y, emb, idx, up(eps), up(epn), n_epochs, self.a_, self.b_,
                                            self.repulsion_strength, self.learning_rate, salt)
            if int(flag.item()):
                raise _lib.AvaHipError("a slot needed more than %d negative samples in one epoch" % MAX_NEG)
        return y.cpu().numpy().astype(np.float32)


def pca_projection(X, n_components=2):
    """``sklearn.decomposition.PCA(n_components, copy=False, random_state=42).fit_transform(X)`` (float64
    ``[N, n_components]``) through sklearn 1.7's ``covariance_eigh`` path: the device sums the columns and ``X^T X``,
    the host forms the covariance, runs ``eigh`` and fixes the signs as ``svd_flip(u_based_decision=False)``, and the
    device projects ``X V^T - mu V^T``."""
    xd = _as_rows(X)
    n, d = int(xd.shape[0]), int(xd.shape[1])
    if int(n_components) != n_components or not 1 <= n_components <= min(n, d):
        raise ValueError("n_components must be an integer in [1, min(n, d)] = [1, %d], got %r"
                         % (min(n, d), n_components))
    if n < 2:
        raise ValueError("PCA needs at least 2 rows")
    if d > MAX_PCA_DIM:
        raise ValueError("row length %d exceeds %d" % (d, MAX_PCA_DIM))
    lib = _lib.load()
    nbytes = lib.ava_pj_gram_workspace_bytes(n, d)
    ws = _lib.workspace(nbytes, xd.device, "[%d, %d]" % (n, d))
    gram = torch.empty((d + 1, d + 1), dtype=torch.float64, device=xd.device)
    st = _lib.stream()
    _lib.check(lib.ava_pj_gram(xd.data_ptr(), _lib.dtype_code(xd), n, d, gram.data_ptr(), ws.data_ptr(), nbytes, st),
               "ava_pj_gram")
    g = gram.cpu().numpy()
    mean = g[:d, d] / n
    C = g[:d, :d] - n * mean.reshape(-1, 1) * mean.reshape(1, -1)
    C /= n - 1
    vals, vecs = np.linalg.eigh(C)
    Vt = np.flip(vecs, axis=1).T
    signs = np.sign(Vt[np.arange(d), np.argmax(np.abs(Vt), axis=1)])
    V = np.ascontiguousarray(Vt[:n_components] * signs[:n_components, None])
    muv = mean.reshape(1, -1) @ V.T
    Vd = torch.from_numpy(V).to(xd.device)
    mud = torch.from_numpy(np.ascontiguousarray(muv.ravel())).to(xd.device)
    out = torch.empty((n, n_components), dtype=torch.float64, device=xd.device)
    _lib.check(lib.ava_pj_project(xd.data_ptr(), _lib.dtype_code(xd), n, d, Vd.data_ptr(), mud.data_ptr(), n_components,
                                  out.data_ptr(), st), "ava_pj_project")
    return out.cpu().numpy()


def _make_latent_mean_umap_projection(self):
    """Project latent means to two dimensions with UMAP (data_container.py:514-535, on the device)."""
    latent_means = self.request('latent_means')
    transform = UMAP(n_components=2, n_neighbors=20, min_dist=0.1, metric='euclidean', random_state=42)
    if self.verbose:
        print("Running UMAP... (n="+str(len(latent_means))+")")
    embedding = transform.fit_transform(latent_means)
    if self.verbose:
        print("\tDone.")
    self._write_projection("latent_mean_umap", embedding)
    return embedding


def _make_latent_mean_pca_projection(self):
    """Project latent means to two dimensions with PCA (data_container.py:538-551, on the device)."""
    latent_means = self.request('latent_means')
    if self.verbose:
        print("Running PCA...")
    embedding = pca_projection(latent_means, n_components=2)
    if self.verbose:
        print("\tDone.")
    self._write_projection("latent_mean_pca", embedding)
    return embedding


def install(module=None):
    """Point ``DataContainer._make_latent_mean_umap_projection`` and ``_make_latent_mean_pca_projection`` of
    ``ava.data.data_container`` here (the reference package imports umap and h5py at import time, so a module
    object may be passed instead)."""
    if module is None:
        import ava.data.data_container as module
    module.DataContainer._make_latent_mean_umap_projection = _make_latent_mean_umap_projection
    module.DataContainer._make_latent_mean_pca_projection = _make_latent_mean_pca_projection
    return module
