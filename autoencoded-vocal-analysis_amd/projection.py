"""UMAP and PCA projections of latent means on the device: DataContainer's ``'latent_mean_umap'`` and
``'latent_mean_pca'`` fields (``ava/data/data_container.py:514-551``).

  ``UMAP``            ``umap.UMAP(n_components=2, n_neighbors=20, min_dist=0.1, metric='euclidean', random_state=42)``
                      with umap-learn 0.5 semantics: exact kNN, bandwidths and memberships, and every layout epoch in
                      ``csrc/projection.hip``; the fuzzy union, the schedule, ``(a, b)`` and the init on the host
  ``pca_projection``  ``PCA(n_components, copy=False, random_state=42).fit_transform(X)`` through sklearn's
                      ``covariance_eigh`` path: device column sums and Gram matrix, host ``eigh``, device projection
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
* ``transform`` (new points) is not supported.

There is no CPU fallback: the kernels need the MI355X.
"""
import warnings

import numpy as np
import scipy.sparse
import torch

from . import _lib

__all__ = ["UMAP", "pca_projection", "install", "knn", "smooth_knn", "fuzzy_union", "find_ab_params",
           "epochs_per_sample", "init_embedding", "Layout", "MAX_K", "MAX_DIM", "MAX_PCA_DIM"]

MAX_K = 64                 # n_neighbors the kNN kernel keeps per row (the row itself included)
MAX_DIM = 65536            # row length of the kNN kernel (as neighbors.MAX_DIM)
MAX_PCA_DIM = 512          # row length of the Gram kernel
MAX_NEG = 16               # negative samples per edge and epoch the layout kernel draws at most
MAX_NEGATIVE_SAMPLE_RATE = 7   # keeps n_neg <= 2 rate + 1 <= 16


def _device():
    if not torch.cuda.is_available():
        raise _lib.AvaHipError("the projection kernels only run on an MI355X: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _as_rows(X, dtype):
    """``X`` as a contiguous 2-D device tensor of ``dtype`` (numpy arrays and host tensors are uploaded)."""
    if torch.is_tensor(X):
        t = X.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(X)))
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("expected a non-empty 2-D array, got shape %s" % (tuple(t.shape),))
    t = t.to(device=_device(), dtype=dtype).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("input contains NaN or infinity")
    return t


def _native_dtype(X):
    """float32 / float64 inputs are read as they are, everything else as float64"""
    dt = X.dtype if torch.is_tensor(X) else torch.from_numpy(np.zeros(0, dtype=np.asarray(X).dtype)).dtype
    return dt if dt in (torch.float32, torch.float64) else torch.float64


def _code(t):
    return 0 if t.dtype == torch.float32 else 1


def _knn_device(xd, k, chunk_rows=None):
    n, d = int(xd.shape[0]), int(xd.shape[1])
    if not 1 <= k <= min(MAX_K, n):
        raise ValueError("k must be in [1, min(%d, n)], got %d" % (MAX_K, k))
    if d > MAX_DIM or n >= 2 ** 31:
        raise ValueError("unsupported shape [%d, %d]" % (n, d))
    if chunk_rows is None:
        chunk_rows = n
    elif int(chunk_rows) != chunk_rows or chunk_rows < 1:
        raise ValueError("chunk_rows must be a positive integer")
    chunk_rows = min(int(chunk_rows), n)
    lib = _lib.load()
    idx = torch.empty((n, k), dtype=torch.int64, device=xd.device)
    dist = torch.empty((n, k), dtype=torch.float64, device=xd.device)
    st = _lib.stream()
    for q0 in range(0, n, chunk_rows):
        nq = min(chunk_rows, n - q0)
        _lib.check(lib.ava_pj_knn(xd.data_ptr(), _code(xd), n, d, k, q0, nq, idx[q0:].data_ptr(),
                                  dist[q0:].data_ptr(), st), "ava_pj_knn")
    return idx, dist


def knn(X, k, chunk_rows=None):
    """Exact euclidean kNN of every row of ``X`` among its rows (fp64 from the given values): ``(idx int64 [n, k],
    dist float64 [n, k])``.  Column 0 is the row itself at distance 0, then the ``k - 1`` nearest other rows ordered
    by (distance, index).  ``chunk_rows`` query rows go to one launch; the result does not depend on it."""
    xd = _as_rows(X, _native_dtype(X))
    idx, dist = _knn_device(xd, int(k), chunk_rows)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _smooth_device(idx, dist, local_connectivity):
    n, k = int(idx.shape[0]), int(idx.shape[1])
    lib = _lib.load()
    mean = torch.empty(1, dtype=torch.float64, device=idx.device)
    sigma = torch.empty(n, dtype=torch.float64, device=idx.device)
    rho = torch.empty_like(sigma)
    w = torch.empty((n, k), dtype=torch.float64, device=idx.device)
    _lib.check(lib.ava_pj_smooth(dist.data_ptr(), idx.data_ptr(), n, k, float(local_connectivity), mean.data_ptr(),
                                 sigma.data_ptr(), rho.data_ptr(), w.data_ptr(), _lib.stream()), "ava_pj_smooth")
    return sigma, rho, w


def smooth_knn(idx, dist, local_connectivity=1.0):
    """umap's ``smooth_knn_dist`` and ``compute_membership_strengths`` of a kNN table (as ``knn`` returns it), on the
    device: ``(sigma [n], rho [n], w [n, k])`` float64 numpy arrays."""
    dev = _device()
    idx = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
    dist = torch.as_tensor(np.ascontiguousarray(dist, dtype=np.float64)).to(dev)
    if idx.dim() != 2 or idx.shape != dist.shape or not 1 <= idx.shape[1] <= MAX_K:
        raise ValueError("idx and dist must both be [n, k] with k <= %d" % MAX_K)
    sigma, rho, w = _smooth_device(idx, dist, local_connectivity)
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


def init_embedding(graph, init, rs):
    """The initial positions (float64 ``[n, 2]``) drawn from ``rs`` (a ``np.random.RandomState``): ``'spectral'``
    (max |.| scaled to 10, plus ``rs.normal(scale=1e-4)``; the random init if that is impossible) or ``'random'``
    (``rs.uniform(-10, 10)``), then every column rescaled to [0, 10]."""
    n = graph.shape[0]
    Y = _spectral(graph) if init == 'spectral' else None
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


class UMAP:
    """``umap.UMAP`` for ``n_components=2`` and ``metric='euclidean'`` with the hot path on the device (see the
    module docstring for the deviations).  ``fit_transform(X)`` returns float32 ``[N, 2]``."""

    def __init__(self, n_components=2, n_neighbors=20, min_dist=0.1, metric='euclidean', random_state=42,
                 n_epochs=None, init='spectral', spread=1.0, learning_rate=1.0, repulsion_strength=1.0,
                 negative_sample_rate=5, set_op_mix_ratio=1.0, local_connectivity=1.0):
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

    def _validate(self):
        if self.n_components != 2:
            raise NotImplementedError("only n_components=2 is supported, got %r" % (self.n_components,))
        if self.metric != 'euclidean':
            raise NotImplementedError("only metric='euclidean' is supported, got %r" % (self.metric,))
        if int(self.n_neighbors) != self.n_neighbors or not 2 <= self.n_neighbors <= MAX_K:
            raise ValueError("n_neighbors must be an integer in [2, %d], got %r" % (MAX_K, self.n_neighbors))
        if self.init not in ('spectral', 'random'):
            raise ValueError("init must be 'spectral' or 'random', got %r" % (self.init,))
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
            return self
        k = int(self.n_neighbors)
        if n <= k:
            warnings.warn("n_neighbors is larger than the dataset size; truncating to X.shape[0] - 1")
            k = n - 1
        idx, dist = _knn_device(x32, k)
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
        Y0 = init_embedding(graph, self.init, rs)
        salt = rs.randint(2 ** 31 - 1)
        lay = Layout(graph, Y0, n_epochs, self.a_, self.b_, self.repulsion_strength, self.learning_rate,
                     self.negative_sample_rate, salt)
        self.embedding_ = lay.run().positions().astype(np.float32)
        return self

    def fit_transform(self, X, y=None):
        return self.fit(X).embedding_

    def transform(self, X):
        raise NotImplementedError("UMAP.transform (embedding new points) is not supported")


def pca_projection(X, n_components=2):
    """``sklearn.decomposition.PCA(n_components, copy=False, random_state=42).fit_transform(X)`` (float64
    ``[N, n_components]``) through sklearn 1.7's ``covariance_eigh`` path: the device sums the columns and ``X^T X``,
    the host forms the covariance, runs ``eigh`` and fixes the signs as ``svd_flip(u_based_decision=False)``, and the
    device projects ``X V^T - mu V^T``."""
    xd = _as_rows(X, _native_dtype(X))
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
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xd.device)
    gram = torch.empty((d + 1, d + 1), dtype=torch.float64, device=xd.device)
    st = _lib.stream()
    _lib.check(lib.ava_pj_gram(xd.data_ptr(), _code(xd), n, d, gram.data_ptr(), ws.data_ptr(), nbytes, st),
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
    _lib.check(lib.ava_pj_project(xd.data_ptr(), _code(xd), n, d, Vd.data_ptr(), mud.data_ptr(), n_components,
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
