"""Spectral embedding (Laplacian eigenmaps) and spectral clustering of a sparse graph on the MI355X (SURVEY.md section
8, row f27), and the eigensolver behind ``projection.init_embedding(..., eigen_solver='device')``.

The reference package has no counterpart: the specification is scikit-learn 1.7's
``sklearn/manifold/_spectral_embedding.py::_spectral_embedding`` and ``sklearn/cluster/_spectral.py::SpectralClustering``
with ``affinity='nearest_neighbors'`` (or ``'precomputed'``) and ``assign_labels='kmeans'``.

The graph is a symmetric scipy sparse matrix A.  With ``deg = A 1`` (the diagonal left out), ``dd = sqrt(deg)`` (1 for
an isolated row) and ``L_sym = I - D^-1/2 A D^-1/2``, the wanted pairs are the smallest eigenvalues of ``L_sym``: the
largest ``mu`` of ``M = D^-1/2 A D^-1/2``, ``lambda = 1 - mu``.  The solver is thick-restart Lanczos (Wu & Simon), the same
Krylov method as ARPACK's implicitly restarted Lanczos, with full re-orthogonalisation (two passes of classical
Gram-Schmidt) on the device (``csrc/spectral.hip``); the host does the ``eigh`` of the projected matrix once per restart
cycle and the test ``|beta s_last| <= tol``.

=====================================  =====================================  ======================
step                                   here                                   C entry point
=====================================  =====================================  ======================
components of the graph                :func:`connected_components`           ``ava_sp_components``
``deg``, ``dd``                        ``_Graph``                             ``ava_sp_degrees``
``y = M x``                            ``_Graph.apply``                       ``ava_sp_apply``
the null space from the components     ``_solve``                             ``ava_sp_null_vectors``
start vector                           ``_solve``                             ``ava_sp_start``
Lanczos steps of a restart cycle       ``_solve``                             ``ava_sp_lanczos``
thick restart, Ritz vectors            ``_solve``                             ``ava_sp_rotate``
k-means of the embedding               :class:`SpectralClustering`            ``kmeans.KMeans`` (f25)
=====================================  =====================================  ======================

Deviations from scikit-learn / ARPACK, on purpose:

* single-vector Lanczos misses multiplicities, and the kNN graph of separated clusters is disconnected: eigenvalue 0 then
  has one eigenvector per component, known in closed form (``dd o 1_C`` normalised, ``e_i`` for an isolated row).  These
  are written from the component labels and locked; Lanczos runs in their orthogonal complement for the remaining
  ``n_components - c`` pairs.  The basis of the null space is therefore the components' own, in the order of their
  smallest row, where sklearn's is arbitrary;
* the start vector is counter-based, ``u01(mix64(row, seed)) - 1/2``, orthogonalised against the locked vectors; with the
  fixed summation orders of the kernels two runs agree bit for bit;
* stored diagonal entries and stored zeros are ignored; a row without neighbours has ``dd = 1`` as scipy's
  ``laplacian`` sets it;
* when ``n - c <= ncv`` the Krylov space is the whole complement: the solver stops after ``n - c`` steps (or at
  ``beta <= BREAKDOWN``) and the pairs are exact.

There is no CPU fallback: without the HIP library / a GPU every device function raises ``AvaHipError``.
"""
import ctypes
import numbers
import warnings

import numpy as np
import scipy.sparse
import torch

from . import _lib, _rows

__all__ = ["laplacian_eigenmaps", "connected_components", "SpectralEmbedding", "SpectralClustering",
           "SpectralConvergenceError", "MAX_BASIS", "DEFAULT_NCV", "BREAKDOWN"]
MAX_N = 2 ** 30             # ava_sp_max_n
MAX_BASIS = 1024            # ava_sp_max_basis: locked vectors + ncv + 1
DEFAULT_NCV = 64            # Lanczos vectors per restart cycle (the sweep: profiles/NOTES.md, the f27 entry)
BREAKDOWN = 1e-12           # a beta at or below this ends the Krylov space: |M| <= 1, so it is absolute
DEFAULT_MAXITER = 5000      # operator applications


class SpectralConvergenceError(RuntimeError):
    """the wanted pairs did not reach ``tol`` within ``maxiter`` operator applications"""


def _device():
    return _lib.device("spectral")


# ---- argument checks (no device) -------------------------------------------------------------------------------------
def _check_int(value, name, owner, lo=1):
    if not isinstance(value, numbers.Integral) or isinstance(value, bool) or value < lo:
        raise ValueError("The %r parameter of %s must be an int in the range [%d, inf). Got %r instead."
                         % (name, owner, lo, value))
    return int(value)


def _check_graph(graph):
    """a float64 CSR matrix with sorted indices and no stored zeros; sklearn's ``check_symmetric`` for the rest"""
    if scipy.sparse.issparse(graph):
        A = scipy.sparse.csr_matrix(graph, dtype=np.float64, copy=True)
    else:
        A = np.asarray(graph, dtype=np.float64)
        if A.ndim != 2:
            raise ValueError("array must be 2-dimensional and square. shape = %s" % (A.shape,))
        A = scipy.sparse.csr_matrix(A)
    if A.shape[0] != A.shape[1]:
        raise ValueError("array must be 2-dimensional and square. shape = %s" % (A.shape,))
    if A.shape[0] < 1 or A.shape[0] > MAX_N:
        raise ValueError("unsupported shape: %d rows, 1 to %d" % (A.shape[0], MAX_N))
    if not np.isfinite(A.data).all():
        raise ValueError("Input contains NaN or infinity.")
    A.sum_duplicates()
    diff = abs(A - A.T)
    if diff.nnz and diff.data.max() > 1e-10:
        warnings.warn("Array is not symmetric, and will be converted to symmetric by average with its transpose.",
                      stacklevel=3)
        A = scipy.sparse.csr_matrix(0.5 * (A + A.T))
    A.eliminate_zeros()
    A.sort_indices()
    return A


def _check_solver_args(n, n_components, tol, ncv, maxiter):
    n_components = _check_int(n_components, "n_components", "laplacian_eigenmaps")
    if n_components > n:
        raise ValueError("n_components = %d: the graph has only %d rows" % (n_components, n))
    if not (isinstance(tol, numbers.Real) and tol >= 0.0):
        raise ValueError("tol must be a non-negative number, got %r" % (tol,))
    if ncv is not None:
        ncv = _check_int(ncv, "ncv", "laplacian_eigenmaps")
    if maxiter is not None:
        maxiter = _check_int(maxiter, "maxiter", "laplacian_eigenmaps")
    return n_components, float(tol), ncv, maxiter


# ---- the graph on the device -----------------------------------------------------------------------------------------
class _Graph:
    """a checked CSR matrix on the device with its components, degrees and ``dd``"""

    def __init__(self, A, dev=None):
        self.dev = _device() if dev is None else dev
        self.lib = _lib.load()
        self.n, self.nnz = int(A.shape[0]), int(A.nnz)
        self.indptr = _rows.upload(A.indptr.astype(np.int64), self.dev)
        self.col = _rows.upload(A.indices.astype(np.int32), self.dev)
        self.val = _rows.upload(A.data.astype(np.float64), self.dev)
        self._ws = {}
        self.deg = torch.empty(self.n, dtype=torch.float64, device=self.dev)
        self.dd = torch.empty(self.n, dtype=torch.float64, device=self.dev)
        ws, nb = self.workspace(1)
        _lib.check(self.lib.ava_sp_degrees(self.indptr.data_ptr(), self.col.data_ptr(), self.val.data_ptr(), self.n,
                                           self.nnz, self.deg.data_ptr(), self.dd.data_ptr(), ws.data_ptr(), nb,
                                           _lib.stream()), "ava_sp_degrees")
        self._components = None

    def workspace(self, capacity):
        if capacity not in self._ws:
            nb = self.lib.ava_sp_workspace_bytes(self.n, int(capacity))
            self._ws = {capacity: (_lib.workspace(nb, self.dev, "n = %d rows, a basis of %d vectors"
                                                  % (self.n, capacity)), nb)}
        return self._ws[capacity]

    def components(self):
        """(count, labels int32 [n] on the device)"""
        if self._components is None:
            labels = torch.empty(self.n, dtype=torch.int32, device=self.dev)
            count = ctypes.c_int(0)
            ws, nb = self.workspace(1)
            _lib.check(self.lib.ava_sp_components(self.indptr.data_ptr(), self.col.data_ptr(), self.val.data_ptr(),
                                                  self.n, self.nnz, labels.data_ptr(), ctypes.byref(count),
                                                  ws.data_ptr(), nb, _lib.stream()), "ava_sp_components")
            self._components = (int(count.value), labels)
        return self._components

    def apply(self, x):
        """``M x`` for a float64 device vector"""
        y = torch.empty_like(x)
        ws, nb = self.workspace(1)
        _lib.check(self.lib.ava_sp_apply(self.indptr.data_ptr(), self.col.data_ptr(), self.val.data_ptr(),
                                         self.dd.data_ptr(), self.n, self.nnz, x.data_ptr(), y.data_ptr(),
                                         ws.data_ptr(), nb, _lib.stream()), "ava_sp_apply")
        return y


class _Basis:
    """the basis ``[capacity, n]`` of a solve, ``nlock`` locked vectors first, and the device tridiagonal"""

    def __init__(self, g, capacity, nlock):
        self.g, self.capacity, self.nlock = g, int(capacity), int(nlock)
        self.V = torch.zeros((self.capacity, g.n), dtype=torch.float64, device=g.dev)
        self.alpha = torch.zeros(self.capacity, dtype=torch.float64, device=g.dev)
        self.beta = torch.zeros(self.capacity, dtype=torch.float64, device=g.dev)
        self.ws, self.nb = g.workspace(self.capacity)

    def null_vectors(self, labels, k):
        g = self.g
        _lib.check(g.lib.ava_sp_null_vectors(labels.data_ptr(), g.dd.data_ptr(), g.n, int(k), self.V.data_ptr(),
                                             self.capacity, self.ws.data_ptr(), self.nb, _lib.stream()),
                   "ava_sp_null_vectors")

    def start(self, seed):
        """the start vector into slot ``nlock``; its length before normalisation"""
        g = self.g
        norm = torch.zeros(1, dtype=torch.float64, device=g.dev)
        _lib.check(g.lib.ava_sp_start(self.V.data_ptr(), g.n, self.capacity, self.nlock, int(seed) % 2 ** 64, BREAKDOWN,
                                      norm.data_ptr(), self.ws.data_ptr(), self.nb, _lib.stream()), "ava_sp_start")
        return float(norm.cpu()[0])

    def lanczos(self, j0, j1):
        g = self.g
        _lib.check(g.lib.ava_sp_lanczos(g.indptr.data_ptr(), g.col.data_ptr(), g.val.data_ptr(), g.dd.data_ptr(), g.n,
                                        g.nnz, self.V.data_ptr(), self.capacity, self.nlock, int(j0), int(j1),
                                        BREAKDOWN, self.alpha.data_ptr(), self.beta.data_ptr(), self.ws.data_ptr(),
                                        self.nb, _lib.stream()), "ava_sp_lanczos")

    def tridiagonal(self, m):
        """(alpha [m], beta [m]) on the host: waits for the device"""
        return self.alpha[:m].cpu().numpy(), self.beta[:m].cpu().numpy()

    def rotate(self, ncv, S):
        """active[:keep] <- active[:ncv] S for the host matrix ``S`` [ncv, keep]"""
        g = self.g
        S = np.ascontiguousarray(S, dtype=np.float64)
        Sd = _rows.upload(S, g.dev)
        active = self.V[self.nlock:]
        _lib.check(g.lib.ava_sp_rotate(active.data_ptr(), g.n, self.capacity - self.nlock, int(ncv), int(S.shape[1]),
                                       Sd.data_ptr(), self.ws.data_ptr(), self.nb, _lib.stream()), "ava_sp_rotate")

    def move(self, src, dst):
        """active[dst] <- active[src]"""
        self.V[self.nlock + dst].copy_(self.V[self.nlock + src])


def projected_matrix(theta, s, alpha, beta, k, m):
    """the ``m x m`` projection of M on a thick-restarted basis: ``diag(theta)`` and the arrow ``s`` for the ``k`` kept
    Ritz vectors, the tridiagonal ``alpha[k:m]``, ``beta[k:m - 1]`` after them"""
    T = np.zeros((m, m), dtype=np.float64)
    T[np.arange(k), np.arange(k)] = theta[:k]
    if k:
        T[k, :k] = s[:k]
        T[:k, k] = s[:k]
    idx = np.arange(k, m)
    T[idx, idx] = alpha[k:m]
    T[idx[:-1], idx[1:]] = beta[k:m - 1]
    T[idx[1:], idx[:-1]] = beta[k:m - 1]
    return T


def restart_size(m, nwant):
    """how many Ritz vectors a thick restart keeps: the wanted ones and half of the others"""
    return nwant + (m - nwant) // 2


def default_ncv(nwant):
    return max(DEFAULT_NCV, 2 * nwant + 1)


class _Solution:
    """``mu`` [k] descending (``lambda = 1 - mu``) and the device vectors ``x`` [k, n], unit eigenvectors of ``L_sym``:
    the locked null vectors first, in the order of their components; ``n_ops`` operator applications and ``n_restarts``"""

    def __init__(self, mu, x, n_comp, labels, n_ops, n_restarts, residuals):
        self.mu, self.x, self.n_comp, self.labels = mu, x, n_comp, labels
        self.n_ops, self.n_restarts, self.residuals = n_ops, n_restarts, residuals


def _solve(g, n_components, tol, ncv=None, seed=0, maxiter=None):
    n = g.n
    c, labels = g.components()
    k_null = min(c, n_components)
    nwant = n_components - k_null
    if nwant == 0:
        basis = _Basis(g, k_null, 0)
        basis.null_vectors(labels, k_null)
        return _Solution(np.ones(k_null), basis.V, c, labels, 0, 0, np.zeros(k_null))
    room = n - c                                   # the dimension of the complement of the null space; >= nwant
    ncv = default_ncv(nwant) if ncv is None else ncv
    if ncv < nwant + 2 and ncv < room:
        raise ValueError("ncv = %d must be at least n_components - components + 2 = %d" % (ncv, nwant + 2))
    m = min(ncv, room)
    if c + m + 1 > MAX_BASIS:
        raise ValueError("unsupported shape: %d components and ncv = %d need a basis of %d vectors, at most %d"
                         % (c, m, c + m + 1, MAX_BASIS))
    maxiter = DEFAULT_MAXITER if maxiter is None else maxiter
    basis = _Basis(g, c + m + 1, c)
    basis.null_vectors(labels, c)
    basis.start(seed)
    k, theta, s = 0, np.zeros(0), np.zeros(0)
    n_ops = n_restarts = 0
    while True:
        basis.lanczos(k, m)
        alpha, beta = basis.tridiagonal(m)
        n_ops += m - k
        broke = np.nonzero(beta[k:m] <= BREAKDOWN)[0]
        exact = m == room or len(broke) > 0
        me = k + int(broke[0]) + 1 if len(broke) else m
        mu, S = np.linalg.eigh(projected_matrix(theta, s, alpha, beta, k, me))
        order = np.argsort(-mu, kind="stable")
        if me < nwant:
            raise SpectralConvergenceError("the Krylov space of the start vector ended after %d vectors, %d pairs "
                                           "were wanted: try another seed" % (me, nwant))
        res = np.zeros(me) if exact else np.abs(beta[me - 1] * S[me - 1, order])
        if exact or bool((res[:nwant] <= tol).all()):
            basis.rotate(me, S[:, order[:nwant]])
            return _Solution(np.concatenate([np.ones(c), mu[order[:nwant]]]), basis.V[:c + nwant], c, labels, n_ops,
                             n_restarts,
                             np.concatenate([np.zeros(c), res[:nwant]]))
        if n_ops >= maxiter:
            raise SpectralConvergenceError("no convergence within %d operator applications: residuals %s, tol %g"
                                           % (n_ops, res[:nwant], tol))
        kk = restart_size(me, nwant)
        keep = order[:kk]
        basis.rotate(me, S[:, keep])
        basis.move(me, kk)
        theta, s, k = mu[keep], beta[me - 1] * S[me - 1, keep], kk
        n_restarts += 1


def _sign_flip(u):
    """sklearn's ``_deterministic_vector_sign_flip`` for vectors in rows: the entry of largest modulus is positive"""
    big = np.argmax(np.abs(u), axis=1)
    return u * np.sign(u[np.arange(u.shape[0]), big])[:, None]


# ---- public functions ------------------------------------------------------------------------------------------------
def connected_components(graph):
    """``(c, labels)`` of a symmetric sparse graph: int32 ``labels`` ``[n]``, the components numbered in the order of
    their smallest row, a function of the graph alone (scipy's ``connected_components`` numbers by traversal)"""
    A = _check_graph(graph)
    c, labels = _Graph(A).components()
    return c, labels.cpu().numpy()


def laplacian_eigenmaps(graph, n_components, *, tol=1e-10, ncv=None, seed=0, drop_first=True, maxiter=None):
    """``(eigenvalues [k], vectors [n, k])``, ``k = n_components``: the smallest eigenpairs of the normalised Laplacian of
    ``graph`` in sklearn's convention, ``u = x / dd`` for the unit eigenvector ``x`` of ``L_sym``, ascending eigenvalue,
    the sign by sklearn's ``_deterministic_vector_sign_flip``; with ``drop_first`` the first of ``n_components + 1``
    pairs is left out, as sklearn's ``spectral_embedding`` does.  A disconnected graph gives sklearn's warning and one
    eigenvalue 0 per component, whose vectors are the components' own.  ``tol`` bounds the residual ``|L x - lambda x|``;
    ``ncv`` is the number of Lanczos vectors of a restart cycle, ``maxiter`` the operator applications allowed
    (``SpectralConvergenceError`` beyond)."""
    A = _check_graph(graph)
    n_components, tol, ncv, maxiter = _check_solver_args(A.shape[0], n_components, tol, ncv, maxiter)
    k = n_components + (1 if drop_first else 0)
    if k > A.shape[0]:
        raise ValueError("n_components = %d with drop_first needs %d rows, the graph has %d"
                         % (n_components, k, A.shape[0]))
    g = _Graph(A)
    sol = _solve(g, k, tol, ncv, seed, maxiter)
    if sol.n_comp > 1:
        warnings.warn("Graph is not fully connected, spectral embedding may not work as expected.", stacklevel=2)
    u = _sign_flip((sol.x / g.dd[None, :]).cpu().numpy())
    lam = 1.0 - sol.mu
    lam[:min(sol.n_comp, k)] = 0.0
    first = 1 if drop_first else 0
    return lam[first:], np.ascontiguousarray(u[first:].T)


def _knn_affinity(X, n_neighbors):
    """sklearn's ``kneighbors_graph(X, n_neighbors, include_self=True)`` followed by ``0.5 (C + C^T)``: the table of
    ``projection.knn``, which holds the row itself"""
    from . import projection as _pj
    idx, _ = _pj.knn(X, n_neighbors)
    n = idx.shape[0]
    C = scipy.sparse.csr_matrix((np.ones(idx.size), (np.repeat(np.arange(n), idx.shape[1]), np.asarray(idx).ravel())),
                                shape=(n, n))
    A = scipy.sparse.csr_matrix(0.5 * (C + C.T))
    A.sort_indices()
    return A


def _check_affinity(est, owner):
    if est.affinity in ('rbf', 'precomputed_nearest_neighbors') or callable(est.affinity):
        raise NotImplementedError("affinity=%r is not on the device: 'nearest_neighbors' or 'precomputed'"
                                  % (est.affinity,))
    if est.affinity not in ('nearest_neighbors', 'precomputed'):
        raise ValueError("The 'affinity' parameter of %s must be a str among {'nearest_neighbors', 'precomputed'}. "
                         "Got %r instead." % (owner, est.affinity))
    if est.eigen_solver not in (None, 'arpack', 'device'):
        if est.eigen_solver in ('lobpcg', 'amg'):
            raise NotImplementedError("eigen_solver=%r is not on the device: the solver is thick-restart Lanczos"
                                      % (est.eigen_solver,))
        raise ValueError("The 'eigen_solver' parameter of %s must be a str among {'arpack', 'lobpcg', 'amg'} or None. "
                         "Got %r instead." % (owner, est.eigen_solver))


def _seed_of(random_state):
    """a start-vector seed from sklearn's ``random_state`` argument"""
    if random_state is None:
        return 0
    if isinstance(random_state, np.random.RandomState):
        return int(random_state.randint(2 ** 31 - 1))
    return _check_int(random_state, "random_state", "the estimator", lo=0)


def _affinity_of(est, X, n_neighbors):
    from . import projection as _pj
    if est.affinity == 'precomputed':
        return _check_graph(X)
    shape = tuple(X.shape)
    if len(shape) != 2:
        raise ValueError("Expected 2D array, got %dD array instead" % len(shape))
    if not 1 <= n_neighbors <= min(_pj.MAX_K, shape[0]):
        raise ValueError("Expected n_neighbors <= n_samples_fit and <= %d, but n_neighbors = %d, n_samples_fit = %d"
                         % (_pj.MAX_K, n_neighbors, shape[0]))
    return _knn_affinity(X, n_neighbors)


class SpectralEmbedding:
    """sklearn 1.7's ``SpectralEmbedding`` with the eigensolver on the device.  ``affinity`` is ``'nearest_neighbors'``
    (``n_neighbors`` defaults to ``max(n / 10, 1)``, at most ``projection.MAX_K``) or ``'precomputed'`` (any symmetric
    scipy sparse matrix, for example ``UMAP.graph_``).  After ``fit``: ``embedding_`` (float64 ``[n, n_components]``),
    ``affinity_matrix_``, ``eigenvalues_``, ``n_connected_components_``."""

    def __init__(self, n_components=2, *, affinity='nearest_neighbors', n_neighbors=None, random_state=None,
                 eigen_solver=None, tol=1e-10, ncv=None):
        self.n_components = n_components
        self.affinity = affinity
        self.n_neighbors = n_neighbors
        self.random_state = random_state
        self.eigen_solver = eigen_solver
        self.tol = tol
        self.ncv = ncv

    def fit(self, X, y=None):
        _check_int(self.n_components, "n_components", "SpectralEmbedding")
        if self.n_neighbors is not None:
            _check_int(self.n_neighbors, "n_neighbors", "SpectralEmbedding")
        _check_affinity(self, "SpectralEmbedding")
        seed = _seed_of(self.random_state)
        k = self.n_neighbors if self.n_neighbors is not None else max(int(X.shape[0] / 10), 1)
        self.affinity_matrix_ = _affinity_of(self, X, int(k))
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            lam, u = laplacian_eigenmaps(self.affinity_matrix_, self.n_components, tol=self.tol, ncv=self.ncv,
                                         seed=seed, drop_first=True)
        for wm in caught:
            warnings.warn(wm.message, wm.category, stacklevel=2)
        self.eigenvalues_, self.embedding_ = lam, u
        return self

    def fit_transform(self, X, y=None):
        return self.fit(X).embedding_


class SpectralClustering:
    """sklearn 1.7's ``SpectralClustering`` with ``assign_labels='kmeans'``: the first ``n_components`` (default
    ``n_clusters``) eigenvectors of the normalised Laplacian of the affinity graph, none dropped, clustered by
    ``kmeans.KMeans`` on the device.  Same two affinities as :class:`SpectralEmbedding`.  After ``fit``: ``labels_``
    (int32), ``affinity_matrix_``, ``embedding_`` (the rows k-means saw)."""

    def __init__(self, n_clusters=8, *, n_components=None, affinity='nearest_neighbors', n_neighbors=10, n_init=10,
                 random_state=None, eigen_solver=None, assign_labels='kmeans', tol=1e-10, ncv=None):
        self.n_clusters = n_clusters
        self.n_components = n_components
        self.affinity = affinity
        self.n_neighbors = n_neighbors
        self.n_init = n_init
        self.random_state = random_state
        self.eigen_solver = eigen_solver
        self.assign_labels = assign_labels
        self.tol = tol
        self.ncv = ncv

    def fit(self, X, y=None):
        from . import kmeans as _km
        k = _check_int(self.n_clusters, "n_clusters", "SpectralClustering")
        nc = k if self.n_components is None else _check_int(self.n_components, "n_components", "SpectralClustering")
        _check_int(self.n_neighbors, "n_neighbors", "SpectralClustering")
        n_init = _check_int(self.n_init, "n_init", "SpectralClustering")
        if self.assign_labels in ('discretize', 'cluster_qr'):
            raise NotImplementedError("assign_labels=%r is not on the device: 'kmeans'" % (self.assign_labels,))
        if self.assign_labels != 'kmeans':
            raise ValueError("The 'assign_labels' parameter of SpectralClustering must be a str among {'kmeans', "
                             "'discretize', 'cluster_qr'}. Got %r instead." % (self.assign_labels,))
        _check_affinity(self, "SpectralClustering")
        seed = _seed_of(self.random_state)
        self.affinity_matrix_ = _affinity_of(self, X, int(self.n_neighbors))
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _, u = laplacian_eigenmaps(self.affinity_matrix_, nc, tol=self.tol, ncv=self.ncv, seed=seed,
                                       drop_first=False)
        for wm in caught:
            warnings.warn(wm.message, wm.category, stacklevel=2)
        self.embedding_ = u
        km = _km.KMeans(k, n_init=n_init, random_state=seed).fit(u)
        self.labels_ = np.asarray(km.labels_)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


def umap_eigenvectors(graph, tol=1e-4, ncv=None, seed=0, maxiter=None):
    """for ``projection.init_embedding(..., eigen_solver='device')``: ``(c, vectors)`` with the eigenvectors 1 and 2 of
    ``L_sym`` (float64 ``[n, 2]``, not divided by ``dd``: umap's ``spectral_layout``), or ``(c, None)`` when the graph has
    ``c > 1`` components"""
    g = _Graph(_check_graph(graph))
    c, _ = g.components()
    if c > 1:
        return c, None
    sol = _solve(g, 3, float(tol), ncv, seed, maxiter)
    return c, np.ascontiguousarray(sol.x[1:3].cpu().numpy().T)
