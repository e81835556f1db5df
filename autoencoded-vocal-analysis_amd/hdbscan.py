"""Hierarchical density clustering (HDBSCAN) of latent rows on the MI355X.

The reference package has no counterpart: the specification is scikit-learn 1.7's ``sklearn/cluster/_hdbscan``
(``hdbscan.py``, ``_reachability.pyx``, ``_linkage.pyx``, ``_tree.pyx``), followed with ``csrc/hdbscan.hip``:

=========================================  ===================================  ======================
scikit-learn 1.7                           here                                 C entry point
=========================================  ===================================  ======================
``mutual_reachability_graph`` (the core    the k-th neighbour of                ``ava_pj_knn`` + ``ava_hd_core``,
distances)                                 ``projection``'s exact kNN           ``ava_hd_core_pre``
``mst_from_mutual_reachability`` /         :func:`mutual_reachability_mst`      ``ava_hd_mst``, ``ava_hd_mst_pre``
``mst_from_data_matrix`` (Prim)            (Boruvka rounds on the device)
``make_single_linkage`` ..                 the tree tail, on the host           ``ava_hd_tree``
``tree_to_labels``
``HDBSCAN``                                :class:`HDBSCAN`                     all of them
=========================================  ===================================  ======================

With ``m(i, j)`` the pair measure -- the direct-difference sum ``sum_c (x_c - y_c)^2`` of ``csrc/sqdist_tile.h`` in fp64
(no square root in any pass), or ``D[i, j]`` of a precomputed matrix --, ``core(i)`` the ``min_samples``-th smallest
``m(i, .)`` (the row itself first) and ``w(i, j) = max(core(i), core(j), m(i, j))``, the N^2 mutual-reachability graph is
never stored: every Boruvka round forms the pairs again, skipping every 64 x 64 tile that lies inside one component.

Deviations from scikit-learn, on purpose:

* **the edge order**: edges are compared by the key ``(w, m, min(i, j), max(i, j))``, a strict total order, so the
  spanning tree, and with it every label, is a function of the data alone.  sklearn resolves ties in ``w`` (which occur
  wherever two clusters meet at some row's core distance) by Prim's visiting order and an unstable argsort;
* **the numbering**: clusters are numbered in ascending order of their smallest row, as ``dbscan.DBSCAN`` does;
* merge distances are ``sqrt(w)`` (euclidean) or ``w`` (precomputed), correctly rounded, and ``lambda = 1 / distance``;
* ``alpha = 1``, ``allow_single_cluster = False``, ``cluster_selection_epsilon = 0``, ``max_cluster_size = None`` only:
  the constructor does not take these parameters;
* a ``'precomputed'`` matrix must be symmetric with a zero diagonal, as in ``dbscan``; no sparse input, no
  ``store_centers``, rows with NaN or infinity are refused;
* ``min_samples <= projection.MAX_K`` = 64 and at most ``MAX_N`` = 2^21 rows.

There is no CPU fallback: without the HIP library / a GPU every device function raises ``AvaHipError``.
"""
import ctypes
import numbers

import numpy as np
import torch

from . import _lib
from . import cluster_metrics as _cm
from . import projection as _pj

__all__ = ["HDBSCAN", "mutual_reachability_mst", "MAX_N"]
MAX_N = 2 ** 21
_KNN_CHUNK = 2 ** 17            # rows of one kNN call: the table of a call stays below 2^17 * 64 * 16 bytes
_METHODS = ('eom', 'leaf')


def _device():
    return _lib.device("HDBSCAN")


def _check_int(value, name, low, none_ok=False):
    if none_ok and value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < low:
        raise ValueError("The %r parameter of HDBSCAN must be an int in the range [%d, inf)%s. Got %r instead."
                         % (name, low, " or None" if none_ok else "", value))
    return int(value)


def _check_min_samples(min_samples, n):
    """sklearn's checks of the resolved min_samples against the rows, then this package's limit"""
    if n == 1:
        raise ValueError("n_samples=1 while HDBSCAN requires more than one sample")
    if min_samples > n:
        raise ValueError("min_samples (%d) must be at most the number of samples in X (%d)" % (min_samples, n))
    if min_samples > _pj.MAX_K:
        raise ValueError("min_samples (%d) must be at most %d (projection.MAX_K, the neighbours the kNN kernel keeps)"
                         % (min_samples, _pj.MAX_K))


def _core_device(Xd, min_samples, metric):
    """float64 [N] on the device: the core measures (squared for euclidean)"""
    lib = _lib.load()
    n = int(Xd.shape[0])
    core = torch.empty(n, dtype=torch.float64, device=Xd.device)
    code = _lib.dtype_code(Xd)
    if metric == 'precomputed':
        _lib.check(lib.ava_hd_core_pre(Xd.data_ptr(), code, n, min_samples, core.data_ptr(), _lib.stream()),
                   "ava_hd_core_pre")
        return core
    kth = torch.empty(n, dtype=torch.int64, device=Xd.device)
    for q0 in range(0, n, _KNN_CHUNK):
        q1 = min(q0 + _KNN_CHUNK, n)
        idx = torch.empty((q1 - q0, min_samples), dtype=torch.int64, device=Xd.device)
        dist = torch.empty((q1 - q0, min_samples), dtype=torch.float64, device=Xd.device)
        _lib.check(lib.ava_pj_knn(Xd.data_ptr(), code, n, int(Xd.shape[1]), min_samples, q0, q1 - q0,
                                  idx.data_ptr(), dist.data_ptr(), _lib.stream()), "ava_pj_knn")
        kth[q0:q1] = idx[:, min_samples - 1]
    _lib.check(lib.ava_hd_core(Xd.data_ptr(), code, n, int(Xd.shape[1]), kth.data_ptr(), core.data_ptr(),
                               _lib.stream()), "ava_hd_core")
    return core


def _mst_device(Xd, core, metric, timings=None):
    """the N - 1 tree edges sorted by the key, on the device: (i int64, j int64, w float64, m float64), and the number
    of Boruvka rounds; ``timings``, a list, receives the milliseconds of every round's row-minimum launch"""
    lib = _lib.load()
    n = int(Xd.shape[0])
    d = int(Xd.shape[1]) if metric == 'euclidean' else 1
    nbytes = lib.ava_hd_workspace_bytes(n, d)
    dev = Xd.device
    ws = _lib.workspace(nbytes, dev, "N = %d, d = %d" % (n, d))
    ei = torch.empty(n - 1, dtype=torch.int32, device=dev)
    ej = torch.empty(n - 1, dtype=torch.int32, device=dev)
    ew = torch.empty(n - 1, dtype=torch.float64, device=dev)
    em = torch.empty(n - 1, dtype=torch.float64, device=dev)
    rounds = ctypes.c_int(0)
    ms = (ctypes.c_float * max(1, lib.ava_hd_max_rounds(n)))()
    tail = (core.data_ptr(), ei.data_ptr(), ej.data_ptr(), ew.data_ptr(), em.data_ptr(), ctypes.addressof(rounds),
            ctypes.addressof(ms) if timings is not None else None, ws.data_ptr(), nbytes, _lib.stream())
    if metric == 'euclidean':
        _lib.check(lib.ava_hd_mst(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, *tail), "ava_hd_mst")
    else:
        _lib.check(lib.ava_hd_mst_pre(Xd.data_ptr(), _lib.dtype_code(Xd), n, *tail), "ava_hd_mst_pre")
    if timings is not None:
        timings.extend(float(ms[r]) for r in range(rounds.value))
    cols = [ew, em, ei.long(), ej.long()]
    for key in (3, 2, 1, 0):                                           # a lexsort: stable sorts, the last key first
        order = torch.sort(cols[key], stable=True)[1]
        cols = [c[order] for c in cols]
    ew, em, ei, ej = cols
    return ei, ej, ew, em, rounds.value


def _mst_host(Xd, min_samples, metric):
    """(mst float64 [N - 1, 3], core distances float64 [N], rounds) as numpy arrays; the square roots are numpy's"""
    core = _core_device(Xd, min_samples, metric)
    ei, ej, ew, _, rounds = _mst_device(Xd, core, metric)
    w, core = ew.cpu().numpy(), core.cpu().numpy()
    if metric == 'euclidean':
        w, core = np.sqrt(w), np.sqrt(core)
    mst = np.stack([ei.cpu().numpy().astype(np.float64), ej.cpu().numpy().astype(np.float64), w], axis=1)
    return mst, core, rounds


def _tree_host(mst, n, min_cluster_size, method):
    """``ava_hd_tree``: (labels int64 [N], probabilities float64 [N], n_clusters, linkage float64 [N - 1, 4])"""
    ei = np.ascontiguousarray(mst[:, 0], dtype=np.int64)
    ej = np.ascontiguousarray(mst[:, 1], dtype=np.int64)
    dist = np.ascontiguousarray(mst[:, 2], dtype=np.float64)
    labels = np.empty(n, dtype=np.int64)
    prob = np.empty(n, dtype=np.float64)
    linkage = np.empty((n - 1, 4), dtype=np.float64)
    count = ctypes.c_int(0)
    _lib.check(_lib.load().ava_hd_tree(ei.ctypes.data, ej.ctypes.data, dist.ctypes.data, n, min_cluster_size,
                                       _METHODS.index(method), labels.ctypes.data, prob.ctypes.data,
                                       ctypes.addressof(count), linkage.ctypes.data), "ava_hd_tree")
    return labels, prob, count.value, linkage


def mutual_reachability_mst(X, min_samples, metric='euclidean'):
    """The minimum spanning tree of the mutual-reachability graph under the key order of the module docstring, for
    single-linkage users: ``(mst, core_distances)``, ``mst`` float64 ``[N - 1, 3]`` with rows ``(i, j, distance)``,
    ``i < j``, in key order, and ``core_distances`` float64 ``[N]`` (both square-rooted for ``'euclidean'``).  ``X`` and
    ``metric`` as for :class:`HDBSCAN`; ``1 <= min_samples <= min(projection.MAX_K, N)``."""
    min_samples = _check_int(min_samples, "min_samples", 1)
    X = _cm._check_pair_rows(X, metric, MAX_N)
    _check_min_samples(min_samples, X.shape[0])
    mst, core, _ = _mst_host(_cm._upload_pair_rows(X, metric, _device()), min_samples, metric)
    return mst, core


class HDBSCAN:
    """scikit-learn 1.7's ``HDBSCAN`` on the device, for ``metric='euclidean'`` (``X`` is ``[N, d]`` rows) or
    ``'precomputed'`` (``X`` is a symmetric ``[N, N]`` matrix of distances with a zero diagonal); ``X`` is a numpy array
    or a tensor, on the host or the device, float32 or float64.  ``min_samples=None`` means ``min_cluster_size``.

    After ``fit``: ``labels_`` (int64 numpy, noise is -1, clusters in ascending order of their smallest row),
    ``probabilities_``, ``n_clusters_``, ``n_noise_``, ``mst_`` (float64 ``[N - 1, 3]``: ``i, j, distance`` in key
    order), ``single_linkage_tree_`` (scipy's ``[N - 1, 4]``), ``core_distances_`` (float64 ``[N]``),
    ``n_boruvka_rounds_`` and ``n_features_in_``.  Nothing changes from run to run (module docstring)."""

    def __init__(self, min_cluster_size=5, *, min_samples=None, metric='euclidean', cluster_selection_method='eom'):
        self.min_cluster_size = min_cluster_size
        self.min_samples = min_samples
        self.metric = metric
        self.cluster_selection_method = cluster_selection_method

    def fit(self, X, y=None):
        min_cluster_size = _check_int(self.min_cluster_size, "min_cluster_size", 2)
        min_samples = _check_int(self.min_samples, "min_samples", 1, none_ok=True)
        if self.cluster_selection_method not in _METHODS:
            raise ValueError("The 'cluster_selection_method' parameter of HDBSCAN must be a str among {'eom', 'leaf'}. "
                             "Got %r instead." % (self.cluster_selection_method,))
        X = _cm._check_pair_rows(X, self.metric, MAX_N)
        n = int(X.shape[0])
        min_samples = min_cluster_size if min_samples is None else min_samples
        _check_min_samples(min_samples, n)
        min_cluster_size = min(min_cluster_size, 2 ** 31 - 1)
        Xd = _cm._upload_pair_rows(X, self.metric, _device())
        mst, core, rounds = _mst_host(Xd, min_samples, self.metric)
        labels, prob, count, linkage = _tree_host(mst, n, min_cluster_size, self.cluster_selection_method)
        self.labels_ = labels
        self.probabilities_ = prob
        self.n_clusters_ = int(count)
        self.n_noise_ = int((labels == -1).sum())
        self.mst_ = mst
        self.single_linkage_tree_ = linkage
        self.core_distances_ = core
        self.n_boruvka_rounds_ = int(rounds)
        self.n_features_in_ = int(X.shape[1])
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
