"""Density clustering (DBSCAN) of latent rows on the MI355X.

The reference package has no counterpart: the specification is scikit-learn 1.7's sklearn/cluster/_dbscan.py and
_dbscan_inner.pyx, followed with the HIP kernels of ``csrc/dbscan.hip``:

=====================================  =====================================  ======================
scikit-learn 1.7                       here                                   C entry point
=====================================  =====================================  ======================
``radius_neighbors`` (the sizes)       :func:`neighbor_counts`                ``ava_db_counts``, ``ava_db_counts_pre``
``DBSCAN.fit`` / ``dbscan_inner``      :class:`DBSCAN`                        the counts, then ``ava_db_labels``,
                                                                              ``ava_db_labels_pre`` (= ``ava_db_union``
                                                                              + ``ava_db_assign``)
(none: one fit per radius)             :func:`dbscan_sweep`                   the same, up to ``MAX_EPS`` radii a pass
``NearestNeighbors.kneighbors``        :func:`k_distances`                    ``ava_pj_knn``
=====================================  =====================================  ======================

The labels are sklearn's exactly, on any input where no pair sits within rounding of the radius:

* row ``i`` is a core row when ``#{j : dist(i, j) <= eps} >= min_samples``, itself included;
* the clusters are the connected components of the core rows under ``dist <= eps``, numbered in ascending order of
  their smallest row;
* a non-core row with core rows within ``eps`` takes the smallest cluster number among them (``dbscan_inner`` expands
  the clusters in label order and never relabels a row);
* every other row is noise, ``-1``.

Deviations from scikit-learn, on purpose:

* all arithmetic is fp64, also for float32 ``X``, and a euclidean pair is within ``eps`` when its direct-difference sum
  ``sum_c (x_c - y_c)^2`` (the tile of ``csrc/sqdist_tile.h``) is ``<= eps * eps``: no square root, no
  ``|x|^2 + |y|^2 - 2 x.y`` expansion, so duplicate rows are at distance exactly 0;
* a ``'precomputed'`` matrix must be symmetric (``ValueError`` otherwise; sklearn accepts it and returns something that
  depends on the row order) and, as in ``cluster_metrics``, have a zero diagonal;
* no ``sample_weight``, no sparse input, no ``algorithm`` / ``leaf_size`` / ``p`` / ``n_jobs``: the neighbourhoods are
  never materialised, every pass forms the pairs' distances again (three passes of N^2 / 2 pairs);
* at most ``MAX_N`` = 2^21 rows.

``metric`` is ``'euclidean'`` or ``'precomputed'``; any other raises ``NotImplementedError``.  There is no CPU fallback:
without the HIP library / a GPU every device function raises ``AvaHipError``.
"""
import numbers

import numpy as np
import torch

from . import _lib, _rows
from . import cluster_metrics as _cm
from . import projection as _pj

__all__ = ["DBSCAN", "neighbor_counts", "dbscan_sweep", "k_distances", "MAX_EPS", "MAX_N"]
MAX_EPS = 8                     # ava_db_max_eps: radii that share one distance pass
MAX_N = 2 ** 21                 # rows (the list of the upper triangle's tiles stays below 2^31)


def _device():
    return _lib.device("DBSCAN")


def _check_eps(eps):
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not eps > 0 or not np.isfinite(eps):
        raise ValueError("The 'eps' parameter of DBSCAN must be a float in the range (0.0, inf). Got %r instead."
                         % (eps,))
    return float(eps)


def _check_min_samples(min_samples):
    if isinstance(min_samples, bool) or not isinstance(min_samples, numbers.Integral) or min_samples < 1:
        raise ValueError("The 'min_samples' parameter of DBSCAN must be an int in the range [1, inf). Got %r instead."
                         % (min_samples,))
    return min(int(min_samples), 2 ** 31 - 1)


def _eps_list(eps_list):
    if isinstance(eps_list, (numbers.Real, str)) or eps_list is None or np.ndim(eps_list) == 0:
        raise ValueError("eps_list must be a sequence of radii, got %r" % (eps_list,))
    radii = [_check_eps(e.item() if isinstance(e, np.generic) else e) for e in eps_list]
    if not radii:
        raise ValueError("eps_list is empty")
    return radii


def _device_rows(X, metric):
    """the checks that need no device, then the rows on the device"""
    return _cm._upload_pair_rows(_cm._check_pair_rows(X, metric, MAX_N), metric, _device())


def _counts_group(Xd, radii, metric):
    """int32 [len(radii), N] on the device; len(radii) <= MAX_EPS"""
    lib = _lib.load()
    n = Xd.shape[0]
    eps = np.asarray(radii, dtype=np.float64)
    counts = torch.empty((len(radii), n), dtype=torch.int32, device=Xd.device)
    code = _lib.dtype_code(Xd)
    if metric == 'euclidean':
        _lib.check(lib.ava_db_counts(Xd.data_ptr(), code, n, Xd.shape[1], eps.ctypes.data, len(radii),
                                     counts.data_ptr(), _lib.stream()), "ava_db_counts")
    else:
        _lib.check(lib.ava_db_counts_pre(Xd.data_ptr(), code, n, eps.ctypes.data, len(radii), counts.data_ptr(),
                                         _lib.stream()), "ava_db_counts_pre")
    return counts


def _labels_group(Xd, radii, min_samples, metric):
    """(labels int64 [E, N], core bool [E, N], n_clusters int32 [E]) on the device; E = len(radii) <= MAX_EPS"""
    lib = _lib.load()
    n, e = Xd.shape[0], len(radii)
    d = Xd.shape[1] if metric == 'euclidean' else 1
    nbytes = lib.ava_db_workspace_bytes(n, d, e)
    ws = _lib.workspace(nbytes, Xd.device, "N = %d, d = %d, %d radii" % (n, d, e))       # raises before any launch
    counts = _counts_group(Xd, radii, metric)
    eps = np.asarray(radii, dtype=np.float64)
    labels = torch.empty((e, n), dtype=torch.int64, device=Xd.device)
    core = torch.empty((e, n), dtype=torch.uint8, device=Xd.device)
    ncl = torch.empty(e, dtype=torch.int32, device=Xd.device)
    tail = (eps.ctypes.data, e, min_samples, counts.data_ptr(), core.data_ptr(), labels.data_ptr(), ncl.data_ptr(),
            ws.data_ptr(), nbytes, _lib.stream())
    if metric == 'euclidean':
        _lib.check(lib.ava_db_labels(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, *tail), "ava_db_labels")
    else:
        _lib.check(lib.ava_db_labels_pre(Xd.data_ptr(), _lib.dtype_code(Xd), n, *tail), "ava_db_labels_pre")
    return labels, core.bool(), ncl


def _sweep_device(Xd, radii, min_samples, metric):
    """all radii in groups of MAX_EPS: (labels [E, N], core [E, N], n_clusters [E]) as numpy arrays"""
    parts = [_labels_group(Xd, radii[g:g + MAX_EPS], min_samples, metric) for g in range(0, len(radii), MAX_EPS)]
    labels, core, ncl = (torch.cat([p[i] for p in parts]).cpu().numpy() for i in range(3))
    return labels, core, ncl.astype(np.int64)


def neighbor_counts(X, eps, metric='euclidean'):
    """The number of rows within ``eps`` of every row, itself included: int64 ``[N]``, or ``[E, N]`` for a sequence of
    ``E`` radii (which share the distance passes in groups of ``MAX_EPS``).  ``X`` as for :class:`DBSCAN`."""
    single = isinstance(eps, numbers.Real) or (isinstance(eps, np.ndarray) and eps.ndim == 0)
    radii = [_check_eps(float(eps) if isinstance(eps, np.ndarray) else eps)] if single else _eps_list(eps)
    Xd = _device_rows(X, metric)
    if _lib.load().ava_db_workspace_bytes(Xd.shape[0], Xd.shape[1] if metric == 'euclidean' else 1, 1) == 0:
        raise ValueError("unsupported shape %s" % (tuple(Xd.shape),))
    parts = [_counts_group(Xd, radii[g:g + MAX_EPS], metric) for g in range(0, len(radii), MAX_EPS)]
    counts = torch.cat(parts).cpu().numpy().astype(np.int64)
    return counts[0] if single else counts


class DBSCAN:
    """scikit-learn 1.7's ``DBSCAN`` on the device, for ``metric='euclidean'`` (``X`` is ``[N, d]`` rows) or
    ``'precomputed'`` (``X`` is a symmetric ``[N, N]`` matrix of distances); ``X`` is a numpy array or a tensor, on the
    host or the device, float32 or float64.

    After ``fit``: ``labels_`` (int64 numpy, noise is -1), ``core_sample_indices_`` (int64, ascending),
    ``components_`` (a copy of the core rows, shape ``(0, d)`` without any), ``n_clusters_`` and ``n_noise_``.  The
    labels are sklearn's (module docstring) and do not change from run to run."""

    def __init__(self, eps=0.5, *, min_samples=5, metric='euclidean'):
        self.eps = eps
        self.min_samples = min_samples
        self.metric = metric

    def fit(self, X, y=None):
        eps, min_samples = _check_eps(self.eps), _check_min_samples(self.min_samples)
        Xd = _device_rows(X, self.metric)
        labels, core, ncl = _sweep_device(Xd, [eps], min_samples, self.metric)
        self.labels_ = labels[0]
        self.core_sample_indices_ = np.flatnonzero(core[0]).astype(np.int64)
        self.components_ = Xd[torch.from_numpy(self.core_sample_indices_).to(Xd.device)].cpu().numpy()
        self.n_clusters_ = int(ncl[0])
        self.n_noise_ = int((labels[0] == -1).sum())
        self.n_features_in_ = int(Xd.shape[1])
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


def _sweep_silhouette(Xd, labels, ncl, metric):
    """``cluster_metrics.silhouette_score`` of the rows that are not noise, per radius; NaN where it is undefined"""
    out = np.full(len(labels), np.nan)
    for e, lab in enumerate(labels):
        keep = lab != -1
        if not 2 <= ncl[e] <= _cm.MAX_K or ncl[e] >= int(keep.sum()):
            continue
        rows = torch.from_numpy(np.flatnonzero(keep)).to(Xd.device)
        sub = Xd[rows][:, rows] if metric == 'precomputed' else Xd[rows]
        out[e] = _cm.silhouette_score(sub, lab[keep], metric=metric)
    return out


def dbscan_sweep(X, eps_list, min_samples=5, metric='euclidean', scores=False):
    """One DBSCAN per radius of ``eps_list`` on rows uploaded once; every distance pass serves up to ``MAX_EPS`` radii,
    and any number of radii is taken in such groups.  Returns a dict of numpy arrays: ``'eps'`` float64 ``[E]``,
    ``'labels'`` int64 ``[E, N]`` (row ``e`` equals ``DBSCAN(eps_list[e], ...).fit(X).labels_``), ``'n_clusters'`` and
    ``'n_noise'`` int64 ``[E]``, ``'core'`` bool ``[E, N]``; with ``scores=True`` also ``'silhouette'`` float64 ``[E]``:
    ``cluster_metrics.silhouette_score`` of the non-noise rows under their labels, NaN when fewer than 2 clusters remain,
    when there are more than ``cluster_metrics.MAX_K`` or when every remaining row is alone in its cluster."""
    radii = _eps_list(eps_list)
    min_samples = _check_min_samples(min_samples)
    Xd = _device_rows(X, metric)
    labels, core, ncl = _sweep_device(Xd, radii, min_samples, metric)
    out = {'eps': np.asarray(radii, dtype=np.float64), 'labels': labels, 'n_clusters': ncl,
           'n_noise': (labels == -1).sum(axis=1).astype(np.int64), 'core': core}
    if scores:
        out['silhouette'] = _sweep_silhouette(Xd, labels, ncl, metric)
    return out


def k_distances(X, k):
    """The distance from every row to its ``k``-th nearest row, counting itself as the first, sorted ascending: float64
    ``[N]``, the usual elbow plot for choosing ``eps`` at ``min_samples = k``.  From the exact kNN of ``projection``
    (the same distance tile, then one fp64 square root); ``1 <= k <= min(projection.MAX_K, N)``."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral):
        raise ValueError("k must be an integer, got %r" % (k,))
    X = _cm._check_rows(X)
    if not 1 <= k <= min(_pj.MAX_K, X.shape[0]):
        raise ValueError("k must be in [1, min(%d, n)], got %d" % (_pj.MAX_K, k))
    Xd = _rows.upload(X, _device())
    dist = _pj._knn_device(Xd, int(k))[1]
    return torch.sort(dist[:, int(k) - 1].contiguous())[0].cpu().numpy()
