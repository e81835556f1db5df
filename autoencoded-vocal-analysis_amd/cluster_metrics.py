"""Silhouette, Calinski-Harabasz and Davies-Bouldin scores of labelled latent rows on the MI355X (SURVEY.md section 8,
row f21).

The reference package has no counterpart: the specification is scikit-learn 1.7's
sklearn/metrics/cluster/_unsupervised.py, followed with the HIP kernels of ``csrc/silhouette.hip``:

=====================================  =====================================  ======================
scikit-learn 1.7                       here                                   C entry point
=====================================  =====================================  ======================
``_silhouette_reduce`` (the sums)      :func:`cluster_sums`                   ``ava_sil_cluster_sums``,
                                                                              ``ava_sil_cluster_sums_pre``
``silhouette_samples``                 :func:`silhouette_samples`             the sums, then ``ava_sil_finish``
``silhouette_score``                   :func:`silhouette_score`               ``ava_sil_finish`` (the mean)
``calinski_harabasz_score``            :func:`calinski_harabasz_score`        ``ava_gm_onehot``, ``ava_gm_means``,
``davies_bouldin_score``               :func:`davies_bouldin_score`           ``ava_sil_centroid_stats``
(none)                                 :func:`select_n_components`            ``mixture.GaussianMixture`` + the above
=====================================  =====================================  ======================

Deviations from scikit-learn, on purpose:

* all arithmetic is fp64, also for float32 ``X`` (sklearn stays in float32 then);
* euclidean distances are direct differences ``sqrt(sum_c (x_c - y_c)^2)`` (the tile of ``csrc/sqdist_tile.h``), where
  sklearn expands ``|x|^2 + |y|^2 - 2 x.y``, which cancels for near rows: duplicate rows are at distance exactly 0 here,
  so a row with ``a = b = 0`` scores 0, where sklearn's rounding noise can give +-1;
* every sum runs in this project's fixed orders (the contract at the head of ``csrc/silhouette.hip``): the same inputs
  give the same bits on every run, for float32 rows and their float64 copies, and under any relabelling of the clusters;
* the cluster means of the two centroid scores are those of ``mixture.m_step`` for one-hot responsibilities (sums over
  2048-row chunks, divided by ``n_k + 10 eps``), and the overall mean of Calinski-Harabasz is their weighted mean; so
  clusters of identical rows leave a within-cluster sum of a few ulp, not 0, and Calinski-Harabasz is then huge where
  sklearn returns its conventional 1.0;
* the centroid scores hold ``d <= mixture.MAX_D`` features and ``mixture.MAX_K`` labels, the silhouette ``MAX_K`` labels
  (sklearn: up to ``n - 1``); more raise ``ValueError``.

``metric`` is ``'euclidean'`` or ``'precomputed'``; any other raises ``NotImplementedError``.  There is no CPU fallback:
without the HIP library / a GPU every device function raises ``AvaHipError``.
"""
import numpy as np
import torch

from . import _lib, _rows
from . import mixture as _mx
from . import projection as _pj

__all__ = ["silhouette_samples", "silhouette_score", "calinski_harabasz_score", "davies_bouldin_score", "cluster_sums",
           "select_n_components", "MAX_K", "CHUNK_COLS"]
MAX_K = 1024                    # ava_sil_max_k
CHUNK_COLS = 2048               # ava_sil_chunk_cols: columns of a chunk of a cluster's sum
_DIAGONAL = ("The precomputed distance matrix contains non-zero elements on the diagonal. Use np.fill_diagonal(X, 0).")
_CRITERIA = ('bic', 'aic', 'silhouette', 'calinski_harabasz', 'davies_bouldin')


def _device():
    return _lib.device("cluster-metric")


def _check_metric(metric):
    if metric not in ('euclidean', 'precomputed'):
        raise NotImplementedError("metric=%r: only 'euclidean' and 'precomputed' are on the device" % (metric,))


def _check_rows(X, metric='euclidean'):
    """sklearn's check_X_y for the rows, on the host or the device; returns float32 or float64 rows as they are"""
    X = _rows.native(X)
    shape = tuple(X.shape)
    if len(shape) != 2:
        raise ValueError("Expected 2D array, got %dD array instead" % len(shape))
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError("Found array with %d sample(s) and %d feature(s) while a minimum of 1 is required"
                         % (shape[0], shape[1]))
    if shape[0] > 2 ** 30:
        raise ValueError("at most 2**30 rows")
    if _rows.has_nan(X):
        raise ValueError("Input X contains NaN.")
    if not _rows.is_finite(X):
        raise ValueError("Input X contains infinity or a value too large for dtype('float64').")
    if metric == 'precomputed':
        if shape[0] != shape[1]:
            raise ValueError("Precomputed metric requires a square distance matrix, got shape %s" % (shape,))
        single = X.dtype == (torch.float32 if torch.is_tensor(X) else np.float32)
        atol = 100.0 * float(np.finfo(np.float32 if single else np.float64).eps)      # sklearn's _atol_for_type
        diag = torch.diagonal(X).abs().max() if torch.is_tensor(X) else np.abs(np.diagonal(X)).max()
        if float(diag) > atol:
            raise ValueError(_DIAGONAL)
    return X


def _check_pair_rows(X, metric, max_n):
    """the host checks that ``dbscan`` and ``hdbscan`` share: the metric, the rows, and the shape their tile walks hold"""
    _check_metric(metric)
    X = _check_rows(X, metric)
    if X.shape[0] > max_n:
        raise ValueError("unsupported shape: N = %d rows, at most %d" % (X.shape[0], max_n))
    if metric == 'euclidean' and X.shape[1] > _pj.MAX_DIM:
        raise ValueError("unsupported shape: d = %d features, at most %d" % (X.shape[1], _pj.MAX_DIM))
    return X


def _upload_pair_rows(X, metric, dev):
    """checked rows on the device; a precomputed matrix must be symmetric (its tiles are formed above the diagonal)"""
    Xd = _rows.upload(X, dev)
    if metric == 'precomputed' and not bool((Xd == Xd.T).all()):
        raise ValueError("The precomputed distance matrix must be symmetric")
    return Xd


def _encode(labels, n, max_k=None):
    """sklearn's LabelEncoder and check_number_of_labels: (encoded labels int64 [n], number of labels)"""
    if torch.is_tensor(labels):
        labels = labels.cpu().numpy()
    labels = np.asarray(labels)
    if labels.ndim == 2 and labels.shape[1] == 1:                      # a column vector, as sklearn's column_or_1d
        labels = labels.reshape(-1)
    if labels.ndim != 1:
        raise ValueError("y should be a 1d array, got an array of shape %s instead." % (labels.shape,))
    if len(labels) != n:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (n, len(labels)))
    if labels.dtype.kind not in "iubUSO":
        raise ValueError("labels must be integers or strings, got dtype %s" % labels.dtype)
    classes, enc = np.unique(labels, return_inverse=True)
    k = len(classes)
    if not 1 < k < n:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % k)
    if max_k is not None and k > max_k:
        raise ValueError("Number of labels is %d: the device path holds at most %d" % (k, max_k))
    return enc.astype(np.int64).reshape(-1), k


def _tables(enc, k):
    """the stable argsort of the encoded labels and the clusters' first sorted rows"""
    order = np.argsort(enc, kind='stable').astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.bincount(enc, minlength=k))]).astype(np.int64)
    return order, off


def _workspace(n, d, k, dev):
    nbytes = _lib.load().ava_sil_workspace_bytes(n, d, k)
    return _lib.workspace(nbytes, dev, "N = %d, d = %d, %d labels" % (n, d, k)), nbytes


def _sums(Xd, order, off, k, metric):
    """S [n][k] in sorted-row order (device), and the workspace"""
    lib = _lib.load()
    n = Xd.shape[0]
    d = Xd.shape[1] if metric == 'euclidean' else 1
    ws, nbytes = _workspace(n, d, k, Xd.device)                       # raises before any launch
    S = torch.empty((n, k), dtype=torch.float64, device=Xd.device)
    code = _lib.dtype_code(Xd)
    if metric == 'euclidean':
        _lib.check(lib.ava_sil_cluster_sums(Xd.data_ptr(), code, n, d, k, order.data_ptr(), off.data_ptr(), S.data_ptr(),
                                            ws.data_ptr(), nbytes, _lib.stream()), "ava_sil_cluster_sums")
    else:
        _lib.check(lib.ava_sil_cluster_sums_pre(Xd.data_ptr(), code, n, k, order.data_ptr(), off.data_ptr(),
                                                S.data_ptr(), _lib.stream()), "ava_sil_cluster_sums_pre")
    return S, (ws, nbytes)


def _prepare(X, labels, metric):
    _check_metric(metric)
    X = _check_rows(X, metric)
    enc, k = _encode(labels, X.shape[0], MAX_K)
    order, off = _tables(enc, k)
    dev = _device()
    Xd = _rows.upload(X, dev)
    return Xd, torch.from_numpy(order).to(dev), torch.from_numpy(off).to(dev), k


def cluster_sums(X, labels, metric='euclidean'):
    """``S [N, K]`` float64 (numpy), rows in the caller's order, columns in the order of the sorted unique labels:
    ``S[i, k]`` is the sum of the distances from row ``i`` to the rows of cluster ``k`` (itself included, at 0)."""
    Xd, order, off, k = _prepare(X, labels, metric)
    S = _sums(Xd, order, off, k, metric)[0]
    out = torch.empty_like(S)
    out[order] = S
    return out.cpu().numpy()


def _silhouette(X, labels, metric):
    Xd, order, off, k = _prepare(X, labels, metric)
    n = Xd.shape[0]
    S, (ws, nbytes) = _sums(Xd, order, off, k, metric)
    out = torch.empty((4, n), dtype=torch.float64, device=Xd.device)
    _lib.check(_lib.load().ava_sil_finish(S.data_ptr(), n, k, order.data_ptr(), off.data_ptr(), out[0].data_ptr(),
                                          out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(),
                                          nbytes, _lib.stream()), "ava_sil_finish")
    return out


def silhouette_samples(X, labels, *, metric='euclidean', return_parts=False):
    """sklearn's ``silhouette_samples``: the coefficient of every row, float64 numpy.  ``X`` is ``[N, d]`` rows
    (``'euclidean'``) or an ``[N, N]`` matrix of distances (``'precomputed'``), numpy or tensor, on the host or the
    device, float32 or float64; ``labels`` any integer or string array.  ``return_parts=True`` returns ``(s, a, b)``:
    the mean distance to the row's own cluster (NaN for a cluster of one row) and to the nearest other cluster."""
    out = _silhouette(X, labels, metric).cpu().numpy()
    return (out[0], out[1], out[2]) if return_parts else out[0]


def _subsample_indices(n, sample_size, random_state):
    """sklearn's draw: ``check_random_state(random_state).permutation(n)[:sample_size]``"""
    if int(sample_size) != sample_size or sample_size < 1:
        raise ValueError("sample_size must be a positive integer, got %r" % (sample_size,))
    return _mx._random_state(random_state).permutation(n)[:int(sample_size)]


def silhouette_score(X, labels, *, metric='euclidean', sample_size=None, random_state=None):
    """sklearn's ``silhouette_score``: the mean coefficient, taken on the device over 2048-row chunks added ascending.
    ``sample_size`` subsamples exactly as sklearn does (both axes of a ``'precomputed'`` matrix)."""
    _check_metric(metric)
    if sample_size is not None:
        X = _check_rows(X, metric)
        if torch.is_tensor(labels):
            labels = labels.cpu().numpy()
        labels = np.asarray(labels).reshape(-1)
        if len(labels) != X.shape[0]:
            raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]"
                             % (X.shape[0], len(labels)))
        idx = _subsample_indices(X.shape[0], sample_size, random_state)
        rows = torch.as_tensor(idx, device=X.device) if torch.is_tensor(X) else idx
        X = X[rows][:, rows] if metric == 'precomputed' else X[rows]
        labels = labels[idx]
    return float(_silhouette(X, labels, metric)[3, 0].item())


def _centroid_stats(X, labels):
    """(cluster sizes, means [K, d], sum ||x - c||, sum ||x - c||^2) as float64 numpy arrays"""
    X = _check_rows(X)
    n, d = X.shape
    enc, k = _encode(labels, n)
    if d > _mx.MAX_D or k > _mx.MAX_K:
        raise ValueError("d = %d features, %d labels: the centroid scores hold at most %d and %d"
                         % (d, k, _mx.MAX_D, _mx.MAX_K))
    lib = _lib.load()
    dev = _device()
    Xd = _rows.upload(X, dev)
    lab = torch.from_numpy(enc).to(dev)
    ws, nbytes = _workspace(n, d, k, dev)
    gws, gbytes = _mx._workspace(n, d, k, 1, dev)
    prev = torch.full((n,), -1, dtype=torch.int64, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    resp = torch.empty((n, k), dtype=torch.float64, device=dev)
    out = torch.empty((4, k), dtype=torch.float64, device=dev)       # weights, nk, sum of distances, of their squares
    means = torch.empty((k, d), dtype=torch.float64, device=dev)
    st = _lib.stream()
    _lib.check(lib.ava_gm_onehot(lab.data_ptr(), prev.data_ptr(), n, k, resp.data_ptr(), changed.data_ptr(), st),
               "ava_gm_onehot")
    _lib.check(lib.ava_gm_means(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, resp.data_ptr(), out[0].data_ptr(),
                                means.data_ptr(), out[1].data_ptr(), gws.data_ptr(), gbytes, st), "ava_gm_means")
    _lib.check(lib.ava_sil_centroid_stats(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, lab.data_ptr(), means.data_ptr(),
                                          out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), nbytes, st),
               "ava_sil_centroid_stats")
    host = out.cpu().numpy()
    return np.bincount(enc, minlength=k).astype(np.float64), means.cpu().numpy(), host[2], host[3]


def _ch_from_stats(sizes, means, sum_sq):
    """sklearn's formula from the device sums, on the host in fp64"""
    n, k = sizes.sum(), len(sizes)
    mean = np.cumsum(sizes[:, None] * means, axis=0)[-1] / n          # ascending over the clusters
    extra = float(np.cumsum(sizes * np.cumsum((means - mean) ** 2, axis=1)[:, -1])[-1])
    intra = float(np.cumsum(sum_sq)[-1])
    return 1.0 if intra == 0.0 else extra * (n - k) / (intra * (k - 1.0))


def _db_from_stats(sizes, means, sum_dist):
    intra = sum_dist / sizes
    diff = means[:, None, :] - means[None, :, :]
    cd = np.sqrt(np.cumsum(diff * diff, axis=2)[:, :, -1])            # direct differences, features ascending
    if np.allclose(intra, 0) or np.allclose(cd, 0):
        return 0.0
    cd[cd == 0] = np.inf
    scores = np.max((intra[:, None] + intra) / cd, axis=1)
    return float(np.cumsum(scores)[-1] / len(sizes))


def calinski_harabasz_score(X, labels):
    """sklearn's ``calinski_harabasz_score`` (the variance ratio criterion) from the device's centroid sums"""
    sizes, means, _, sum_sq = _centroid_stats(X, labels)
    return _ch_from_stats(sizes, means, sum_sq)


def davies_bouldin_score(X, labels):
    """sklearn's ``davies_bouldin_score`` from the device's centroid sums"""
    sizes, means, sum_dist, _ = _centroid_stats(X, labels)
    return _db_from_stats(sizes, means, sum_dist)


def select_n_components(X, n_components, *, covariance_type='full', criteria=_CRITERIA, **gmm_kwargs):
    """One :class:`mixture.GaussianMixture` fit per entry of ``n_components`` on rows uploaded once, scored by
    ``criteria`` (any of ``'bic'``, ``'aic'``, ``'silhouette'``, ``'calinski_harabasz'``, ``'davies_bouldin'``) on the
    labels of ``predict``.  Returns a dict of arrays with one row per entry: ``'n_components'``, one float64 array per
    criterion and ``'labels'`` (int64 ``[len(n_components), N]``).  Where a fit leaves a single non-empty cluster the
    three geometric scores are NaN (they are undefined there; sklearn raises)."""
    counts = [int(c) for c in np.asarray(n_components).reshape(-1)]
    criteria = tuple(criteria)
    for c in criteria:
        if c not in _CRITERIA:
            raise ValueError("criteria must be among %s, got %r" % (_CRITERIA, c))
    if not counts:
        raise ValueError("n_components is empty")
    X = _mx._check_rows(X, max(counts))
    models = [_mx.GaussianMixture(c, covariance_type=covariance_type, **gmm_kwargs) for c in counts]
    Xd = _rows.upload(X, _device())
    out = {c: np.full(len(counts), np.nan) for c in criteria}
    labels = np.empty((len(counts), Xd.shape[0]), dtype=np.int64)
    for i, g in enumerate(models):
        g.fit(Xd)
        labels[i] = g.predict(Xd)
        several = len(np.unique(labels[i])) > 1
        stats = None                                                   # one centroid pass serves both centroid scores
        if several and ('calinski_harabasz' in criteria or 'davies_bouldin' in criteria):
            stats = _centroid_stats(Xd, labels[i])
        for c in criteria:
            if c in ('bic', 'aic'):
                out[c][i] = getattr(g, c)(Xd)
            elif not several:
                continue
            elif c == 'silhouette':
                out[c][i] = silhouette_score(Xd, labels[i])
            elif c == 'calinski_harabasz':
                out[c][i] = _ch_from_stats(stats[0], stats[1], stats[3])
            else:
                out[c][i] = _db_from_stats(stats[0], stats[1], stats[2])
    out['n_components'] = np.asarray(counts, dtype=np.int64)
    out['labels'] = labels
    return out
