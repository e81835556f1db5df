"""Cross-validated k-nearest-neighbour prediction from latent rows on the MI355X: do the
latent features carry the information?  Held-out R^2 of acoustic features predicted from the k nearest latent neighbours
(Goffinet et al. 2021, figures 2 and 3) and k-nearest-neighbour classification of strain, individual or social context
under cross-validation (its tables).

The reference package has no counterpart: the specification is scikit-learn 1.7's ``sklearn/neighbors``
(``_classification.py``, ``_regression.py``, ``_base.py::_get_weights``) under ``cross_val_predict`` /
``cross_val_score`` with a ``PredefinedSplit``, followed with ``csrc/knn_predict.hip``:

=========================================  ===================================  ======================
scikit-learn 1.7                           here                                 C entry point
=========================================  ===================================  ======================
one ``fit`` + ``kneighbors`` per fold      :func:`masked_kneighbors`: one pass  ``ava_kp_knn_masked``
                                           over all rows with a fold mask
``KNeighborsClassifier.predict``           the vote at every k of a sweep       ``ava_kp_vote``
``KNeighborsClassifier.predict_proba``     :meth:`KNeighborsClassifier          ``ava_kp_proba``
                                           .predict_proba`
``KNeighborsRegressor.predict``            the weighted mean at every k         ``ava_kp_regress``
``cross_val_predict(.., PredefinedSplit)``  :func:`cross_val_predict`            the three above
``cross_val_score(.., PredefinedSplit)``   :func:`cross_val_score`              (torch reductions)
``KFold(n_splits)`` (no shuffling)         :func:`kfold`                        --
``LeaveOneGroupOut``                       :func:`group_folds`                  --
``kneighbors(X)`` on new rows              ``projection``'s query kernel        ``ava_pj_knn_query``
=========================================  ===================================  ======================

Every pair of rows has the same distance bits in every kernel (the order contract of ``csrc/sqdist_tile.h``), and the
neighbour lists are ordered by ``(distance, index)``, a strict total order, so the list for ``k' < k`` is a prefix of the
list for ``k``: one masked pass at the largest k serves every fold and every k of a sweep, and every prediction is a
function of the data alone.

Deviations from scikit-learn, on purpose:

* **neighbour ties** are resolved by ``(distance, index)``; sklearn leaves rows at equal distance to ``argpartition``;
* **distances** are formed by direct differences in fp64; sklearn expands ``|x|^2 + |y|^2 - 2 x.y``;
* **folds** are given as a label vector (``PredefinedSplit``'s ``test_fold`` without the -1 code): row i is predicted
  from the rows of the other folds;
* a sweep of ``n_neighbors`` is strictly ascending, at most 16 values, each at most ``projection.MAX_K`` = 64;
* ``weights`` is ``'uniform'`` or ``'distance'``; callables, other metrics, ``p``, ``algorithm`` (other than
  ``'auto'`` / ``'brute'``) and ``radius`` raise ``NotImplementedError``; rows with NaN or infinity are refused.

There is no CPU fallback: without the HIP library / a GPU every device function raises ``AvaHipError``.
"""
import numbers

import numpy as np
import torch

from . import _lib, _rows
from . import cluster_metrics as _cm
from . import projection as _pj

__all__ = ["masked_kneighbors", "kfold", "group_folds", "cross_val_predict", "cross_val_score", "KNeighborsClassifier",
           "KNeighborsRegressor", "MAX_N", "MAX_SWEEP", "MAX_CLASSES", "MAX_OUTPUTS"]
MAX_N = 2 ** 24                 # rows of one table
MAX_SWEEP = 16                  # ava_kp_max_sweep
MAX_CLASSES = 4096              # ava_kp_max_classes: predict_proba only
MAX_OUTPUTS = 256               # ava_kp_max_outputs
_KNN_CHUNK = 2 ** 17            # query rows of one kNN launch
_WEIGHTS = ('uniform', 'distance')
_TASKS = ('classify', 'regress')


def _device():
    return _lib.device("kNN prediction")


# ---- argument checks (no device) -------------------------------------------------------------------------------------
def _check_weights(weights):
    if callable(weights):
        raise NotImplementedError("a callable 'weights' is not on the device: use 'uniform' or 'distance'")
    if not isinstance(weights, str) or weights not in _WEIGHTS:
        raise ValueError("The 'weights' parameter must be a str among {'uniform', 'distance'}. Got %r instead."
                         % (weights,))
    return _WEIGHTS.index(weights)


def _check_unsupported(metric='euclidean', p=2, algorithm='auto', radius=None):
    if not (metric == 'euclidean' or (metric == 'minkowski' and p == 2)):
        raise NotImplementedError("metric=%r: only the euclidean metric is on the device" % (metric,))
    if p != 2:
        raise NotImplementedError("p=%r: only the euclidean metric (p = 2) is on the device" % (p,))
    if algorithm not in ('auto', 'brute'):
        raise NotImplementedError("algorithm=%r: the device search is exact and brute-force" % (algorithm,))
    if radius is not None:
        raise NotImplementedError("radius neighbours are not on the device")


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _check_sweep(n_neighbors):
    """(ks int32 ascending, scalar): an int, or a strictly ascending sequence of at most MAX_SWEEP ints"""
    if _is_int(n_neighbors):
        ks, scalar = [int(n_neighbors)], True
    else:
        if isinstance(n_neighbors, (str, bytes)) or not hasattr(n_neighbors, '__len__'):
            raise ValueError("n_neighbors must be an int or a sequence of ints, got %r" % (n_neighbors,))
        ks, scalar = list(n_neighbors), False
        if len(ks) == 0:
            raise ValueError("n_neighbors is empty")
        if len(ks) > MAX_SWEEP:
            raise ValueError("n_neighbors holds %d values: a sweep has at most %d" % (len(ks), MAX_SWEEP))
        if not all(_is_int(k) for k in ks):
            raise ValueError("n_neighbors must be an int or a sequence of ints, got %r" % (n_neighbors,))
        ks = [int(k) for k in ks]
        if any(b <= a for a, b in zip(ks, ks[1:])):
            raise ValueError("n_neighbors must be strictly ascending, got %r" % (ks,))
    if ks[0] < 1:
        raise ValueError("Expected n_neighbors > 0. Got %d" % ks[0])
    if ks[-1] > _pj.MAX_K:
        raise ValueError("n_neighbors = %d: at most %d (projection.MAX_K, the neighbours the kNN kernel keeps)"
                         % (ks[-1], _pj.MAX_K))
    return np.asarray(ks, dtype=np.int32), scalar


def _check_x(X):
    return _cm._check_pair_rows(X, 'euclidean', MAX_N)


def _as_1d(a, n, what):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    a = np.asarray(a)
    if a.ndim == 2 and a.shape[1] == 1 and what != 'y_regress':
        a = a.reshape(-1)
    if what != 'y_regress' and a.ndim != 1:
        raise ValueError("%s should be a 1d array, got an array of shape %s instead." % (what, a.shape))
    if len(a) != n:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (n, len(a)))
    return a


def _check_fold(fold, n, kmax):
    """the folds coded 0 .. n_folds - 1 (int32 [n]) and the number of folds"""
    fold = _as_1d(fold, n, "fold")
    if fold.dtype.kind not in "iu":
        raise ValueError("fold must be integers, got dtype %s" % fold.dtype)
    values, codes, counts = np.unique(fold, return_inverse=True, return_counts=True)
    if len(values) < 2:
        raise ValueError("fold holds %d distinct value(s): cross-validation needs at least 2 folds" % len(values))
    if n - int(counts.max()) < kmax:
        raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d: the largest "
                         "fold leaves too few eligible rows" % (kmax, n - int(counts.max())))
    return codes.reshape(-1).astype(np.int32), len(values)


def _check_classes(y, n):
    """(classes, codes int32 [n])"""
    y = _as_1d(y, n, "y")
    if y.dtype.kind not in "iubUSO":
        raise ValueError("Unknown label type: classes must be integers or strings, got dtype %s" % y.dtype)
    classes, codes = np.unique(y, return_inverse=True)
    return classes, codes.reshape(-1).astype(np.int32)


def _check_targets(y, n):
    """(Y float64 [n, n_out], whether y was 1-d)"""
    y = _as_1d(y, n, "y_regress")
    if y.ndim not in (1, 2):
        raise ValueError("y should be a 1d or 2d array, got an array of shape %s instead." % (y.shape,))
    if y.dtype.kind not in "fiu":
        raise ValueError("regression targets must be numbers, got dtype %s" % y.dtype)
    Y = np.ascontiguousarray(y.reshape(n, -1), dtype=np.float64)
    if Y.shape[1] < 1 or Y.shape[1] > MAX_OUTPUTS:
        raise ValueError("y has %d outputs: between 1 and %d" % (Y.shape[1], MAX_OUTPUTS))
    if not np.isfinite(Y).all():
        raise ValueError("Input y contains NaN or infinity.")
    return Y, y.ndim == 1


def kfold(n, n_splits=5):
    """The ``test_fold`` of ``sklearn.model_selection.KFold(n_splits)`` without shuffling, int64 ``[n]``: consecutive
    runs, the first ``n % n_splits`` one row longer."""
    if not _is_int(n_splits) or n_splits < 2:
        raise ValueError("k-fold cross-validation requires at least one train/test split by setting n_splits=2 or more,"
                         " got n_splits=%r." % (n_splits,))
    if not _is_int(n) or n < n_splits:
        raise ValueError("Cannot have number of splits n_splits=%d greater than the number of samples: n_samples=%r."
                         % (n_splits, n))
    sizes = np.full(n_splits, n // n_splits, dtype=np.int64)
    sizes[:n % n_splits] += 1
    return np.repeat(np.arange(n_splits, dtype=np.int64), sizes)


def group_folds(groups):
    """One fold per distinct group (``LeaveOneGroupOut``: leave-one-animal-out), int64 ``[n]``: the rank of each row's
    group among the sorted distinct groups.  ``groups`` are integers or strings."""
    if torch.is_tensor(groups):
        groups = groups.cpu().numpy()
    groups = np.asarray(groups)
    if groups.ndim != 1:
        raise ValueError("groups should be a 1d array, got an array of shape %s instead." % (groups.shape,))
    if groups.dtype.kind not in "iubUSO":
        raise ValueError("groups must be integers or strings, got dtype %s" % groups.dtype)
    values, codes = np.unique(groups, return_inverse=True)
    if len(values) < 2:
        raise ValueError("The groups parameter contains fewer than 2 unique groups (%s). LeaveOneGroupOut expects at "
                         "least 2." % (values,))
    return codes.reshape(-1).astype(np.int64)


# ---- the launches ----------------------------------------------------------------------------------------------------
def _masked_device(Xd, fold_d, k):
    """(idx int64 [N, k], dist float64 [N, k]) on the device: ``ava_kp_knn_masked`` in row chunks"""
    lib = _lib.load()
    n, d = int(Xd.shape[0]), int(Xd.shape[1])
    idx = torch.empty((n, k), dtype=torch.int64, device=Xd.device)
    dist = torch.empty((n, k), dtype=torch.float64, device=Xd.device)
    for q0 in range(0, n, _KNN_CHUNK):
        nq = min(_KNN_CHUNK, n - q0)
        _lib.check(lib.ava_kp_knn_masked(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, fold_d.data_ptr(), q0, nq,
                                         idx[q0:].data_ptr(), dist[q0:].data_ptr(), _lib.stream()), "ava_kp_knn_masked")
    return idx, dist


def _vote_device(idx, dist, y_d, ks, weighted):
    """int32 [n_k, nq] class codes"""
    nq, kmax = int(idx.shape[0]), int(idx.shape[1])
    out = torch.empty((len(ks), nq), dtype=torch.int32, device=idx.device)
    _lib.check(_lib.load().ava_kp_vote(idx.data_ptr(), dist.data_ptr(), nq, kmax, y_d.data_ptr(), ks.ctypes.data,
                                       len(ks), weighted, out.data_ptr(), _lib.stream()), "ava_kp_vote")
    return out


def _regress_device(idx, dist, Y_d, ks, weighted):
    """float64 [n_k, nq, n_out]"""
    nq, kmax, n_out = int(idx.shape[0]), int(idx.shape[1]), int(Y_d.shape[1])
    out = torch.empty((len(ks), nq, n_out), dtype=torch.float64, device=idx.device)
    _lib.check(_lib.load().ava_kp_regress(idx.data_ptr(), dist.data_ptr(), nq, kmax, Y_d.data_ptr(), n_out,
                                          ks.ctypes.data, len(ks), weighted, out.data_ptr(), _lib.stream()),
               "ava_kp_regress")
    return out


def _proba_device(idx, dist, y_d, n_classes, weighted):
    """float64 [nq, n_classes] from a [nq, k] table"""
    nq, k = int(idx.shape[0]), int(idx.shape[1])
    out = torch.empty((nq, n_classes), dtype=torch.float64, device=idx.device)
    _lib.check(_lib.load().ava_kp_proba(idx.data_ptr(), dist.data_ptr(), nq, k, y_d.data_ptr(), n_classes, weighted,
                                        out.data_ptr(), _lib.stream()), "ava_kp_proba")
    return out


# ---- cross-validation ------------------------------------------------------------------------------------------------
def masked_kneighbors(X, fold, k):
    """The ``k`` nearest rows of every row of ``X`` among the rows of OTHER folds: ``(dist float64 [N, k],
    idx int64 [N, k])`` as numpy arrays, ordered by (distance, index) -- what ``kneighbors`` of a model fitted on the
    other folds returns for the row, for every fold at once.  ``X`` is ``[N, d]``, numpy or tensor, host or device,
    float32 or float64; ``fold`` ``[N]`` of any integer dtype.  Every fold must leave at least ``k`` rows."""
    if not _is_int(k) or not 1 <= k <= _pj.MAX_K:
        raise ValueError("k must be an int in [1, %d], got %r" % (_pj.MAX_K, k))
    X = _check_x(X)
    codes, _ = _check_fold(fold, int(X.shape[0]), int(k))
    dev = _device()
    idx, dist = _masked_device(_rows.upload(X, dev), torch.from_numpy(codes).to(dev), int(k))
    return dist.cpu().numpy(), idx.cpu().numpy()


def _cross_val_device(X, y, fold, n_neighbors, weights, task):
    """everything of a cross-validation on the device: a dict with pred ([n_k, N] int32 codes or [n_k, N, n_out]
    float64), the targets (codes int64 or float64 [N, n_out]), the fold codes, the sweep and the classes"""
    if task not in _TASKS:
        raise ValueError("task must be 'classify' or 'regress', got %r" % (task,))
    weighted = _check_weights(weights)
    ks, scalar = _check_sweep(n_neighbors)
    X = _check_x(X)
    n = int(X.shape[0])
    codes, n_folds = _check_fold(fold, n, int(ks[-1]))
    if task == 'classify':
        classes, target = _check_classes(y, n)
        flat = True
    else:
        classes = None
        target, flat = _check_targets(y, n)
    dev = _device()
    fold_d = torch.from_numpy(codes).to(dev)
    target_d = torch.from_numpy(target).to(dev)
    idx, dist = _masked_device(_rows.upload(X, dev), fold_d, int(ks[-1]))
    if task == 'classify':
        pred = _vote_device(idx, dist, target_d, ks, weighted)
    else:
        pred = _regress_device(idx, dist, target_d, ks, weighted)
    return dict(pred=pred, target=target_d, fold=fold_d, n_folds=n_folds, ks=ks, scalar=scalar, classes=classes,
                flat=flat)


def cross_val_predict(X, y, fold, *, n_neighbors=5, weights='uniform', task='classify'):
    """The out-of-fold predictions of sklearn's ``cross_val_predict(KNeighborsClassifier / KNeighborsRegressor
    (n_neighbors, weights=weights, algorithm='brute'), X, y, cv=PredefinedSplit(fold))`` for every ``n_neighbors`` of a
    sweep: one masked distance pass at the largest, then one vote (``task='classify'``) or regress launch.

    ``n_neighbors`` is an int or a strictly ascending sequence of at most 16.  Returns a numpy array ``[n_k, N]`` --
    classes in ``y``'s own dtype (integers or strings), or float64 values -- or ``[n_k, N, n_out]`` for 2-d regression
    targets; a scalar ``n_neighbors`` drops the leading axis.  A tie between classes goes to the smallest class, as in
    sklearn; neighbours at equal distance are ordered by index (module docstring)."""
    r = _cross_val_device(X, y, fold, n_neighbors, weights, task)
    pred = r["pred"].cpu().numpy()
    if task == 'classify':
        pred = r["classes"][pred]
    elif r["flat"]:
        pred = pred[:, :, 0]
    return pred[0] if r["scalar"] else pred


def _r2(target, pred):
    """sklearn's r2_score(multioutput='uniform_average', force_finite=True) of [m, n_out] tensors, as a float"""
    res = ((target - pred) ** 2).sum(dim=0)
    tot = ((target - target.mean(dim=0, keepdim=True)) ** 2).sum(dim=0)
    ok = tot != 0
    score = torch.where(ok, 1.0 - res / torch.where(ok, tot, torch.ones_like(tot)),
                        torch.where(res != 0, torch.zeros_like(res), torch.ones_like(res)))
    return float(score.mean())


def cross_val_score(X, y, fold, *, n_neighbors=5, weights='uniform', task='classify', confusion=False):
    """The scores of the out-of-fold predictions of :func:`cross_val_predict`, a dict:

    * ``per_fold`` float64 ``[n_folds, n_k]`` (folds in ascending order of their label): ``accuracy_score`` or
      ``r2_score(multioutput='uniform_average')`` of each fold's rows -- sklearn's ``cross_val_score`` with
      ``PredefinedSplit(fold)``;
    * ``pooled`` float64 ``[n_k]``: the same score over all rows at once;
    * ``n_neighbors`` int64 ``[n_k]``; ``classes`` (classification);
    * with ``confusion=True`` (classification) ``confusion`` int64 ``[n_k, C, C]``: rows are true classes, columns
      predicted ones, as ``sklearn.metrics.confusion_matrix``.

    A scalar ``n_neighbors`` keeps the ``n_k = 1`` axis.  The reductions are torch on the device."""
    if confusion and task != 'classify':
        raise ValueError("confusion=True needs task='classify'")
    r = _cross_val_device(X, y, fold, n_neighbors, weights, task)
    pred, target, ks = r["pred"], r["target"], r["ks"]
    order = torch.sort(r["fold"], stable=True)[1]
    bounds = np.concatenate([[0], np.cumsum(np.bincount(r["fold"].cpu().numpy(), minlength=r["n_folds"]))])
    per_fold = np.empty((r["n_folds"], len(ks)), dtype=np.float64)
    pooled = np.empty(len(ks), dtype=np.float64)
    out = dict(n_neighbors=ks.astype(np.int64))
    if task == 'classify':
        # counts on the device (exact), one correctly rounded division each on the host, as accuracy_score's mean
        hit = (pred == target[None, :].to(pred.dtype))[:, order].to(torch.float64)
        for f in range(r["n_folds"]):
            per_fold[f] = hit[:, bounds[f]:bounds[f + 1]].sum(dim=1).cpu().numpy() / float(bounds[f + 1] - bounds[f])
        pooled[:] = hit.sum(dim=1).cpu().numpy() / float(hit.shape[1])
        out["classes"] = r["classes"]
        if confusion:
            c = len(r["classes"])
            pair = target[None, :].to(torch.int64) * c + pred.to(torch.int64)
            out["confusion"] = torch.stack([torch.bincount(p, minlength=c * c) for p in pair]).reshape(
                len(ks), c, c).cpu().numpy().astype(np.int64)
    else:
        t_sorted, p_sorted = target[order], pred[:, order]
        for a in range(len(ks)):
            for f in range(r["n_folds"]):
                per_fold[f, a] = _r2(t_sorted[bounds[f]:bounds[f + 1]], p_sorted[a, bounds[f]:bounds[f + 1]])
            pooled[a] = _r2(target, pred[a])
    out["per_fold"], out["pooled"] = per_fold, pooled
    return out


# ---- the estimators --------------------------------------------------------------------------------------------------
class _KNeighbors:
    """what the two estimators share: the fitted rows on the device and the neighbour tables"""

    def __init__(self, n_neighbors=5, *, weights='uniform', algorithm='auto', p=2, metric='euclidean', radius=None):
        self.n_neighbors = n_neighbors
        self.weights = weights
        self.algorithm = algorithm
        self.p = p
        self.metric = metric
        self.radius = radius

    def _check(self):
        _check_unsupported(self.metric, self.p, self.algorithm, self.radius)
        self._weighted = _check_weights(self.weights)
        ks, scalar = _check_sweep(self.n_neighbors)
        if not scalar:
            raise ValueError("n_neighbors of an estimator is one int; sweeps go through cross_val_predict")
        return int(ks[0])

    def _fit_rows(self, X):
        self._check()
        X = _check_x(X)
        self.n_samples_fit_ = int(X.shape[0])
        self.n_features_in_ = int(X.shape[1])
        return X

    def _table(self, Xq, k):
        """(idx, dist) on the device: of the fitted rows without themselves (``Xq`` None), or of new rows"""
        if not hasattr(self, "_Xd"):
            raise ValueError("This %s instance is not fitted yet. Call 'fit' first." % type(self).__name__)
        n = self.n_samples_fit_
        if Xq is None:
            if k > n - 1:
                raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d, "
                                 "n_samples = %d" % (k, n - 1, n))
            fold = torch.arange(n, dtype=torch.int32, device=self._Xd.device)
            return _masked_device(self._Xd, fold, k)
        if k > n:
            raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d"
                             % (k, n))
        Xq = _check_x(Xq)
        if int(Xq.shape[1]) != self.n_features_in_:
            raise ValueError("X has %d features, but %s is expecting %d features as input."
                             % (int(Xq.shape[1]), type(self).__name__, self.n_features_in_))
        qd = _rows.upload(Xq, self._Xd.device).to(self._Xd.dtype)
        return _pj._knn_query_device(qd, self._Xd, k, _KNN_CHUNK)

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
        """sklearn's ``kneighbors``: ``(dist float64 [m, k], idx int64 [m, k])`` ordered by (distance, index).  Without
        ``X`` the table of the fitted rows, each without itself (sklearn's leave-one-out table)."""
        k = self._check() if n_neighbors is None else int(_check_sweep(n_neighbors)[0][0])
        idx, dist = self._table(X, k)
        return (dist.cpu().numpy(), idx.cpu().numpy()) if return_distance else idx.cpu().numpy()


class KNeighborsClassifier(_KNeighbors):
    """scikit-learn 1.7's ``KNeighborsClassifier`` on the device for the euclidean metric: ``fit``, ``kneighbors``,
    ``predict``, ``predict_proba``, ``score`` (accuracy) and ``classes_``.  ``X`` is numpy or tensor, host or device,
    float32 or float64; ``y`` holds integers or strings.  ``predict(None)`` / ``predict_proba(None)`` predict the fitted
    rows, each without itself (leave-one-out).  Deviations: module docstring."""

    def fit(self, X, y):
        X = self._fit_rows(X)
        self.classes_, codes = _check_classes(y, self.n_samples_fit_)
        dev = _device()
        self._Xd = _rows.upload(X, dev)
        self._yd = torch.from_numpy(codes).to(dev)
        return self

    def predict(self, X=None):
        k = self._check()
        idx, dist = self._table(X, k)
        pred = _vote_device(idx, dist, self._yd, np.asarray([k], dtype=np.int32), self._weighted)
        return self.classes_[pred[0].cpu().numpy()]

    def predict_proba(self, X=None):
        k = self._check()
        if len(self.classes_) > MAX_CLASSES:
            raise ValueError("predict_proba holds at most %d classes, got %d" % (MAX_CLASSES, len(self.classes_)))
        idx, dist = self._table(X, k)
        return _proba_device(idx, dist, self._yd, len(self.classes_), self._weighted).cpu().numpy()

    def score(self, X, y):
        pred = self.predict(X)
        y = _as_1d(y, len(pred), "y")
        return float(np.mean(pred == y))


class KNeighborsRegressor(_KNeighbors):
    """scikit-learn 1.7's ``KNeighborsRegressor`` on the device for the euclidean metric: ``fit``, ``kneighbors``,
    ``predict`` and ``score`` (R^2, ``uniform_average`` over the outputs).  ``y`` is ``[N]`` or ``[N, n_out]``,
    ``n_out <= 256``; ``predict(None)`` predicts the fitted rows, each without itself.  Deviations: module docstring."""

    def fit(self, X, y):
        X = self._fit_rows(X)
        Y, self._flat = _check_targets(y, self.n_samples_fit_)
        dev = _device()
        self._Xd = _rows.upload(X, dev)
        self._yd = torch.from_numpy(Y).to(dev)
        return self

    def _predict_device(self, X):
        k = self._check()
        idx, dist = self._table(X, k)
        return _regress_device(idx, dist, self._yd, np.asarray([k], dtype=np.int32), self._weighted)[0]

    def predict(self, X=None):
        pred = self._predict_device(X).cpu().numpy()
        return pred[:, 0] if self._flat else pred

    def score(self, X, y):
        pred = self._predict_device(X)
        Y, _ = _check_targets(y, int(pred.shape[0]))
        return _r2(torch.from_numpy(Y).to(pred.device), pred)
