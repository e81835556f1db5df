"""Lloyd k-means with k-means++ seeding of latent rows on the MI355X: the fast partition
and the sweep over k ("k = 2 ... 40 clusters, pick by silhouette") of a syllable repertoire.

The reference package has no counterpart: the specification is scikit-learn 1.7's ``cluster/_kmeans.py``
(``_kmeans_plusplus``, ``_init_centroids``, ``_tolerance``, ``_kmeans_single_lloyd``, the ``n_init`` loop and best-run
rule of ``KMeans.fit``) and ``_relocate_empty_clusters_dense`` / ``_inertia_dense`` of ``_k_means_common.pyx``, followed
step by step with ``csrc/kmeans.hip``:

=====================================  ========================================  ====================================
scikit-learn 1.7                       here                                      C entry point
=====================================  ========================================  ====================================
``_kmeans_plusplus``                   :func:`kmeans_plusplus`                   ``ava_km_pp_start``, ``ava_km_pp_step``
``_tolerance``                         the variance of a fit                     ``ava_km_variance``
``_kmeans_single_lloyd``               one run of :meth:`KMeans.fit`             ``ava_km_fit``, ``ava_km_assign``
``lloyd_iter_chunked_dense`` (E-step)  :func:`assign`                            ``ava_km_assign``
``lloyd_iter_chunked_dense`` (M-step)  :func:`update`                            ``ava_km_update``
``KMeans.transform``                   :meth:`KMeans.transform`                  ``ava_km_transform``
=====================================  ========================================  ====================================

The model
---------
* **Arithmetic.**  All arithmetic is fp64, also for float32 rows.  Every distance is the tile of ``csrc/sqdist_tile.h``:
  direct differences, ``fma``, features ascending; a (row, centre) pair has the bits ``ava_pair_sqdist`` gives it.  Rows
  are not centred: sklearn subtracts the column means only to tame its ``|x|^2 - 2 x.c + |c|^2`` expansion.
* **Assignment.**  Each row takes its nearest centre; ties go to the lowest centre index (``np.argmin``).
* **Sums.**  No floating-point atomics.  Every sum over rows (per-cluster sums and counts, inertia, the k-means++
  potentials, the column variances) is taken inside chunks of 2048 rows in ascending row order, and the chunk partials
  are added in ascending chunk order.  A fit gives the same bits on every run, for float32 and float64 copies of the same
  values, and for every ``iter_block``.
* **k-means++.**  The host makes sklearn's draws with the caller's ``RandomState``, call for call: ``choice(n, p=1/n)``,
  then one ``uniform(size=L)`` per later centre, ``L = 2 + int(log K)``.  The device keeps ``closest [N]``, forms its
  inclusive scan (sequential inside the chunks, the ascending chunk offsets added), finds the candidates as
  ``searchsorted(scan, r * pot)`` clipped to ``N - 1``, forms ``min(closest, d2(candidate, .))`` and the potentials, and
  commits the candidate of least potential, the first on a tie.  The chosen rows stay on the device until the last
  centre: the host reads them once.
* **Iteration** (sklearn's loop).  Assign; new centres = sum / count; ``shift = sum |c_new - c_old|^2``; stop when no
  label changed (strict), else when ``shift <= tol * mean(var(X, axis=0))``; then one assignment at the final centres
  gives ``labels_`` and ``inertia_ = sum d2(x, c_label)`` (after a strict stop it repeats the labels: the final centres
  have the bits of the ones before them).  ``n_iter_`` counts as sklearn's does.  The variance is taken once per fit, on
  the device.  The stopping rule is evaluated on the device after every iteration; the loop is enqueued in blocks of
  ``iter_block`` iterations between two host reads of a small control array, and once it has stopped later launches
  return at once (the design of ``mixture``'s EM loop).
* **Empty clusters.**  The empty clusters, in ascending id, take the rows with the largest distance to their own centre of
  this iteration, ties to the lowest row; each such row leaves its old cluster's sum and count.  sklearn's
  ``argpartition`` leaves the order among several such rows unspecified: the one place this model fixes something
  sklearn does not.
* **Restarts.**  ``n_init='auto'`` is 1 for ``'k-means++'`` and an array, 10 for ``'random'``; a run replaces the best
  when its inertia is smaller and the clustering is not the same (``_is_same_clustering``); every run draws from the same
  ``RandomState`` in sequence.

Deviations from scikit-learn, on purpose: the distance arithmetic and the order of the sums above (sklearn's results
agree to rounding; the labels agree wherever no rule is within rounding of a tie); ``algorithm='elkan'``,
``sample_weight``, a callable ``init`` and sparse input raise ``NotImplementedError``; rows with NaN or infinity are
refused; ``1 <= d <= 128``, ``n_clusters <= 256``.  Numpy rows give numpy results, tensors give device tensors.

There is no CPU fallback: without the HIP library / a GPU every device function raises ``AvaHipError``.
``mixture``'s private k-means start is another model and is left as it is (profiles/NOTES.md).
"""
import numbers
import warnings

import numpy as np
import torch

from . import _lib, _rows

__all__ = ["KMeans", "kmeans_plusplus", "assign", "update", "kmeans_sweep", "KMeansConvergenceWarning", "MAX_D", "MAX_K",
           "CHUNK_ROWS"]
MAX_D = 128                     # ava_km_max_d
MAX_K = 256                     # ava_km_max_k
CHUNK_ROWS = 2048               # ava_km_chunk_rows
MAX_N = 2 ** 31 - 64


class KMeansConvergenceWarning(UserWarning):
    """what sklearn reports as ``ConvergenceWarning``: fewer distinct clusters than ``n_clusters``"""


def _device():
    return _lib.device("k-means")


# ---- argument checks (no device) -------------------------------------------------------------------------------------
def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _check_int(v, name, owner, low=1):
    if not _is_int(v) or v < low:
        raise ValueError("The %r parameter of %s must be an int in the range [%d, inf). Got %r instead."
                         % (name, owner, low, v))
    return int(v)


def _check_rows(X, what="X"):
    """sklearn's check_array for dense rows: float32 or float64 rows as they are, every other dtype as float64"""
    if callable(getattr(X, "tocsr", None)):
        raise NotImplementedError("sparse input is not on the device: pass dense rows")
    X = _rows.native(X)
    shape = tuple(X.shape)
    if len(shape) != 2:
        raise ValueError("Expected 2D array, got %dD array instead" % len(shape))
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError("Found array with %d sample(s) and %d feature(s) while a minimum of 1 is required"
                         % (shape[0], shape[1]))
    if shape[0] > MAX_N:
        raise ValueError("unsupported shape: N = %d rows, at most %d" % (shape[0], MAX_N))
    if shape[1] > MAX_D:
        raise ValueError("unsupported shape: d = %d features, at most %d" % (shape[1], MAX_D))
    if _rows.has_nan(X):
        raise ValueError("Input %s contains NaN." % what)
    if not _rows.is_finite(X):
        raise ValueError("Input %s contains infinity or a value too large for dtype('float64')." % what)
    return X


def _check_k(k, owner="KMeans"):
    k = _check_int(k, "n_clusters", owner)
    if k > MAX_K:
        raise ValueError("n_clusters = %d: the device path holds at most %d clusters" % (k, MAX_K))
    return k


def _random_state(seed):
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, np.random.RandomState):
        return seed
    if _is_int(seed):
        return np.random.RandomState(seed)
    raise ValueError("%r cannot be used to seed a numpy.random.RandomState instance" % (seed,))


def _is_same_clustering(a, b, k):
    """sklearn's ``_is_same_clustering``: every cluster of ``a`` lies in one cluster of ``b``"""
    return len(np.unique(a.astype(np.int64) * k + b)) == len(np.unique(a))


def _like(t, X):
    """a device result in the kind of the caller's rows: numpy for numpy, the device tensor for a tensor"""
    return t if torch.is_tensor(X) else t.cpu().numpy()


# ---- the launches ----------------------------------------------------------------------------------------------------
def _workspace(n, d, k, dev):
    nbytes = int(_lib.load().ava_km_workspace_bytes(n, d, k))
    return _lib.workspace(nbytes, dev, "N = %d rows, d = %d features, %d clusters" % (n, d, k)), nbytes


def _assign_device(Xd, centres, inertia=False):
    """(labels int32 [N], d2 float64 [N], inertia float64 [1] or None) of rows and centres on the device"""
    n, d, k = int(Xd.shape[0]), int(Xd.shape[1]), int(centres.shape[0])
    ws, nbytes = _workspace(n, d, k, Xd.device)
    labels = torch.empty(n, dtype=torch.int32, device=Xd.device)
    d2 = torch.empty(n, dtype=torch.float64, device=Xd.device)
    total = torch.empty(1, dtype=torch.float64, device=Xd.device) if inertia else None
    _lib.check(_lib.load().ava_km_assign(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, centres.data_ptr(),
                                         labels.data_ptr(), d2.data_ptr(), _lib.ptr(total), ws.data_ptr(), nbytes,
                                         _lib.stream()), "ava_km_assign")
    return labels, d2, total


def _update_device(Xd, labels, k):
    n, d = int(Xd.shape[0]), int(Xd.shape[1])
    ws, nbytes = _workspace(n, d, k, Xd.device)
    centres = torch.empty((k, d), dtype=torch.float64, device=Xd.device)
    counts = torch.empty(k, dtype=torch.int64, device=Xd.device)
    _lib.check(_lib.load().ava_km_update(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, labels.data_ptr(),
                                         centres.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()),
               "ava_km_update")
    return centres, counts


def _variance_device(Xd):
    """float64 [1 + d] on the device: the mean of the column variances, then the variances"""
    n, d = int(Xd.shape[0]), int(Xd.shape[1])
    ws, nbytes = _workspace(n, d, 1, Xd.device)
    out = torch.empty(1 + d, dtype=torch.float64, device=Xd.device)
    _lib.check(_lib.load().ava_km_variance(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, out.data_ptr(), ws.data_ptr(),
                                           nbytes, _lib.stream()), "ava_km_variance")
    return out


def _transform_device(Xd, centres):
    n, d, k = int(Xd.shape[0]), int(Xd.shape[1]), int(centres.shape[0])
    out = torch.empty((n, k), dtype=torch.float64, device=Xd.device)
    _lib.check(_lib.load().ava_km_transform(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, centres.data_ptr(),
                                            out.data_ptr(), _lib.stream()), "ava_km_transform")
    return out


def _n_trials(k):
    return 2 + int(np.log(k))


def _plusplus_device(Xd, k, rs, rand=None, first=None):
    """sklearn's ``_kmeans_plusplus``: the chosen rows, int32 [k] on the device.  The draws are made here, before the first
    launch; ``rand`` ``[k - 1, L]`` and ``first`` replace them (the tests' thresholds at 0 and at the potential)."""
    lib = _lib.load()
    n, d = int(Xd.shape[0]), int(Xd.shape[1])
    trials = _n_trials(k)
    if first is None:
        first = int(rs.choice(n, p=np.full(n, 1.0 / n)))
    if rand is None:
        rand = np.empty((k - 1, trials), dtype=np.float64)
        for c in range(k - 1):
            rand[c] = rs.uniform(size=trials)
    rand = np.ascontiguousarray(rand, dtype=np.float64).reshape(k - 1, trials)
    dev = Xd.device
    ws, nbytes = _workspace(n, d, 1, dev)
    rand_d = torch.from_numpy(rand).to(dev)
    closest = torch.empty(n, dtype=torch.float64, device=dev)
    idx = torch.full((k,), first, dtype=torch.int32, device=dev)
    pot = torch.zeros(k, dtype=torch.float64, device=dev)
    code, st = _lib.dtype_code(Xd), _lib.stream()
    _lib.check(lib.ava_km_pp_start(Xd.data_ptr(), code, n, d, first, closest.data_ptr(), st), "ava_km_pp_start")
    for c in range(1, k):
        _lib.check(lib.ava_km_pp_step(Xd.data_ptr(), code, n, d, trials, rand_d[c - 1].data_ptr(), closest.data_ptr(),
                                      idx[c:].data_ptr(), pot[c:].data_ptr(), ws.data_ptr(), nbytes, st),
                   "ava_km_pp_step")
    return idx


def _lloyd_device(Xd, centres, tol, mean_var, max_iter, iter_block):
    """one run of sklearn's ``_kmeans_single_lloyd`` from ``centres`` (float64 [k, d] on the device, overwritten):
    (labels int32 [N], inertia float, n_iter int), the first still on the device"""
    lib = _lib.load()
    n, d, k = int(Xd.shape[0]), int(Xd.shape[1]), int(centres.shape[0])
    dev = Xd.device
    ws, nbytes = _workspace(n, d, k, dev)
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    ctl = torch.zeros(3 + max_iter, dtype=torch.int32, device=dev)
    code, st = _lib.dtype_code(Xd), _lib.stream()
    it = 0
    while it < max_iter:
        nb = min(iter_block, max_iter - it)
        _lib.check(lib.ava_km_fit(Xd.data_ptr(), code, n, d, k, centres.data_ptr(), labels.data_ptr(), d2.data_ptr(),
                                  float(tol), mean_var.data_ptr(), it, nb, ctl.data_ptr(), None, ws.data_ptr(), nbytes,
                                  st), "ava_km_fit")
        it += nb
        host = ctl.cpu().numpy()
        if host[2 + it]:
            break
    n_iter = int(ctl[1].item())
    labels, d2, inertia = _assign_device(Xd, centres, inertia=True)
    return labels, float(inertia.item()), n_iter


# ---- public functions ------------------------------------------------------------------------------------------------
def kmeans_plusplus(X, n_clusters, *, random_state=None):
    """sklearn's ``kmeans_plusplus(X, n_clusters, random_state=random_state)``: ``(centres [K, d], indices [K])``, the
    centres in the dtype of ``X``, the indices int64; numpy for numpy rows, device tensors for a tensor."""
    k = _check_k(n_clusters, "kmeans_plusplus")
    X = _check_rows(X)
    if X.shape[0] < k:
        raise ValueError("n_samples=%d should be >= n_clusters=%d." % (X.shape[0], k))
    rs = _random_state(random_state)
    Xd = _rows.upload(X, _device())
    idx = _plusplus_device(Xd, k, rs).to(torch.int64)
    return _like(Xd[idx], X), _like(idx, X)


def _check_centres(centres, d, what="centres"):
    centres = _rows.native(centres)
    if len(tuple(centres.shape)) != 2 or centres.shape[0] < 1 or centres.shape[0] > MAX_K:
        raise ValueError("%s must be [K, d] with 1 <= K <= %d, got shape %s" % (what, MAX_K, tuple(centres.shape)))
    if int(centres.shape[1]) != d:
        raise ValueError("%s has %d features, the rows have %d" % (what, int(centres.shape[1]), d))
    if not _rows.is_finite(centres):
        raise ValueError("Input %s contains NaN or infinity." % what)
    return centres


def assign(X, centres):
    """The nearest centre of every row: ``(labels int32 [N], d2 float64 [N])`` as device tensors; ``d2`` is the squared
    distance to that centre, ties go to the lowest centre."""
    X = _check_rows(X)
    centres = _check_centres(centres, int(X.shape[1]))
    dev = _device()
    labels, d2, _ = _assign_device(_rows.upload(X, dev), _rows.upload(centres, dev, torch.float64))
    return labels, d2


def update(X, labels, k):
    """One M-step: ``(centres float64 [k, d], counts int64 [k])`` as device tensors, the mean of the rows of every label in
    the chunk order; an empty cluster has a centre of zeros."""
    k = _check_k(k, "update")
    X = _check_rows(X)
    if not torch.is_tensor(labels):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    if labels.dim() != 1 or int(labels.shape[0]) != int(X.shape[0]) or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("labels must be [N] integers, got shape %s of %s" % (tuple(labels.shape), labels.dtype))
    dev = _device()
    return _update_device(_rows.upload(X, dev), labels.to(device=dev, dtype=torch.int32).contiguous(), k)


class KMeans:
    """scikit-learn 1.7's ``KMeans`` on the device (``algorithm='lloyd'``): ``fit``, ``fit_predict``, ``predict``,
    ``transform``, ``fit_transform``, ``score``; after a fit ``cluster_centers_`` (float64 ``[K, d]``), ``labels_``
    (int32), ``inertia_``, ``n_iter_``, ``n_features_in_``.  Rows are ``[N, d]``, numpy or tensor, host or device, float32
    or float64, ``1 <= d <= 128``, ``n_clusters <= 256``; numpy rows give numpy results, tensors device tensors.  ``init``
    is ``'k-means++'``, ``'random'`` or a ``[K, d]`` array (which forces ``n_init`` 1).  The Lloyd loop runs on the device
    in blocks of ``iter_block`` iterations between two host reads; no result depends on ``iter_block``.  The model and the
    deviations from sklearn: module docstring."""

    def __init__(self, n_clusters=8, *, init='k-means++', n_init='auto', max_iter=300, tol=1e-4, random_state=None,
                 algorithm='lloyd', iter_block=16):
        self.n_clusters = n_clusters
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.tol = tol
        self.random_state = random_state
        self.algorithm = algorithm
        self.iter_block = iter_block

    def _check_params(self):
        """(k, init kind, the init array or None, n_init, random state)"""
        k = _check_k(self.n_clusters)
        if self.algorithm == 'elkan':
            raise NotImplementedError("algorithm='elkan' is not on the device: use 'lloyd'")
        if self.algorithm != 'lloyd':
            raise ValueError("The 'algorithm' parameter of KMeans must be a str among {'lloyd', 'elkan'}. Got %r instead."
                             % (self.algorithm,))
        init, centres = self.init, None
        if isinstance(init, str):
            if init not in ('k-means++', 'random'):
                raise ValueError("The 'init' parameter of KMeans must be a str among {'k-means++', 'random'} or an "
                                 "array-like. Got %r instead." % (init,))
        elif callable(init):
            raise NotImplementedError("a callable 'init' is not on the device: pass 'k-means++', 'random' or an array")
        else:
            centres, init = init, 'array'
        if self.n_init == 'auto':
            n_init = 10 if init == 'random' else 1
        else:
            n_init = _check_int(self.n_init, "n_init", "KMeans")
            if init == 'array' and n_init != 1:
                warnings.warn("Explicit initial center position passed: performing only one init in KMeans instead of "
                              "n_init=%d." % n_init, RuntimeWarning, stacklevel=3)
                n_init = 1
        _check_int(self.max_iter, "max_iter", "KMeans")
        _check_int(self.iter_block, "iter_block", "KMeans")
        if isinstance(self.tol, bool) or not isinstance(self.tol, numbers.Real) or not self.tol >= 0:
            raise ValueError("The 'tol' parameter of KMeans must be a float in the range [0.0, inf). Got %r instead."
                             % (self.tol,))
        return k, init, centres, n_init, _random_state(self.random_state)

    def _check_fit(self, X, sample_weight):
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not on the device")
        k, init, centres, n_init, rs = self._check_params()
        X = _check_rows(X)
        n, d = int(X.shape[0]), int(X.shape[1])
        if n < k:
            raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, k))
        if init == 'array':
            centres = _rows.native(centres)
            if len(tuple(centres.shape)) != 2 or int(centres.shape[0]) != k:
                raise ValueError("The shape of the initial centers %s does not match the number of clusters %d."
                                 % (tuple(centres.shape), k))
            if int(centres.shape[1]) != d:
                raise ValueError("The shape of the initial centers %s does not match the number of features of the data "
                                 "%d." % (tuple(centres.shape), d))
            if not _rows.is_finite(centres):
                raise ValueError("Input init contains NaN or infinity.")
        return X, k, init, centres, n_init, rs

    def _fit_device(self, Xd, k, init, centres, n_init, rs):
        """the runs on uploaded rows: sets the fitted state on the device"""
        n = int(Xd.shape[0])
        mean_var = _variance_device(Xd)
        best = None
        for _ in range(n_init):
            if init == 'k-means++':
                start = Xd[_plusplus_device(Xd, k, rs).to(torch.int64)].to(torch.float64)
            elif init == 'random':
                seeds = rs.choice(n, size=k, replace=False, p=np.full(n, 1.0 / n))
                start = Xd[torch.from_numpy(np.asarray(seeds, dtype=np.int64)).to(Xd.device)].to(torch.float64)
            else:
                start = _rows.upload(centres, Xd.device, torch.float64).clone()
            start = start.contiguous()
            labels, inertia, n_iter = _lloyd_device(Xd, start, self.tol, mean_var, int(self.max_iter),
                                                    int(self.iter_block))
            host = labels.cpu().numpy()
            if best is None or (inertia < best[1] and not _is_same_clustering(host, best[4], k)):
                best = (labels, inertia, n_iter, start, host)
        labels, inertia, n_iter, start, host = best
        distinct = len(np.unique(host))
        if distinct < k:
            warnings.warn("Number of distinct clusters (%d) found smaller than n_clusters (%d). Possibly due to duplicate "
                          "points in X." % (distinct, k), KMeansConvergenceWarning, stacklevel=3)
        self._centres = start
        self._labels = labels
        self.inertia_ = inertia
        self.n_iter_ = n_iter
        self.n_features_in_ = int(Xd.shape[1])
        return self

    def _publish(self, X):
        self.cluster_centers_ = _like(self._centres, X)
        self.labels_ = _like(self._labels, X)

    def fit(self, X, y=None, sample_weight=None):
        X, k, init, centres, n_init, rs = self._check_fit(X, sample_weight)
        self._fit_device(_rows.upload(X, _device()), k, init, centres, n_init, rs)
        self._publish(X)
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_

    def fit_transform(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).transform(X)

    def _query(self, X):
        if not hasattr(self, "_centres"):
            raise ValueError("This KMeans instance is not fitted yet. Call 'fit' with appropriate arguments before using "
                             "this estimator.")
        X = _check_rows(X)
        if int(X.shape[1]) != self.n_features_in_:
            raise ValueError("X has %d features, but KMeans is expecting %d features as input."
                             % (int(X.shape[1]), self.n_features_in_))
        return X, _rows.upload(X, self._centres.device)

    def predict(self, X):
        """the nearest fitted centre of every row, int32 ``[N]``"""
        X, Xd = self._query(X)
        return _like(_assign_device(Xd, self._centres)[0], X)

    def transform(self, X):
        """the euclidean distance of every row to every fitted centre, float64 ``[N, K]``"""
        X, Xd = self._query(X)
        return _like(_transform_device(Xd, self._centres), X)

    def score(self, X, y=None, sample_weight=None):
        """minus the inertia of ``X`` at the fitted centres, as sklearn's ``score``"""
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not on the device")
        X, Xd = self._query(X)
        return -float(_assign_device(Xd, self._centres, inertia=True)[2].item())


def kmeans_sweep(X, ks, *, scores=False, **kw):
    """One :class:`KMeans` fit per entry of ``ks`` on rows uploaded once (``kw`` are its other arguments).  Returns a dict
    of numpy arrays: ``'k'`` int64 ``[len(ks)]``, ``'inertia'`` float64, ``'n_iter'`` int64, ``'labels'`` int32
    ``[len(ks), N]``; row ``a`` equals ``KMeans(ks[a], **kw).fit(X)``.  With ``scores=True`` also ``'silhouette'``,
    ``'calinski_harabasz'`` and ``'davies_bouldin'`` float64 ``[len(ks)]`` of those labels through ``cluster_metrics``,
    NaN where a score is not defined or not held there (fewer than 2 distinct labels, more than its label limits)."""
    from . import cluster_metrics as _cm
    if isinstance(ks, (str, bytes)) or not hasattr(ks, '__len__') or len(ks) == 0:
        raise ValueError("ks must be a non-empty sequence of ints, got %r" % (ks,))
    models = [KMeans(k, **kw) for k in ks]
    checked = [m._check_fit(X, None) for m in models]
    Xd = _rows.upload(checked[0][0], _device())
    out = {'k': np.asarray([c[1] for c in checked], dtype=np.int64), 'inertia': np.empty(len(ks), dtype=np.float64),
           'n_iter': np.empty(len(ks), dtype=np.int64), 'labels': np.empty((len(ks), int(Xd.shape[0])), dtype=np.int32)}
    names = ('silhouette', 'calinski_harabasz', 'davies_bouldin') if scores else ()
    for name in names:
        out[name] = np.full(len(ks), np.nan, dtype=np.float64)
    for a, (m, c) in enumerate(zip(models, checked)):
        m._fit_device(Xd, *c[1:])
        out['inertia'][a], out['n_iter'][a] = m.inertia_, m.n_iter_
        out['labels'][a] = m._labels.cpu().numpy()
        for name, fn in zip(names, (_cm.silhouette_score, _cm.calinski_harabasz_score, _cm.davies_bouldin_score)):
            try:
                out[name][a] = fn(Xd, out['labels'][a])
            except ValueError:
                pass
    return out
