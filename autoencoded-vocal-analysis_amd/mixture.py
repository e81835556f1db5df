"""Gaussian mixture models of latent means on the MI355X.

The reference package has no counterpart: the specification is scikit-learn 1.7's ``GaussianMixture``
(sklearn/mixture/_gaussian_mixture.py, _base.py) with ``covariance_type`` ``'full'`` or ``'diag'``, followed step by
step with the HIP kernels of ``csrc/mixture.hip``:

=====================================  =====================================  ======================
scikit-learn 1.7                       here                                   C entry point
=====================================  =====================================  ======================
``_estimate_log_prob_resp``            :func:`e_step`                         ``ava_gm_e_step``
``_m_step`` (from ``resp``)            :func:`m_step`                         ``ava_gm_m_step``
the EM loop of ``fit_predict``         :meth:`GaussianMixture.fit`            ``ava_gm_fit``
``KMeans`` (``init_params='kmeans'``)  :func:`kmeans_labels` (own model)      ``ava_nn_argmin``, ``ava_gm_onehot``,
                                                                              ``ava_gm_means``
=====================================  =====================================  ======================

Deviations from scikit-learn, on purpose:

* all arithmetic is fp64, also for float32 ``X`` (sklearn 1.7 stays in float32 then);
* direct differences ``x - mu`` everywhere: ``(x - mu)^T P`` in the E-step (sklearn expands ``X P - mu P``) and centred
  second moments in the ``'diag'`` covariance (sklearn takes ``E[x^2] - 2 mu E[x] + mu^2``);
* every sum runs in this project's fixed orders (the contract at the head of ``csrc/mixture.hip``), so a fit gives the
  same bits on every run, for every ``iter_block`` and for float32 and float64 copies of the same values;
* ``init_params='kmeans'`` is this project's own Lloyd iteration, NOT sklearn's ``KMeans`` (:func:`kmeans_labels`);
* the start's weights are normalised like every other M-step's (sklearn's ``_initialize`` leaves ``nk / N`` as it is).

``'tied'`` and ``'spherical'`` covariances, ``init_params`` ``'k-means++'`` and ``'random'`` and ``warm_start`` are not
on the device and raise ``NotImplementedError``.  There is no CPU fallback: without the HIP library / a GPU every device
function raises ``AvaHipError``.
"""
import numpy as np
import torch

from . import _lib, _rows

__all__ = ["GaussianMixture", "e_step", "m_step", "kmeans_labels", "MAX_D", "MAX_K", "CHUNK_ROWS", "KMEANS_MAX_ITER"]
MAX_D = 128                     # ava_gm_max_d
MAX_K = 64                      # ava_gm_max_k
CHUNK_ROWS = 2048               # ava_gm_chunk_rows: rows of a chunk of the partial sums
KMEANS_MAX_ITER = 30
_COV = {'full': 0, 'diag': 1}
_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for "
                "instance caused by singleton or collapsed samples). Try to decrease the number of components, "
                "increase reg_covar, or scale the input data.")


def _device():
    return _lib.device("mixture")


def _cov_code(covariance_type):
    if covariance_type in ('tied', 'spherical'):
        raise NotImplementedError("covariance_type=%r: only 'full' and 'diag' are on the device" % (covariance_type,))
    if covariance_type not in _COV:
        raise ValueError("covariance_type must be 'full' or 'diag', got %r" % (covariance_type,))
    return _COV[covariance_type]


def _check_rows(X, n_components=1):
    """host-side checks of the rows; returns them as they go to the device (numpy or tensor, float32 or float64)"""
    X = _rows.native(X)
    shape = tuple(X.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("expected a non-empty 2-D array of rows, got shape %s" % (shape,))
    n, d = shape
    if d > MAX_D:
        raise ValueError("d = %d features: the device path holds at most MAX_D = %d" % (d, MAX_D))
    if not 1 <= n_components <= MAX_K:
        raise ValueError("n_components = %r: the device path holds 1 .. MAX_K = %d" % (n_components, MAX_K))
    if n < n_components:
        raise ValueError("n_samples = %d must be at least n_components = %d" % (n, n_components))
    if n >= 2 ** 31:
        raise ValueError("at most 2**31 - 1 rows")
    if not _rows.is_finite(X):
        raise ValueError("the input contains NaN or infinity")
    return X


def _f64(a, dev, shape, what):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
    return t.to(device=dev, dtype=torch.float64).contiguous()


def _workspace(n, d, k, code, dev):
    nbytes = _lib.load().ava_gm_workspace_bytes(n, d, k, code)
    return _lib.workspace(nbytes, dev, "N = %d, d = %d, n_components = %d" % (n, d, k)), nbytes


def _param_shape(k, d, code):
    return (k, d, d) if code == 0 else (k, d)


def _log_det(pchol, code):
    """sum of log diag P_k, ascending, as the factorisation kernel takes it; ``pchol`` a host array"""
    diag = np.diagonal(pchol, axis1=1, axis2=2) if code == 0 else pchol
    return np.cumsum(np.log(diag), axis=1)[:, -1].copy()


def _e_step(Xd, weights, means, pchol, log_det, code):
    n, d = Xd.shape
    k = weights.shape[0]
    dev = Xd.device
    lpn = torch.empty(n, dtype=torch.float64, device=dev)
    log_resp = torch.empty((n, k), dtype=torch.float64, device=dev)
    resp = torch.empty((n, k), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().ava_gm_e_step(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, code, weights.data_ptr(),
                                         means.data_ptr(), pchol.data_ptr(), log_det.data_ptr(), lpn.data_ptr(),
                                         log_resp.data_ptr(), resp.data_ptr(), _lib.stream()), "ava_gm_e_step")
    return lpn, log_resp, resp


def e_step(X, weights, means, precisions_cholesky, covariance_type='full'):
    """sklearn's ``_estimate_log_prob_resp`` on the device: ``(log_prob_norm [N], log_resp [N, K], resp [N, K])`` as
    float64 device tensors, ``resp = exp(log_resp)``.  ``X`` is ``[N, d]`` float32 or float64 (numpy or tensor); the
    parameters are arrays or tensors of sklearn's shapes (``precisions_cholesky`` ``[K, d, d]`` upper triangular for
    ``'full'``, ``[K, d]`` for ``'diag'``)."""
    code = _cov_code(covariance_type)
    k = int(np.shape(weights)[0])
    X = _check_rows(X, k)
    dev = _device()
    Xd = _rows.upload(X, dev)
    d = Xd.shape[1]
    w = _f64(weights, dev, (k,), "weights")
    mu = _f64(means, dev, (k, d), "means")
    P = _f64(precisions_cholesky, dev, _param_shape(k, d, code), "precisions_cholesky")
    log_det = torch.from_numpy(_log_det(P.cpu().numpy(), code)).to(dev)
    return _e_step(Xd, w, mu, P, log_det, code)


def _m_step(Xd, resp, reg_covar, code, ws=None):
    n, d = Xd.shape
    k = resp.shape[1]
    dev = Xd.device
    ws, nbytes = ws if ws is not None else _workspace(n, d, k, code, dev)
    weights = torch.empty(k, dtype=torch.float64, device=dev)
    means = torch.empty((k, d), dtype=torch.float64, device=dev)
    cov = torch.empty(_param_shape(k, d, code), dtype=torch.float64, device=dev)
    pchol = torch.zeros(_param_shape(k, d, code), dtype=torch.float64, device=dev)
    log_det = torch.zeros(k, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().ava_gm_m_step(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, code, resp.data_ptr(),
                                         float(reg_covar), weights.data_ptr(), means.data_ptr(), cov.data_ptr(),
                                         pchol.data_ptr(), log_det.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes,
                                         _lib.stream()), "ava_gm_m_step")
    if int(status.item()) != 0:
        raise ValueError(_ILL_DEFINED)
    return weights, means, cov, pchol, log_det


def m_step(X, resp, reg_covar=1e-6, covariance_type='full'):
    """sklearn's ``_m_step`` from the responsibilities ``resp`` (``[N, K]``, not their logarithms): ``(weights, means,
    covariances, precisions_cholesky, log_det)`` as float64 device tensors; ``log_det[k]`` is the sum of the logarithms
    of the diagonal of ``precisions_cholesky[k]``.  Raises sklearn's ``ValueError`` when a covariance is not positive
    definite."""
    code = _cov_code(covariance_type)
    if not reg_covar >= 0:
        raise ValueError("reg_covar must be non-negative, got %r" % (reg_covar,))
    if len(np.shape(resp)) != 2:
        raise ValueError("resp must be [N, K]")
    k = int(np.shape(resp)[1])
    X = _check_rows(X, k)
    dev = _device()
    Xd = _rows.upload(X, dev)
    r = _f64(resp, dev, (Xd.shape[0], k), "resp")
    return _m_step(Xd, r, reg_covar, code)


def _kmeans(Xd, seeds):
    """Lloyd's iteration from the rows ``seeds``: the device tensor of labels (int64) and the number of assignments"""
    lib = _lib.load()
    dev = Xd.device
    n, d = Xd.shape
    k = len(seeds)
    centres = Xd[torch.as_tensor(np.asarray(seeds, dtype=np.int64), device=dev)].to(torch.float64).contiguous()
    nn_bytes = lib.ava_nn_workspace_bytes(n, k, d, 1)
    nn_ws = _lib.workspace(nn_bytes, dev, "N = %d, d = %d, n_components = %d" % (n, d, k))
    ws, nbytes = _workspace(n, d, k, 1, dev)
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    dist = torch.empty(n, dtype=torch.float64, device=dev)
    prev = torch.full((n,), -1, dtype=torch.int64, device=dev)
    resp = torch.empty((n, k), dtype=torch.float64, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    weights = torch.empty(k, dtype=torch.float64, device=dev)
    means = torch.empty((k, d), dtype=torch.float64, device=dev)
    nk = torch.empty(k, dtype=torch.float64, device=dev)
    st = _lib.stream()
    rounds = 0
    for _ in range(KMEANS_MAX_ITER):
        _lib.check(lib.ava_nn_argmin(Xd.data_ptr(), _lib.dtype_code(Xd), n, centres.data_ptr(), 1, k, d, 1,
                                     labels.data_ptr(), dist.data_ptr(), nn_ws.data_ptr(), nn_bytes, st),
                   "ava_nn_argmin")
        changed.zero_()
        _lib.check(lib.ava_gm_onehot(labels.data_ptr(), prev.data_ptr(), n, k, resp.data_ptr(), changed.data_ptr(), st),
                   "ava_gm_onehot")
        rounds += 1
        if int(changed.item()) == 0:
            break
        _lib.check(lib.ava_gm_means(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, resp.data_ptr(), weights.data_ptr(),
                                    means.data_ptr(), nk.data_ptr(), ws.data_ptr(), nbytes, st), "ava_gm_means")
        centres = torch.where(nk[:, None] > 0.5, means, centres).contiguous()       # an empty cluster keeps its centre
    return labels, resp, rounds


def kmeans_labels(X, seeds):
    """The labels of this package's k-means start (NOT sklearn's ``KMeans``): the centres start at the rows ``seeds``;
    at most ``KMEANS_MAX_ITER`` times every row takes the nearest centre (``ava_nn_argmin``, euclidean: direct fp64
    squared differences, the lowest index wins ties) and, unless no label changed, every centre becomes the mean of its
    rows (an empty cluster keeps its centre).  Returns ``(labels int64 [N] numpy, number of assignments)``."""
    seeds = np.asarray(seeds, dtype=np.int64)
    X = _check_rows(X, len(seeds))
    if seeds.ndim != 1 or len(seeds) < 1 or seeds.min() < 0 or seeds.max() >= X.shape[0]:
        raise ValueError("seeds must be row indices")
    labels, _, rounds = _kmeans(_rows.upload(X, _device()), seeds)
    return labels.cpu().numpy(), rounds


def _random_state(seed):
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, np.random.RandomState):
        return seed
    return np.random.RandomState(seed)


class GaussianMixture:
    """scikit-learn 1.7's ``GaussianMixture`` with ``'full'`` or ``'diag'`` covariances on the device.

    ``fit`` takes ``[N, d]`` rows, numpy or device tensor, float32 or float64 (``1 <= d <= 128``, ``n_components <=
    64``).  Attributes after a fit, as sklearn's: ``weights_``, ``means_``, ``covariances_``, ``precisions_cholesky_``,
    ``precisions_`` (numpy float64), ``converged_``, ``n_iter_``, ``lower_bound_``, ``lower_bounds_``.  The EM loop runs
    on the device in blocks of ``iter_block`` iterations between two host reads; the stopping rule is evaluated on the
    device after every iteration, so ``iter_block`` changes no result.

    ``init_params='kmeans'`` (the default) is this package's own model, not sklearn's ``KMeans``: the seeds are the rows
    ``'random_from_data'`` draws, followed by :func:`kmeans_labels`.  ``'random_from_data'`` is sklearn's."""

    def __init__(self, n_components=1, *, covariance_type='full', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params='kmeans', weights_init=None, means_init=None, precisions_init=None, random_state=42,
                 warm_start=False, iter_block=10):
        _cov_code(covariance_type)
        if init_params in ('k-means++', 'random'):
            raise NotImplementedError("init_params=%r: only 'kmeans' and 'random_from_data' are on the device"
                                      % (init_params,))
        if init_params not in ('kmeans', 'random_from_data'):
            raise ValueError("init_params must be 'kmeans' or 'random_from_data', got %r" % (init_params,))
        if warm_start:
            raise NotImplementedError("warm_start=True is not on the device")
        if int(n_components) != n_components or not 1 <= n_components <= MAX_K:
            raise ValueError("n_components must be an integer in 1 .. %d, got %r" % (MAX_K, n_components))
        if not tol >= 0:
            raise ValueError("tol must be non-negative, got %r" % (tol,))
        if not reg_covar >= 0:
            raise ValueError("reg_covar must be non-negative, got %r" % (reg_covar,))
        for name, v in (("max_iter", max_iter), ("n_init", n_init), ("iter_block", iter_block)):
            if int(v) != v or v < 1:
                raise ValueError("%s must be a positive integer, got %r" % (name, v))
        self.n_components = int(n_components)
        self.covariance_type = covariance_type
        self.tol = float(tol)
        self.reg_covar = float(reg_covar)
        self.max_iter = int(max_iter)
        self.n_init = int(n_init)
        self.init_params = init_params
        self.weights_init = weights_init
        self.means_init = means_init
        self.precisions_init = precisions_init
        self.random_state = random_state
        self.warm_start = False
        self.iter_block = int(iter_block)

    # ---- host-side checks -------------------------------------------------------------------------------------------
    def _check_init(self, d):
        """sklearn's checks of the ``*_init`` arrays; returns them as float64 numpy arrays (or None)"""
        k, code = self.n_components, _COV[self.covariance_type]
        w = mu = prec = None
        if self.weights_init is not None:
            w = np.array(self.weights_init, dtype=np.float64)
            if w.shape != (k,):
                raise ValueError("weights_init must have shape (%d,), got %s" % (k, w.shape))
            if np.any(w < 0.0) or np.any(w > 1.0) or not np.allclose(np.abs(1.0 - np.sum(w)), 0.0):
                raise ValueError("weights_init must lie in [0, 1] and sum to 1")
        if self.means_init is not None:
            mu = np.array(self.means_init, dtype=np.float64)
            if mu.shape != (k, d):
                raise ValueError("means_init must have shape (%d, %d), got %s" % (k, d, mu.shape))
        if self.precisions_init is not None:
            prec = np.array(self.precisions_init, dtype=np.float64)
            if prec.shape != _param_shape(k, d, code):
                raise ValueError("precisions_init must have shape %s, got %s" % (_param_shape(k, d, code), prec.shape))
            if code == 0:
                for p in prec:
                    if not (np.allclose(p, p.T) and np.all(np.linalg.eigvalsh(p) > 0.0)):
                        raise ValueError("'full' precisions_init must be symmetric, positive-definite")
            elif np.any(prec <= 0.0):
                raise ValueError("'diag' precisions_init must be positive")
        for a in (w, mu, prec):
            if a is not None and not np.isfinite(a).all():
                raise ValueError("the initial parameters contain NaN or infinity")
        return w, mu, prec

    def _n_parameters(self, d):
        k = self.n_components
        cov = k * d * (d + 1) // 2 if self.covariance_type == 'full' else k * d
        return int(cov + d * k + k - 1)

    # ---- the start --------------------------------------------------------------------------------------------------
    def _initialize(self, Xd, rs, w0, mu0, prec0, ws):
        """sklearn's ``_initialize_parameters`` / ``_initialize``: the device tensors (weights, means, covariances,
        precisions_cholesky, log_det)"""
        dev = Xd.device
        n, d = Xd.shape
        k, code = self.n_components, _COV[self.covariance_type]
        weights = means = cov = pchol = log_det = None
        if w0 is None or mu0 is None or prec0 is None:
            seeds = rs.choice(n, size=k, replace=False)
            if self.init_params == 'kmeans':
                resp = _kmeans(Xd, seeds)[1]
            else:
                resp = torch.zeros((n, k), dtype=torch.float64, device=dev)
                resp[torch.as_tensor(seeds, device=dev), torch.arange(k, device=dev)] = 1.0
            if prec0 is None:
                weights, means, cov, pchol, log_det = _m_step(Xd, resp, self.reg_covar, code, ws)
            else:
                weights = torch.empty(k, dtype=torch.float64, device=dev)
                means = torch.empty((k, d), dtype=torch.float64, device=dev)
                nk = torch.empty(k, dtype=torch.float64, device=dev)
                ws1 = _workspace(n, d, k, 1, dev)
                _lib.check(_lib.load().ava_gm_means(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, resp.data_ptr(),
                                                    weights.data_ptr(), means.data_ptr(), nk.data_ptr(),
                                                    ws1[0].data_ptr(), ws1[1], _lib.stream()), "ava_gm_means")
        if w0 is not None:
            weights = torch.from_numpy(w0).to(dev)
        if mu0 is not None:
            means = torch.from_numpy(mu0).to(dev)
        if prec0 is not None:
            if code == 0:               # _compute_precision_cholesky_from_precisions: flipped Cholesky factors
                ph = np.array([np.linalg.cholesky(p[::-1, ::-1])[::-1, ::-1] for p in prec0])
            else:
                ph = np.sqrt(prec0)
            pchol = torch.from_numpy(np.ascontiguousarray(ph)).to(dev)
            log_det = torch.from_numpy(_log_det(ph, code)).to(dev)
            cov = torch.zeros(_param_shape(k, d, code), dtype=torch.float64, device=dev)
        return [weights.contiguous(), means.contiguous(), cov, pchol, log_det]

    def _em(self, Xd, params, ws):
        """the EM loop from ``params`` (advanced in place): (converged, n_iter, lower bounds)"""
        lib = _lib.load()
        dev = Xd.device
        n, d = Xd.shape
        k, code = self.n_components, _COV[self.covariance_type]
        ctl = torch.zeros(3 + self.max_iter, dtype=torch.int32, device=dev)
        bounds = torch.zeros(self.max_iter, dtype=torch.float64, device=dev)
        lpn = torch.empty(n, dtype=torch.float64, device=dev)
        log_resp = torch.empty((n, k), dtype=torch.float64, device=dev)
        resp = torch.empty((n, k), dtype=torch.float64, device=dev)
        weights, means, cov, pchol, log_det = params
        stopped = False
        for it0 in range(0, self.max_iter, self.iter_block):
            n_iters = min(self.iter_block, self.max_iter - it0)
            _lib.check(lib.ava_gm_fit(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, code, weights.data_ptr(),
                                      means.data_ptr(), cov.data_ptr(), pchol.data_ptr(), log_det.data_ptr(), self.tol,
                                      self.reg_covar, it0, n_iters, bounds.data_ptr(), ctl.data_ptr(), lpn.data_ptr(),
                                      log_resp.data_ptr(), resp.data_ptr(), ws[0].data_ptr(), ws[1], _lib.stream()),
                       "ava_gm_fit")
            host = ctl.cpu().numpy()                       # the only host read of a block
            if host[0] != 0:
                raise ValueError(_ILL_DEFINED)
            stopped = bool(host[2 + it0 + n_iters])
            if stopped:
                break
        n_iter = int(host[1])
        return stopped, n_iter, bounds[:n_iter].cpu().numpy()

    # ---- sklearn's interface ----------------------------------------------------------------------------------------
    def fit(self, X, y=None):
        X = _check_rows(X, self.n_components)
        n, d = X.shape
        w0, mu0, prec0 = self._check_init(d)
        dev = _device()
        Xd = _rows.upload(X, dev)
        code = _COV[self.covariance_type]
        ws = _workspace(n, d, self.n_components, code, dev)
        rs = _random_state(self.random_state)
        best = None
        for _ in range(self.n_init):
            params = self._initialize(Xd, rs, w0, mu0, prec0, ws)
            converged, n_iter, bounds = self._em(Xd, params, ws)
            if best is None or bounds[-1] > best[3][-1]:
                best = (params, converged, n_iter, bounds)
        params, self.converged_, self.n_iter_, bounds = best
        self._params = params
        self.lower_bounds_ = [float(b) for b in bounds]
        self.lower_bound_ = self.lower_bounds_[-1]
        self.weights_, self.means_, self.covariances_, self.precisions_cholesky_ = (p.cpu().numpy() for p in params[:4])
        if code == 0:
            self.precisions_ = np.array([p @ p.T for p in self.precisions_cholesky_])
        else:
            self.precisions_ = self.precisions_cholesky_ ** 2
        self.n_features_in_ = d
        return self

    def _estimate(self, X):
        if not hasattr(self, "_params"):
            raise ValueError("this GaussianMixture is not fitted yet")
        X = _check_rows(X, 1)
        if X.shape[1] != self.n_features_in_:
            raise ValueError("X has %d features, the model was fitted with %d" % (X.shape[1], self.n_features_in_))
        Xd = _rows.upload(X, self._params[0].device)
        weights, means, _, pchol, log_det = self._params
        return _e_step(Xd, weights, means, pchol, log_det, _COV[self.covariance_type])

    def fit_predict(self, X, y=None):
        return self.fit(X).predict(X)

    def predict(self, X):
        return self._estimate(X)[1].argmax(dim=1).cpu().numpy().astype(np.int64)

    def predict_proba(self, X):
        return self._estimate(X)[2].cpu().numpy()

    def score_samples(self, X):
        return self._estimate(X)[0].cpu().numpy()

    def score(self, X, y=None):
        return float(self.score_samples(X).mean())

    def bic(self, X):
        n = X.shape[0]
        return -2.0 * self.score(X) * n + self._n_parameters(self.n_features_in_) * np.log(n)

    def aic(self, X):
        return -2.0 * self.score(X) * X.shape[0] + 2.0 * self._n_parameters(self.n_features_in_)
