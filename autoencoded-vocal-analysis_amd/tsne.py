"""Exact t-SNE on the MI355X: the layout step of the reference's ``mmd_tsne_plot_DC``.

``mmd_tsne_plot_DC`` (ava/plotting/mmd_plots.py:171-252) lays the conditions out with ``TSNE(n_components=2,
random_state=42, metric='precomputed', method='exact', perplexity=perplexity)`` on the MMD^2 matrix.  With
scikit-learn 1.7 that call raises ``ValueError`` (``init`` defaults to ``'pca'``, which ``metric='precomputed'``
forbids).  :class:`TSNE` here takes the same call and runs scikit-learn 1.7's exact path on the device, with the HIP
kernels of ``csrc/tsne.hip``:

=====================================  =====================================  ======================
scikit-learn 1.7 (manifold/_t_sne.py)  here                                   C entry point
=====================================  =====================================  ======================
``pairwise_distances`` / ``**= 2``     :func:`squared_distances`              ``ava_ts_sqdist`` / ``ava_ts_square``
``_joint_probabilities``               :func:`joint_probabilities`            ``ava_ts_joint``
``_kl_divergence``                     :func:`kl_gradient`                    ``ava_ts_kl_gradient``
``_gradient_descent`` (iterations)     :func:`descend`                        ``ava_ts_descend``
``_gradient_descent`` (checks),        :func:`schedule`                       (host only)
``TSNE._tsne``
=====================================  =====================================  ======================

Deviations from scikit-learn, on purpose: positions, gradient, gains and update are fp64 throughout
(sklearn holds them in float32 when the init is float32); euclidean squared distances are direct differences, not the
``|x|^2 + |y|^2 - 2xy`` expansion; every sum runs in this project's fixed orders; only ``n_components=2``,
``method='exact'``, the metrics ``'euclidean'`` and ``'precomputed'`` and a random or array init are there;
``kl_divergence_`` is the KL of the returned positions (sklearn's is that of the positions one update earlier).  A whole
run is therefore not comparable point by point with sklearn's (the descent amplifies a rounding difference to the size
of the layout within 100 iterations); each step is.

There is no CPU fallback: without the HIP library / a GPU every device function raises ``AvaHipError``.
"""
import numpy as np
import torch

from . import _lib, _rows

__all__ = ["TSNE", "squared_distances", "joint_probabilities", "kl_gradient", "descend", "schedule", "MAX_N",
           "N_ITER_CHECK", "EXPLORATION_MAX_ITER"]
MAX_N = 32768                   # P takes 8.6 GB there (ava_ts_max_n)
N_ITER_CHECK = 50               # TSNE._N_ITER_CHECK
EXPLORATION_MAX_ITER = 250      # TSNE._EXPLORATION_MAX_ITER


def _device():
    return _lib.device("t-SNE")


def _matrix(n, dev):
    """an ``[n, n]`` float64 view whose rows start on 16-byte boundaries (row stride ``n`` rounded up to even)"""
    return torch.empty((n, n + (n & 1)), dtype=torch.float64, device=dev)[:, :n]


def _as_matrix(M):
    """``M`` itself if the kernels can read it (float64, unit column stride, even row stride, 16-byte base), else a
    copy that they can"""
    if M.dim() != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("expected a square matrix, got shape %s" % (tuple(M.shape),))
    n = M.shape[0]
    if not 2 <= n <= MAX_N:
        raise ValueError("t-SNE needs 2 <= N <= %d rows, got %d" % (MAX_N, n))
    ok = (M.dtype == torch.float64 and M.is_cuda and M.stride(1) == 1 and M.stride(0) >= n and M.stride(0) % 2 == 0
          and M.data_ptr() % 16 == 0)
    if ok:
        return M
    out = _matrix(n, _device())
    out.copy_(M)
    return out


def _workspace(n, col_chunks, dev):
    nbytes = _lib.load().ava_ts_workspace_bytes(n, 0 if col_chunks is None else int(col_chunks))
    if nbytes == 0:
        raise ValueError("unsupported N = %d or col_chunks = %r" % (n, col_chunks))
    return _lib.workspace(nbytes, dev, "t-SNE"), nbytes


def _pairs(t, n, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.shape == (n, 2)
            and t.is_contiguous()):
        raise ValueError("%s must be a contiguous float64 [%d, 2] tensor on the device" % (what, n))
    return t


def squared_distances(X, metric='euclidean', round_float32=True):
    """The ``[N, N]`` float64 matrix of squared distances that sklearn's exact path hands to
    ``_joint_probabilities``, on the device.

    ``metric='euclidean'``: ``X`` is ``[N, d]`` float32 or float64 rows; every entry has the bits of
    ``ava_pair_sqdist`` (direct differences, csrc/sqdist_tile.h).  ``metric='precomputed'``: ``X`` is an ``[N, N]``
    distance matrix, which is squared as sklearn 1.7 does for every metric but ``'euclidean'``.  Every entry is then
    rounded to the nearest float32 (sklearn's ``distances.astype(np.float32)``); ``round_float32=False`` keeps the
    euclidean sums as they are."""
    dev = _device()
    lib = _lib.load()
    if metric == 'euclidean':
        t = _rows.upload(_rows.native(X), dev)
        if t.dim() != 2 or not 1 <= t.shape[1] <= 65536:
            raise ValueError("X must be [N, d] with 1 <= d <= 65536")
        n, d = t.shape
        if not 2 <= n <= MAX_N:
            raise ValueError("t-SNE needs 2 <= N <= %d rows, got %d" % (MAX_N, n))
        out = _matrix(n, dev)
        _lib.check(lib.ava_ts_sqdist(t.data_ptr(), _lib.dtype_code(t), n, d, int(bool(round_float32)), out.data_ptr(),
                                     out.stride(0), _lib.stream()), "ava_ts_sqdist")
        return out
    if metric == 'precomputed':
        t = X if torch.is_tensor(X) else np.asarray(X)
        if t.ndim != 2 or t.shape[0] != t.shape[1]:
            raise ValueError("a precomputed distance matrix must be square, got shape %s" % (tuple(t.shape),))
        n = t.shape[0]
        if not 2 <= n <= MAX_N:
            raise ValueError("t-SNE needs 2 <= N <= %d rows, got %d" % (MAX_N, n))
        t = _rows.upload(t, dev, torch.float64)
        out = _matrix(n, dev)
        _lib.check(lib.ava_ts_square(t.data_ptr(), n, out.data_ptr(), out.stride(0), _lib.stream()), "ava_ts_square")
        return out
    raise NotImplementedError("metric %r: only 'euclidean' and 'precomputed' are on the device" % (metric,))


def joint_probabilities(D2, perplexity):
    """sklearn's ``_joint_probabilities`` as a square matrix: ``D2`` (from :func:`squared_distances`) is OVERWRITTEN
    with P -- symmetric, zero diagonal, sum 1, every other entry at least ``DBL_EPSILON`` -- and returned."""
    _device()
    P = _as_matrix(D2)
    n = P.shape[0]
    if not 0 < perplexity < n:
        raise ValueError("perplexity (%r) must be positive and less than n_samples (%d)" % (perplexity, n))
    ws, nbytes = _workspace(n, None, P.device)
    _lib.check(_lib.load().ava_ts_joint(P.data_ptr(), P.stride(0), n, float(perplexity), ws.data_ptr(), nbytes,
                                        _lib.stream()), "ava_ts_joint")
    return P


def kl_gradient(Y, P, exaggeration=1.0, col_chunks=None):
    """sklearn's ``_kl_divergence`` at the positions ``Y`` (float64 ``[N, 2]`` on the device) with ``P`` scaled by
    ``exaggeration``: ``(kl, grad)``, ``kl`` a float and ``grad`` a float64 ``[N, 2]`` device tensor.  ``col_chunks``
    (default: a function of N alone) splits the columns of every row among that many workgroups; the partial sums are
    added in ascending order."""
    _device()
    P = _as_matrix(P)
    n = P.shape[0]
    Y = _pairs(Y, n, "Y")
    ws, nbytes = _workspace(n, col_chunks, P.device)
    grad = torch.empty((n, 2), dtype=torch.float64, device=P.device)
    stats = torch.empty(2, dtype=torch.float64, device=P.device)
    _lib.check(_lib.load().ava_ts_kl_gradient(Y.data_ptr(), P.data_ptr(), P.stride(0), n, float(exaggeration),
                                              0 if col_chunks is None else int(col_chunks), grad.data_ptr(),
                                              stats.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()),
               "ava_ts_kl_gradient")
    return float(stats[0].item()), grad


def _descend(Y, update, gains, P, n_iters, momentum, lr, exaggeration, col_chunks, ws, nbytes):
    """enqueue ``n_iters`` iterations; returns the device tensor ``[n_iters, 2]`` of ``{KL, |grad gains|}`` (the KL
    of the last iteration only: the others are NaN, as with sklearn's ``compute_error=False``)"""
    stats = torch.empty((n_iters, 2), dtype=torch.float64, device=P.device)
    _lib.check(_lib.load().ava_ts_descend(Y.data_ptr(), update.data_ptr(), gains.data_ptr(), P.data_ptr(), P.stride(0),
                                          P.shape[0], int(n_iters), float(momentum), float(lr), float(exaggeration),
                                          0 if col_chunks is None else int(col_chunks), stats.data_ptr(),
                                          ws.data_ptr(), nbytes, _lib.stream()), "ava_ts_descend")
    return stats


def descend(Y, update, gains, P, n_iters, momentum, lr, exaggeration, col_chunks=None):
    """``n_iters`` iterations of sklearn's ``_gradient_descent`` on the device, enqueued without a host
    synchronisation: ``Y``, ``update`` and ``gains`` (float64 ``[N, 2]`` device tensors) advance IN PLACE.  Returns
    ``(kl, grad_norm)`` of the last iteration: the KL divergence at the positions it started from and the norm of its
    gradient times the gains, as sklearn's check takes them."""
    _device()
    P = _as_matrix(P)
    n = P.shape[0]
    for t, what in ((Y, "Y"), (update, "update"), (gains, "gains")):
        _pairs(t, n, what)
    if n_iters < 1:
        raise ValueError("n_iters must be at least 1")
    ws, nbytes = _workspace(n, col_chunks, P.device)
    last = _descend(Y, update, gains, P, n_iters, momentum, lr, exaggeration, col_chunks, ws, nbytes)[-1].cpu()
    return float(last[0]), float(last[1])


def _phase(run, it, max_iter, n_iter_without_progress, min_grad_norm, exaggeration, momentum):
    """one call of sklearn's ``_gradient_descent`` from iteration ``it``: ``(error, last iteration)``"""
    error = best_error = np.finfo(float).max
    best_iter = i = it
    nxt = it
    while nxt < max_iter:
        i = min((nxt // N_ITER_CHECK + 1) * N_ITER_CHECK, max_iter) - 1       # the next check, or the last iteration
        error, grad_norm = run(i - nxt + 1, exaggeration, momentum)
        nxt = i + 1
        if (i + 1) % N_ITER_CHECK == 0:
            if error < best_error:
                best_error = error
                best_iter = i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
    return error, i


def schedule(run, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, early_exaggeration=12.0):
    """The host half of ``TSNE._tsne`` and ``_gradient_descent``: which iterations run under which momentum and
    exaggeration, and when a phase stops.  ``run(n_iters, exaggeration, momentum) -> (kl, grad_norm)`` advances the
    descent by ``n_iters`` iterations and returns the two scalars of the last of them; this function owns no device
    state and reads nothing else.  Returns ``(kl_divergence, n_iter)`` as sklearn's ``kl_divergence_`` and ``n_iter_``.

    Phase 1: iterations 0 .. 249, momentum 0.5, the early exaggeration, ``n_iter_without_progress`` 250.  Phase 2: from
    the next iteration to ``max_iter``, momentum 0.8, exaggeration 1.  At every iteration ``i`` with ``(i + 1) % 50 ==
    0`` the KL of that iteration is compared with the phase's best (stop when ``i - best_iter >
    n_iter_without_progress``), and the phase stops when the gradient norm is ``<= min_grad_norm``."""
    kl, it = _phase(run, 0, EXPLORATION_MAX_ITER, EXPLORATION_MAX_ITER, min_grad_norm, early_exaggeration, 0.5)
    if it < EXPLORATION_MAX_ITER or max_iter - EXPLORATION_MAX_ITER > 0:
        kl, it = _phase(run, it + 1, max_iter, n_iter_without_progress, min_grad_norm, 1.0, 0.8)
    return kl, it


class TSNE:
    """scikit-learn 1.7's ``TSNE(method='exact', n_components=2)`` on the device.

    ``fit`` / ``fit_transform`` take ``[N, d]`` rows (``metric='euclidean'``) or an ``[N, N]`` distance matrix
    (``metric='precomputed'``; it is squared, like sklearn 1.7 does), numpy or torch.  Attributes after a fit:
    ``embedding_`` (float32 ``[N, 2]`` numpy), ``kl_divergence_``, ``n_iter_``, ``learning_rate_``.  ``init`` is
    ``'random'`` (sklearn's draw: ``1e-4 * RandomState(random_state).standard_normal((N, 2)).astype(float32)``) or an
    ``[N, 2]`` array.  Keywords sklearn has and this class does not use (``verbose``, ``n_jobs``, ``angle`` ...) are
    accepted and ignored."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, metric='euclidean', init='random',
                 random_state=None, method='exact', **ignored):
        if n_components != 2:
            raise NotImplementedError("n_components=%r: only 2 components are on the device" % (n_components,))
        if method != 'exact':
            raise NotImplementedError("method=%r: only the exact method is on the device" % (method,))
        if metric not in ('euclidean', 'precomputed'):
            raise NotImplementedError("metric %r: only 'euclidean' and 'precomputed' are on the device" % (metric,))
        if isinstance(init, str) and init != 'random':
            raise NotImplementedError("init=%r: only 'random' or an [N, 2] array" % (init,))
        if max_iter < EXPLORATION_MAX_ITER:
            raise ValueError("max_iter must be at least %d, got %r" % (EXPLORATION_MAX_ITER, max_iter))
        if not (learning_rate == 'auto' or float(learning_rate) > 0):
            raise ValueError("learning_rate must be 'auto' or positive, got %r" % (learning_rate,))
        if not (perplexity > 0 and early_exaggeration >= 1):
            raise ValueError("perplexity must be positive and early_exaggeration at least 1")
        self.n_components = n_components
        self.perplexity = perplexity
        self.early_exaggeration = early_exaggeration
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.n_iter_without_progress = n_iter_without_progress
        self.min_grad_norm = min_grad_norm
        self.metric = metric
        self.init = init
        self.random_state = random_state
        self.method = method

    def _check(self, X):
        """host-side checks of the input; returns it as it goes to the device"""
        X = _rows.native(X)
        shape, finite = tuple(X.shape), _rows.is_finite(X)
        negative = self.metric == 'precomputed' and bool((X < 0).any())
        if len(shape) != 2:
            raise ValueError("expected a 2-D array, got shape %s" % (shape,))
        if self.metric == 'precomputed' and shape[0] != shape[1]:
            raise ValueError("a precomputed distance matrix must be square, got shape %s" % (shape,))
        if not finite:
            raise ValueError("the input contains NaN or infinity")
        if negative:
            raise ValueError("a precomputed distance matrix must not contain negative distances")
        n = shape[0]
        if n > MAX_N:
            raise ValueError("N = %d rows: the device path holds at most MAX_N = %d" % (n, MAX_N))
        if self.perplexity >= n:
            raise ValueError("perplexity (%r) must be less than n_samples (%d)" % (self.perplexity, n))
        if not isinstance(self.init, str) and \
                tuple(self.init.shape if hasattr(self.init, "shape") else np.shape(self.init)) != (n, 2):
            raise ValueError("init must be 'random' or an array of shape (%d, 2)" % n)
        return X

    def _start(self, n):
        if isinstance(self.init, str):
            rs = self.random_state if isinstance(self.random_state, np.random.RandomState) \
                else np.random.RandomState(self.random_state)
            return (1e-4 * rs.standard_normal(size=(n, 2)).astype(np.float32)).astype(np.float64)
        init = self.init.detach().cpu().numpy() if torch.is_tensor(self.init) else np.asarray(self.init)
        return np.ascontiguousarray(init, dtype=np.float64)

    def fit(self, X, y=None):
        X = self._check(X)
        dev = _device()
        P = joint_probabilities(squared_distances(X, self.metric), self.perplexity)
        n = P.shape[0]
        if self.learning_rate == 'auto':
            self.learning_rate_ = max(n / self.early_exaggeration / 4, 50)
        else:
            self.learning_rate_ = float(self.learning_rate)
        Y = torch.from_numpy(self._start(n)).to(dev)
        update = torch.zeros_like(Y)
        gains = torch.ones_like(Y)
        ws, nbytes = _workspace(n, None, dev)

        def run(n_iters, exaggeration, momentum):
            stats = _descend(Y, update, gains, P, n_iters, momentum, self.learning_rate_, exaggeration, None, ws,
                             nbytes)
            last = stats[-1].cpu()                        # the only host read between two checks
            return float(last[0]), float(last[1])

        _, self.n_iter_ = schedule(run, self.max_iter, self.n_iter_without_progress, self.min_grad_norm,
                                   self.early_exaggeration)
        # the KL of the positions that are returned; sklearn reports that of the positions before the last update
        self.kl_divergence_ = kl_gradient(Y, P)[0]
        self.embedding_ = Y.cpu().numpy().astype(np.float32)
        return self

    def fit_transform(self, X, y=None):
        return self.fit(X).embedding_
