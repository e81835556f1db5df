"""Trustworthiness, continuity and preserved neighbours of a projection on the MI355X: how
far a 2-D picture (``projection.UMAP``, ``projection.pca_projection``, ``tsne.TSNE``) keeps the neighbourhoods of the rows
it was made from, or how far two feature spaces of the same rows agree.

The reference package has no counterpart: the specification of :func:`trustworthiness` is scikit-learn 1.7's
``sklearn.manifold.trustworthiness``; continuity (Venna & Kaski) is the same quantity with the spaces exchanged, and
``Q_NX(k)`` / ``LCMC(k)`` are the preserved-neighbour share of the co-ranking literature.  sklearn builds the N x N
distance matrix, its full ``argsort`` and an N x N inverted index; here a rank is a count over one sweep of the fp64
distance tile (``csrc/embed_quality.hip``) and nothing of size N x N exists.

Definitions, for n rows in two spaces X [n, d] and Y [n, e], both under the euclidean metric:

* ``(d2(i, l), l)`` comes before ``(d2(i, j), j)`` when ``d2(i, l) < d2(i, j)``, or when they are equal and ``l < j``;
* ``r_X(i, j) = 1 + #{l != i : (d2_X(i, l), l) before (d2_X(i, j), j)}``: 1 .. n - 1;
* ``N_k^Y(i)``: the k nearest other rows of i in Y, columns 1 .. k of ``projection.knn(Y, k + 1)``;
* ``P_T(k) = sum_i sum_{j in N_k^Y(i)} max(0, r_X(i, j) - k)``, an exact integer, and
  ``T(k) = 1 - P_T(k) * (2 / (n k (2 n - 3 k - 1)))``; ``C(k)`` is ``T(k)`` of ``(Y, X)``;
* ``Q_NX(k) = (1 / (n k)) sum_i |N_k^X(i) and N_k^Y(i)|`` and ``LCMC(k) = Q_NX(k) - k / (n - 1)``.

=====================================  =====================================  ======================
quantity                               here                                   C entry point
=====================================  =====================================  ======================
``r_X(i, j)`` of listed rows           :func:`neighbor_ranks`                 ``ava_eq_ranks``
``T(k)``                               :func:`trustworthiness`                ``ava_pj_knn``, ``ava_eq_ranks``,
``C(k)``                               :func:`continuity`                     ``ava_eq_penalties``
``Q_NX(k)``                            :func:`neighborhood_preservation`      ``ava_pj_knn``, ``ava_eq_overlap``
all of them over a sweep of k          :func:`quality_curve`                  the above, once at ``max(ks)``
the per-row values                     :func:`local_quality`
several projections of the same rows   :func:`compare_projections`
=====================================  =====================================  ======================

Deviations from scikit-learn, on purpose:

* distances are direct differences ``sum_c fma(x_c - y_c, x_c - y_c, .)`` in fp64 and stay squared (the tile of
  ``csrc/sqdist_tile.h``); sklearn expands ``|x|^2 + |y|^2 - 2 x.y`` and takes the root;
* ties are ordered by index, where sklearn leaves them to an unstable ``argsort`` and to ``NearestNeighbors``: every
  count is a function of the data alone, the same on every run and for every launch shape;
* rows may be float32 or float64 and are read into fp64: float32 rows and their float64 copy give the same integers.

Each scalar is evaluated with sklearn's own expression from the exact integer, so where no two distances of a row are
within rounding of each other it equals sklearn's float bit for bit (tests/golden/embed_quality.npz).  ``k`` is at most
``MAX_NEIGHBORS`` = 63 (a kNN list of ``projection.MAX_K`` without its self column) and, as in sklearn, below ``n / 2``.
There is no CPU fallback: without the HIP library / a GPU every device function raises ``AvaHipError``.
"""
import ctypes
import numbers

import numpy as np
import torch

from . import _lib, _rows
from . import projection as _pj

__all__ = ["trustworthiness", "continuity", "neighborhood_preservation", "neighbor_ranks", "quality_curve",
           "local_quality", "compare_projections", "MAX_NEIGHBORS", "MAX_SWEEP"]
MAX_NEIGHBORS = _pj.MAX_K - 1   # ava_eq_max_targets
MAX_SWEEP = 16                  # ava_eq_max_sweep
MAX_N = 2 ** 31 - 65            # ava_eq_ranks: n < 2^31 - 64


def _device():
    return _lib.device("embedding-quality")


# ---- argument checks (no device) -------------------------------------------------------------------------------------
def _check_rows(X, what):
    X = _rows.native(X.detach() if torch.is_tensor(X) else X)
    shape = tuple(X.shape)
    if len(shape) != 2:
        raise ValueError("Expected 2D array, got %dD array instead (%s)" % (len(shape), what))
    if shape[0] < 2 or shape[1] < 1:
        raise ValueError("%s has %d row(s) and %d feature(s): at least 2 rows and 1 feature are required"
                         % (what, shape[0], shape[1]))
    if shape[0] > MAX_N:
        raise ValueError("unsupported shape: N = %d rows, at most %d" % (shape[0], MAX_N))
    if shape[1] > _pj.MAX_DIM:
        raise ValueError("unsupported shape: d = %d features, at most %d" % (shape[1], _pj.MAX_DIM))
    if _rows.has_nan(X):
        raise ValueError("Input %s contains NaN." % what)
    if not _rows.is_finite(X):
        raise ValueError("Input %s contains infinity or a value too large for dtype('float64')." % what)
    return X


def _check_pair(X, Y, names=("X", "X_embedded")):
    X, Y = _check_rows(X, names[0]), _check_rows(Y, names[1])
    if X.shape[0] != Y.shape[0]:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]"
                         % (X.shape[0], Y.shape[0]))
    return X, Y


def _check_k(k, n):
    if not isinstance(k, numbers.Integral) or isinstance(k, bool) or k < 1:
        raise ValueError("n_neighbors must be an int in the range [1, inf). Got %r instead." % (k,))
    if k >= n / 2:
        raise ValueError("n_neighbors (%d) should be less than n_samples / 2 (%s)" % (k, n / 2))
    if k > MAX_NEIGHBORS:
        raise ValueError("n_neighbors = %d: the device path holds at most %d" % (k, MAX_NEIGHBORS))
    return int(k)


def _check_ks(ks, n):
    ks = [ks] if isinstance(ks, numbers.Integral) else list(ks)
    if not 1 <= len(ks) <= MAX_SWEEP:
        raise ValueError("ks must hold 1 to %d values, got %d" % (MAX_SWEEP, len(ks)))
    return [_check_k(k, n) for k in ks]


def _check_metric(metric):
    if metric != 'euclidean':
        raise NotImplementedError("metric=%r: only 'euclidean' is on the device" % (metric,))


# ---- device steps ----------------------------------------------------------------------------------------------------
def _neighbours_device(xd, m):
    """[n, m] int64: every row's m nearest other rows by (distance, index)"""
    idx, _ = _pj._knn_device(xd, m + 1)
    return idx[:, 1:].contiguous()


def _ranks_device(xd, tgt, col_splits=0):
    """[n, m] int32 (device): the rank among the rows of ``xd`` of every target"""
    lib = _lib.load()
    n, d, m = int(xd.shape[0]), int(xd.shape[1]), int(tgt.shape[1])
    nbytes = lib.ava_eq_workspace_bytes(n, m)
    ws = _lib.workspace(nbytes, xd.device, "N = %d rows, %d targets a row" % (n, m))
    rank = torch.empty((n, m), dtype=torch.int32, device=xd.device)
    _lib.check(lib.ava_eq_ranks(xd.data_ptr(), _lib.dtype_code(xd), n, d, tgt.data_ptr(), m, int(col_splits),
                                rank.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "ava_eq_ranks")
    return rank


def _sweep(ks):
    return (ctypes.c_int * len(ks))(*ks)


def _penalties_device(rank, ks):
    """(pen [n, n_k] int64, totals [n_k] int64) on the device"""
    n, m = int(rank.shape[0]), int(rank.shape[1])
    pen = torch.empty((n, len(ks)), dtype=torch.int64, device=rank.device)
    tot = torch.empty(len(ks), dtype=torch.int64, device=rank.device)
    _lib.check(_lib.load().ava_eq_penalties(rank.data_ptr(), n, m, _sweep(ks), len(ks), pen.data_ptr(), tot.data_ptr(),
                                            _lib.stream()), "ava_eq_penalties")
    return pen, tot


def _overlap_device(na, nb, ks):
    """(overlap [n, n_k] int32, totals [n_k] int64) on the device"""
    n, m = int(na.shape[0]), int(na.shape[1])
    ov = torch.empty((n, len(ks)), dtype=torch.int32, device=na.device)
    tot = torch.empty(len(ks), dtype=torch.int64, device=na.device)
    _lib.check(_lib.load().ava_eq_overlap(na.data_ptr(), nb.data_ptr(), n, m, _sweep(ks), len(ks), ov.data_ptr(),
                                          tot.data_ptr(), _lib.stream()), "ava_eq_overlap")
    return ov, tot


def _scalar(t, n, k):
    """sklearn's expression, from the exact integer"""
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def _trust_device(xd, ny, ks):
    """(per-row penalties [n, n_k], their totals as Python ints) of the neighbours ``ny`` [n, max(ks)] ranked in ``xd``"""
    pen, tot = _penalties_device(_ranks_device(xd, ny), ks)
    return pen, [int(t) for t in tot.cpu().numpy()]


def _upload_pair(X, Y):
    dev = _device()
    return _rows.upload(X, dev), _rows.upload(Y, dev)


# ---- public functions ------------------------------------------------------------------------------------------------
def trustworthiness(X, X_embedded, *, n_neighbors=5, metric='euclidean'):
    """sklearn's ``trustworthiness(X, X_embedded, n_neighbors=...)``: how far the ``n_neighbors`` nearest rows of every
    row in the embedding are near it in ``X`` too; 1 when every one of them is among its ``n_neighbors`` nearest there."""
    _check_metric(metric)
    X, Y = _check_pair(X, X_embedded)
    n = X.shape[0]
    k = _check_k(n_neighbors, n)
    xd, yd = _upload_pair(X, Y)
    _, tot = _trust_device(xd, _neighbours_device(yd, k), [k])
    return _scalar(tot[0], n, k)


def continuity(X, X_embedded, *, n_neighbors=5):
    """Venna & Kaski's continuity: the trustworthiness of ``(X_embedded, X)``, how far the neighbours in ``X`` stay
    near in the embedding"""
    X, Y = _check_pair(X, X_embedded)
    k = _check_k(n_neighbors, X.shape[0])
    return trustworthiness(Y, X, n_neighbors=k)


def neighborhood_preservation(A, B, *, n_neighbors=5):
    """``Q_NX(k)``: the mean share of a row's ``n_neighbors`` nearest rows in ``A`` that are among its nearest in ``B``,
    for any two representations of the same rows"""
    A, B = _check_pair(A, B, ("A", "B"))
    n = A.shape[0]
    k = _check_k(n_neighbors, n)
    ad, bd = _upload_pair(A, B)
    _, tot = _overlap_device(_neighbours_device(ad, k), _neighbours_device(bd, k), [k])
    return int(tot[0]) / (n * k)


def neighbor_ranks(X, targets):
    """int32 ``[n, m]``: ``r_X(i, targets[i, s])``, the rank of the listed rows among the other rows of row i (1 the
    nearest).  ``targets`` (integers, ``[n, m]``, ``m <= MAX_NEIGHBORS``) may repeat a row and need not hold neighbours;
    a target outside [0, n) or equal to its row is refused.  A tensor ``X`` gives a device tensor."""
    X = _check_rows(X, "X")
    tensors = torch.is_tensor(X)
    t = targets.detach().cpu().numpy() if torch.is_tensor(targets) else np.asarray(targets)
    if t.ndim != 2 or t.shape[0] != X.shape[0] or not 1 <= t.shape[1] <= MAX_NEIGHBORS or t.dtype.kind not in "iu":
        raise ValueError("targets must be integers of shape [%d, m], 1 <= m <= %d, got %s %s"
                         % (X.shape[0], MAX_NEIGHBORS, t.dtype, t.shape))
    t = t.astype(np.int64)
    if t.min() < 0 or t.max() >= X.shape[0] or bool((t == np.arange(len(t))[:, None]).any()):
        raise ValueError("a target lies outside [0, n) or is its own row")
    dev = _device()
    rank = _ranks_device(_rows.upload(X, dev), _rows.upload(t, dev))
    return rank if tensors else rank.cpu().numpy()


def _curve_device(xd, nx, yd, ks):
    """the curve of the rows ``yd`` against ``xd``, whose neighbour table at max(ks) is ``nx``"""
    n = int(xd.shape[0])
    ny = _neighbours_device(yd, max(ks))
    pen_t, tot_t = _trust_device(xd, ny, ks)
    pen_c, tot_c = _trust_device(yd, nx, ks)
    ov, tot_o = _overlap_device(nx, ny, ks)
    return pen_t, tot_t, pen_c, tot_c, ov, [int(t) for t in tot_o.cpu().numpy()], n


def _curve_dict(res, ks):
    _, tot_t, _, tot_c, _, tot_o, n = res
    q = np.array([t / (n * k) for t, k in zip(tot_o, ks)], dtype=np.float64)
    return {"trustworthiness": np.array([_scalar(t, n, k) for t, k in zip(tot_t, ks)], dtype=np.float64),
            "continuity": np.array([_scalar(t, n, k) for t, k in zip(tot_c, ks)], dtype=np.float64),
            "preservation": q, "lcmc": q - np.asarray(ks, dtype=np.float64) / (n - 1.0)}


def quality_curve(X, Y, ks):
    """a dict of float64 arrays over ``ks``: ``trustworthiness``, ``continuity``, ``preservation`` (Q_NX) and ``lcmc``
    of the rows ``Y`` as a picture of the rows ``X``.  The rows are uploaded once; one kNN pass and one rank pass per
    space at ``max(ks)`` serve the whole sweep, since the list for k' < k is a prefix of the list for k."""
    X, Y = _check_pair(X, Y, ("X", "Y"))
    ks = _check_ks(ks, X.shape[0])
    xd, yd = _upload_pair(X, Y)
    return _curve_dict(_curve_device(xd, _neighbours_device(xd, max(ks)), yd, ks), ks)


def local_quality(X, Y, n_neighbors=5):
    """the per-row values at ``n_neighbors``, for colouring a scatter: ``trustworthiness`` and ``continuity`` (float64
    ``[n]``, the scalar's expression with the row's own penalty; their means are the scalars) and ``overlap`` (int32
    ``[n]``, ``|N_k^X(i) and N_k^Y(i)|``)"""
    X, Y = _check_pair(X, Y, ("X", "Y"))
    n = X.shape[0]
    k = _check_k(n_neighbors, n)
    xd, yd = _upload_pair(X, Y)
    pen_t, _, pen_c, _, ov, _, _ = _curve_device(xd, _neighbours_device(xd, k), yd, [k])
    f = 2.0 / (k * (2.0 * n - 3.0 * k - 1.0))
    return {"trustworthiness": 1.0 - pen_t[:, 0].cpu().numpy() * f, "continuity": 1.0 - pen_c[:, 0].cpu().numpy() * f,
            "overlap": ov[:, 0].cpu().numpy()}


def compare_projections(X, embeddings, ks):
    """``{name: quality_curve(X, embeddings[name], ks)}`` for a dict of ``[n, e]`` pictures of the same rows (the outputs
    of ``UMAP``, ``pca_projection``, ``TSNE``, ...): X is uploaded and its kNN table made once for all of them."""
    X = _check_rows(X, "X")
    ks = _check_ks(ks, X.shape[0])
    checked = {name: _check_pair(X, Y, ("X", "embeddings[%r]" % (name,)))[1] for name, Y in dict(embeddings).items()}
    if not checked:
        return {}
    dev = _device()
    xd = _rows.upload(X, dev)
    nx = _neighbours_device(xd, max(ks))
    return {name: _curve_dict(_curve_device(xd, nx, _rows.upload(Y, dev), ks), ks) for name, Y in checked.items()}
