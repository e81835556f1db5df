"""MMD^2 between conditions on the MI355X.

Host-side mirror of the estimator functions of the reference's ``ava/plotting/mmd_plots.py`` -- same names, same
arguments, same random-number use and error behaviour -- with the O(n^2) Python double loops replaced by the HIP
kernels of ``csrc/mmd.hip`` (fp64, like the reference's numpy arithmetic):

=============================  ==========================================  =============================
reference (mmd_plots.py)       here                                        C entry point
=============================  ==========================================  =============================
``estimate_median_sigma``      :func:`estimate_median_sigma`  (:450-474)   ``ava_pair_sqdist``
``_estimate_mmd2``             :func:`_estimate_mmd2`         (:255-296)   ``ava_mmd2``
``_estimate_mmd2_linear_time`` :func:`_estimate_mmd2_linear_time` (:299-312) ``ava_mmd2_linear``
loop of ``_calculate_mmd2``    :func:`mmd2_matrix`            (:395-418)   the above per condition pair
the same loop, in one pass     :func:`mmd2_matrix_one_pass`                ``ava_mmd2_matrix`` / ``_linear``
``_calculate_mmd2``            :func:`_calculate_mmd2`        (:337-434)   the one-pass matrix
=============================  ==========================================  =============================

``install()`` swaps the three estimator functions of an imported ``ava.plotting.mmd_plots`` for these, so the
reference's plotting functions (``mmd_matrix_plot_DC`` ...) run unchanged on top of them; ``install(matrix=True)`` also
swaps ``_calculate_mmd2``, so that the whole condition-by-condition matrix is one launch sequence (every block sum of
the sorted index list at once, each within-set term once) instead of a host loop over the pairs.  There is no CPU fallback:
without the HIP library / a GPU every function raises ``AvaHipError``.
"""
import numpy as np
import torch

from . import _lib

EPSILON = 1e-8          # ava/plotting/mmd_plots.py:34

__all__ = ["estimate_median_sigma", "_estimate_mmd2", "_estimate_mmd2_linear_time", "mmd2_matrix", "mmd2_block_terms",
           "mmd2_matrix_one_pass", "_calculate_mmd2", "install", "EPSILON"]
TILE = 64               # rows of a tile of the pairwise kernel (SQD_T of csrc/sqdist_tile.h)


def _device():
    if not torch.cuda.is_available():
        raise _lib.AvaHipError("the MMD kernels only run on an MI355X: there is no CPU fallback in this package")
    return torch.device("cuda", torch.cuda.current_device())


def _latent_dev(latent):
    """[N, z] float64 on the device (accepts the numpy array VAE.get_latent returns, or a tensor already there)."""
    dev = _device()
    t = latent if torch.is_tensor(latent) else torch.from_numpy(np.ascontiguousarray(latent, dtype=np.float64))
    t = t.to(device=dev, dtype=torch.float64).contiguous()
    if t.dim() != 2 or t.shape[1] < 1 or t.shape[1] > 128:
        raise ValueError("latent must be [N, z] with 1 <= z <= 128")
    return t


def _index_dev(idx, n_rows):
    a = np.ascontiguousarray(np.asarray(idx), dtype=np.int64)
    if a.size and (a.min() < -n_rows or a.max() >= n_rows):
        raise IndexError("index out of bounds for latent with %d rows" % n_rows)      # numpy would raise the same
    a = np.where(a < 0, a + n_rows, a)
    return torch.from_numpy(a).to(_device())


def estimate_median_sigma(latent, n=10000, seed=42):
    """Median pairwise Euclidean distance of ``n`` random pairs (mmd_plots.py:450-474): the same ``np.random`` draws
    in the same order (``randint`` twice per pair), distances on the device, median on the host."""
    L = _latent_dev(latent)
    np.random.seed(seed)
    pairs = np.random.randint(len(L), size=2 * n).reshape(n, 2)          # == n x (randint, randint), same stream
    np.random.seed(None)
    a = torch.from_numpy(np.ascontiguousarray(pairs[:, 0])).to(L.device)
    b = torch.from_numpy(np.ascontiguousarray(pairs[:, 1])).to(L.device)
    out = torch.empty(n, dtype=torch.float64, device=L.device)
    _lib.check(_lib.load().ava_pair_sqdist(L.data_ptr(), L.shape[1], a.data_ptr(), b.data_ptr(), n, out.data_ptr(),
                                           _lib.stream()), "ava_pair_sqdist")
    return np.sqrt(np.median(out.cpu().numpy()) + EPSILON)


def _terms(L, i1, i2, sigma):
    n1, n2 = len(i1), len(i2)
    if n1 * (n1 - 1) == 0 or n2 * (n2 - 1) == 0:
        raise ZeroDivisionError("division by zero")                       # the reference's 2/(n*(n-1))
    lib = _lib.load()
    d1, d2 = _index_dev(i1, len(L)), _index_dev(i2, len(L))
    nbytes = lib.ava_mmd2_workspace_bytes(n1, n2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=L.device)
    out = torch.empty(4, dtype=torch.float64, device=L.device)
    _lib.check(lib.ava_mmd2(L.data_ptr(), L.shape[1], d1.data_ptr(), n1, d2.data_ptr(), n2, float(sigma),
                            out.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "ava_mmd2")
    return out.cpu().numpy()


def _estimate_mmd2(latent, i1, i2, sigma=None, max_n=None, seed=None):
    """Unbiased quadratic-time MMD^2 estimate (Gretton et al. 2012; mmd_plots.py:255-296).  Like the reference, with
    ``max_n`` the index arrays are shuffled IN PLACE under ``np.random.seed(seed)`` and truncated."""
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    n1, n2 = len(i1), len(i2)
    if max_n is not None:
        np.random.seed(seed)
        n1, n2 = min(max_n, n1), min(max_n, n2)
        if n1 < len(i1):
            np.random.shuffle(i1)
            i1 = i1[:n1]
        if n2 < len(i2):
            np.random.shuffle(i2)
            i2 = i2[:n2]
        np.random.seed(None)
    return float(_terms(_latent_dev(latent), i1, i2, sigma)[3])


def _estimate_mmd2_linear_time(latent, i1, i2, sigma=None):
    """Linear-time estimate (mmd_plots.py:299-312)."""
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    n = min(len(i1), len(i2))
    m = n // 2
    assert m > 0
    L = _latent_dev(latent)
    lib = _lib.load()
    d1, d2 = _index_dev(i1[:2 * m], len(L)), _index_dev(i2[:2 * m], len(L))
    ws = torch.empty((min((m + 255) // 256, 1024) + 8) * 8, dtype=torch.uint8, device=L.device)
    out = torch.empty(1, dtype=torch.float64, device=L.device)
    _lib.check(lib.ava_mmd2_linear(L.data_ptr(), L.shape[1], d1.data_ptr(), d2.data_ptr(), m, float(sigma), out.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _lib.stream()), "ava_mmd2_linear")
    return float(out.item())


def mmd2_matrix(latent, condition, alg='quadratic', sigma=None, max_n=None):
    """The condition-by-condition loop of ``_calculate_mmd2`` (mmd_plots.py:395-418, serial branch): returns
    ``(result [n, n], all_conditions)`` with ``result[i, j] = result[j, i] = MMD^2(condition i, condition j)``.  The
    latent means are uploaded once for all pairs."""
    condition = np.asarray(condition)
    all_conditions = np.unique(condition)
    n = len(all_conditions)
    result = np.zeros((n, n))
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    L = _latent_dev(latent)
    for i in range(n - 1):
        for j in range(i + 1, n):
            i1 = np.argwhere(condition == all_conditions[i]).flatten()
            i2 = np.argwhere(condition == all_conditions[j]).flatten()
            if alg == 'linear':
                temp = _estimate_mmd2_linear_time(L, i1, i2, sigma=sigma)
            elif alg == 'quadratic':
                temp = _estimate_mmd2(L, i1, i2, sigma=sigma, max_n=max_n)
            else:
                raise NotImplementedError
            result[i, j] = temp
            result[j, i] = temp
    return result, all_conditions


def _group_plan(condition):
    """Everything the one-pass launches need to know about the grouping, in numpy (no GPU): a dict with

    ``all_conditions``  ``np.unique(condition)`` (sorted), ``C`` of them
    ``index``           int64 ``[N]``: the rows of condition 0, then of condition 1, ...; within a condition ascending,
                        i.e. ``np.argwhere(condition == c).flatten()`` (one stable argsort)
    ``offsets``         int64 ``[C + 1]``: condition ``c`` owns ``index[offsets[c]:offsets[c + 1]]``
    ``counts``, ``tiles``  rows and ``ceil(rows / 64)`` tiles per condition
    ``blocks``          int64 ``[C (C + 1) / 2 + 1, 4]``: a row ``{first workgroup, first workspace slot, a, b}`` per
                        block ``a <= b`` in row-major order, then the totals (the table of ``ava_mmd2_matrix``)
    ``pairs``           the same for the pairs ``a < b`` of the linear estimator (``ava_mmd2_matrix_linear``)
    """
    condition = np.asarray(condition).reshape(-1)
    order = np.argsort(condition, kind='stable').astype(np.int64)
    ordered = condition[order]
    starts = np.concatenate([[0], np.flatnonzero(ordered[1:] != ordered[:-1]) + 1]) if len(ordered) else np.zeros(0)
    starts = starts.astype(np.int64)
    offsets = np.concatenate([starts, [len(ordered)]]).astype(np.int64)
    counts = np.diff(offsets)
    tiles = (counts + TILE - 1) // TILE

    def table(a, b, workgroups, slots):
        out = np.zeros((len(a) + 1, 4), dtype=np.int64)
        out[1:, 0], out[1:, 1] = np.cumsum(workgroups), np.cumsum(slots)
        out[:-1, 2], out[:-1, 3] = a, b
        return out
    a, b = np.triu_indices(len(counts))
    full = tiles[a] * tiles[b]
    blocks = table(a, b, np.where(a == b, tiles[a] * (tiles[a] + 1) // 2, full), full)
    a, b = np.triu_indices(len(counts), 1)
    groups = np.minimum((np.minimum(counts[a], counts[b]) // 2 + 255) // 256, 1024)
    return {"all_conditions": ordered[starts], "index": order, "offsets": offsets, "counts": counts, "tiles": tiles,
            "blocks": blocks, "pairs": table(a, b, groups, groups)}


def _launch_matrix(latent, plan, sigma, linear):
    """One upload of the plan, one launch sequence, one download: ``(within [C] or None, cross / linear [C, C])``."""
    L = _latent_dev(latent)
    C = len(plan["counts"])
    if len(L) != len(plan["index"]):
        raise ValueError("latent has %d rows, condition %d" % (len(L), len(plan["index"])))
    lib = _lib.load()
    offsets = np.ascontiguousarray(plan["offsets"])
    table = plan["pairs"] if linear else plan["blocks"]
    host = np.concatenate([plan["index"], offsets, table.reshape(-1)])
    dev = torch.from_numpy(host).to(L.device)
    idx, off, tab = dev[:len(L)], dev[len(L):len(L) + C + 1], dev[len(L) + C + 1:]
    nbytes = lib.ava_mmd2_matrix_workspace_bytes(offsets.ctypes.data, C, int(linear))
    if nbytes == 0:
        raise _lib.AvaHipError("ava_mmd2_matrix_workspace_bytes: unsupported grouping (%d conditions)" % C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=L.device)
    out = (torch.zeros if linear else torch.empty)(C * C + C, dtype=torch.float64, device=L.device)
    if linear:
        _lib.check(lib.ava_mmd2_matrix_linear(L.data_ptr(), L.shape[1], idx.data_ptr(), offsets.ctypes.data,
                                              off.data_ptr(), C, tab.data_ptr(), int(table[-1, 0]), float(sigma),
                                              out.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()),
                   "ava_mmd2_matrix_linear")
    else:
        _lib.check(lib.ava_mmd2_matrix(L.data_ptr(), L.shape[1], idx.data_ptr(), offsets.ctypes.data, off.data_ptr(), C,
                                       tab.data_ptr(), int(table[-1, 0]), float(sigma), out[C * C:].data_ptr(),
                                       out.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "ava_mmd2_matrix")
    host_out = out.cpu().numpy()
    return (None if linear else host_out[C * C:]), host_out[:C * C].reshape(C, C)


def mmd2_block_terms(latent, condition, sigma=None):
    """The normalised block sums behind the whole MMD^2 matrix, from one launch sequence: ``(within [C], cross [C, C],
    all_conditions)`` with ``within[a]`` the within-set term of condition ``a`` (``term_1`` / ``term_2`` of
    mmd_plots.py:276-288) and ``cross[a, b] = cross[b, a]`` the cross term of the pair (``term_3``, :289-294);
    ``cross[a, a] = 0``.  Bit for bit the terms :func:`_terms` gives pair by pair.  Needs two conditions or more, each
    of two rows or more (``ZeroDivisionError`` otherwise, as the reference's ``2/(n*(n-1))``)."""
    plan = _group_plan(condition)
    if len(plan["counts"]) < 2:
        raise ValueError("mmd2_block_terms needs at least two conditions")
    if plan["counts"].min() < 2:
        raise ZeroDivisionError("division by zero")
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    within, cross = _launch_matrix(latent, plan, sigma, False)
    return within, cross, plan["all_conditions"]


def mmd2_matrix_one_pass(latent, condition, alg='quadratic', sigma=None, max_n=None):
    """:func:`mmd2_matrix` without the host loop: ``(result [C, C], all_conditions)``, the same values bit for bit.

    The rows are grouped by condition once and every pair's sums come out of one launch sequence (``alg='quadratic'``:
    ``result[i, j] = within[i] + within[j] - cross[i, j]`` of :func:`mmd2_block_terms`, each within-set term computed
    once; ``alg='linear'``: every pair's linear-time estimate).  No conditions give a ``(0, 0)`` result, one gives
    ``[[0.]]``; otherwise an unknown ``alg`` raises ``NotImplementedError`` and a condition of fewer than two rows
    ``ZeroDivisionError`` (quadratic) or ``AssertionError`` (linear), like the reference's loop, before any launch.

    ``max_n``: the reference draws a fresh, unseeded subsample of the larger conditions for every pair, which one pass
    over fixed index lists cannot restate.  So when ``alg='quadratic'``, ``max_n`` is not ``None`` and some condition
    has more than ``max_n`` rows, this calls the per-pair :func:`mmd2_matrix`; otherwise ``max_n`` has no effect (the
    linear estimator never looks at it) and the one-pass path runs."""
    plan = _group_plan(condition)
    all_conditions, counts = plan["all_conditions"], plan["counts"]
    n = len(counts)
    result = np.zeros((n, n))
    if n < 2:
        return result, all_conditions
    if alg not in ('linear', 'quadratic'):
        raise NotImplementedError
    if alg == 'linear':
        assert counts.min() // 2 > 0
    elif counts.min() < 2:
        raise ZeroDivisionError("division by zero")
    elif max_n is not None and counts.max() > max_n:
        return mmd2_matrix(latent, condition, alg=alg, sigma=sigma, max_n=max_n)
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    within, cross = _launch_matrix(latent, plan, sigma, alg == 'linear')
    i, j = np.triu_indices(n, 1)
    upper = cross[i, j] if alg == 'linear' else within[i] + within[j] - cross[i, j]
    result[i, j] = upper
    result[j, i] = upper
    return result, all_conditions


def _calculate_mmd2(dc, condition_from_fn, mmd2_fn=None, condition_fn=None, parallel=False, alg='quadratic', max_n=None,
                    sigma=None, verbose=True):
    """``_calculate_mmd2`` of the reference (mmd_plots.py:337-434) on :func:`mmd2_matrix_one_pass`: same arguments,
    asserts, messages, saved files and return value ``(mmd2 [C, C], conditions [C])``.  ``dc`` needs a
    ``request(field)`` method for ``'latent_means'`` and ``'audio_filenames'`` (a ``DataContainer``).

    ``parallel=True`` starts no joblib workers (each would open the GPU for a share of one launch sequence); the
    ``i j mmd2`` lines the reference's workers print are printed once the matrix is there, in ``(i, j)`` order, so
    ``_matrix_from_txt`` on the captured output still rebuilds the matrix."""
    assert alg in ['linear', 'quadratic']
    assert mmd2_fn is not None
    if verbose:
        print("Estimating an MMD matrix...")
        print("\talg:", alg)
        print("\tparallel:", parallel)
        print("\tmax_n:", max_n)
    latent = dc.request('latent_means')
    audio_fns = dc.request('audio_filenames')
    condition = np.array([condition_from_fn(str(i)) for i in audio_fns], dtype='int')
    n = len(np.unique(condition))
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    if verbose:
        print("\tconditions found:", n)
        print("\tsigma:", sigma)
    result, all_conditions = mmd2_matrix_one_pass(latent, condition, alg=alg, sigma=sigma, max_n=max_n)
    if parallel:
        for i in range(n - 1):
            for j in range(i + 1, n):
                print(i, j, float(result[i, j]), flush=True)
    if mmd2_fn is not None:
        if verbose:
            print("\tSaving MMD^2 to:", mmd2_fn)
        np.save(mmd2_fn, result)
    if condition_fn is not None:
        if verbose:
            print("\tSaving conditions to:", condition_fn)
        np.save(condition_fn, all_conditions)
    if verbose:
        print("\tDone.")
    return result, all_conditions


def install(module=None, matrix=False):
    """Point ``ava.plotting.mmd_plots``'s estimators at this module (call after importing the reference package).
    ``matrix=True`` also replaces its ``_calculate_mmd2``, the function behind ``mmd_matrix_plot_DC``, with the
    one-pass :func:`_calculate_mmd2` of this module."""
    if module is None:
        import ava.plotting.mmd_plots as module
    module.estimate_median_sigma = estimate_median_sigma
    module._estimate_mmd2 = _estimate_mmd2
    module._estimate_mmd2_linear_time = _estimate_mmd2_linear_time
    if matrix:
        module._calculate_mmd2 = _calculate_mmd2
    return module
