"""MMD^2 between conditions on the MI355X.

Host-side mirror of the estimator functions of the reference's ``ava/plotting/mmd_plots.py`` -- same names, same
arguments, same random-number use and error behaviour -- with the O(n^2) Python double loops replaced by the HIP
kernels of ``csrc/mmd.hip`` (fp64, like the reference's numpy arithmetic):

=============================  ==========================================  =============================
reference (mmd_plots.py)       here                                        C entry point
=============================  ==========================================  =============================
``estimate_median_sigma``      :func:`estimate_median_sigma`  (:450-474)   ``ava_pair_sqdist``
``_estimate_mmd2``             :func:`_estimate_mmd2`         (:255-296)   ``ava_mmd2_matrix``, two conditions
``_estimate_mmd2_linear_time`` :func:`_estimate_mmd2_linear_time` (:299-312) ``ava_mmd2_matrix_linear``, two conditions
loop of ``_calculate_mmd2``    :func:`mmd2_matrix`            (:395-418)   ``ava_mmd2_matrix`` / ``_linear`` per pair
the same loop, in one pass     :func:`mmd2_matrix_one_pass`                ``ava_mmd2_matrix`` / ``_linear``, all at once
``_calculate_mmd2``            :func:`_calculate_mmd2`        (:337-434)   the one-pass matrix
(none: Gretton et al. 2012)    :func:`mmd2_permutation_test`, ``_matrix``  ``ava_mmd2_perm`` (row f18)
=============================  ==========================================  =============================

``install()`` swaps the three estimator functions of an imported ``ava.plotting.mmd_plots`` for these, so the
reference's plotting functions (``mmd_matrix_plot_DC`` ...) run unchanged on top of them; ``install(matrix=True)`` also
swaps ``_calculate_mmd2``, so that the whole condition-by-condition matrix is one launch sequence (every block sum of
the sorted index list at once, each within-set term once) instead of a host loop over the pairs.

:func:`mmd2_permutation_test` and :func:`mmd2_permutation_matrix` add what the reference lacks, a measure of significance
for the quadratic estimate: the one-sided permutation p-value of Gretton et al. 2012 (section 5), the null distribution
computed on the device by ``csrc/mmd_perm.hip`` (model: DESIGN.md section 1, row f18).  There is no CPU fallback:
without the HIP library / a GPU every function raises ``AvaHipError``.
"""
import numpy as np
import torch

from . import _lib, _rows

EPSILON = 1e-8          # ava/plotting/mmd_plots.py:34

__all__ = ["estimate_median_sigma", "_estimate_mmd2", "_estimate_mmd2_linear_time", "mmd2_matrix", "mmd2_block_terms",
           "mmd2_matrix_one_pass", "_calculate_mmd2", "mmd2_permutation_test", "mmd2_permutation_matrix",
           "_calculate_mmd2_pvalues", "install", "EPSILON", "PERM_TILE", "PERM_MAX_BYTES"]
TILE = 64               # rows of a tile of the pairwise kernel (SQD_T of csrc/sqdist_tile.h)
PERM_TILE = 64          # columns (splits) of a workgroup of the statistic kernel (MP_COLS of csrc/mmd_perm.hip)
PERM_MAX_BYTES = 256 << 20          # default bound on the membership bytes plus workspace of one chunk of splits
PERM_MAX_CHUNK = 1 << 20            # splits per call of ava_mmd2_perm


def _device():
    return _lib.device("MMD")


def _latent_dev(latent):
    """[N, z] float64 on the device (accepts the numpy array VAE.get_latent returns, or a tensor already there)."""
    t = _rows.upload(latent, _device(), torch.float64)
    if t.dim() != 2 or t.shape[1] < 1 or t.shape[1] > 128:
        raise ValueError("latent must be [N, z] with 1 <= z <= 128")
    return t


def _pair_index(i1, i2, n_rows):
    """the index list ``i1`` followed by ``i2``, int64 on the host, as rows 0 .. n_rows - 1 (negative ones wrapped)"""
    a = np.concatenate([np.asarray(i1, dtype=np.int64), np.asarray(i2, dtype=np.int64)])
    if a.size and (a.min() < -n_rows or a.max() >= n_rows):
        raise IndexError("index out of bounds for latent with %d rows" % n_rows)      # numpy would raise the same
    return np.where(a < 0, a + n_rows, a)


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
    """float64 ``[term_1, term_2, term_3, term_1 + term_2 - term_3]`` of mmd_plots.py:276-295 for two index lists (in any
    order, rows may repeat or be in both): the one-pass matrix of two conditions, the last entry formed on the host"""
    n1, n2 = len(i1), len(i2)
    if n1 * (n1 - 1) == 0 or n2 * (n2 - 1) == 0:
        raise ZeroDivisionError("division by zero")                       # the reference's 2/(n*(n-1))
    within, cross = _launch_pair(L, i1, i2, sigma, False)
    return np.array([within[0], within[1], cross[0, 1], within[0] + within[1] - cross[0, 1]])


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
    return float(_launch_pair(_latent_dev(latent), i1[:2 * m], i2[:2 * m], sigma, True)[1][0, 1])


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


def _count_plan(counts):
    """What the launches need to know about conditions of ``counts`` rows each, in numpy (no GPU): a dict with

    ``counts``, ``tiles``  int64 ``[C]``: rows and ``ceil(rows / 64)`` tiles per condition
    ``offsets``         int64 ``[C + 1]``: condition ``c`` owns ``index[offsets[c]:offsets[c + 1]]`` of the index list
    ``blocks``          int64 ``[C (C + 1) / 2 + 1, 4]``: a row ``{first workgroup, first workspace slot, a, b}`` per
                        block ``a <= b`` in row-major order, then the totals (the table of ``ava_mmd2_matrix``)
    ``pairs``           the same for the pairs ``a < b`` of the linear estimator (``ava_mmd2_matrix_linear``)
    """
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    tiles = (counts + TILE - 1) // TILE

    def table(a, b, workgroups, slots):
        out = np.zeros((len(a) + 1, 4), dtype=np.int64)
        np.cumsum(workgroups, out=out[1:, 0])
        np.cumsum(slots, out=out[1:, 1])
        out[:-1, 2], out[:-1, 3] = a, b
        return out
    r = np.arange(len(counts))
    a, b = np.nonzero(r[:, None] <= r)                     # row-major; a two-condition call builds this per estimate
    full = tiles[a] * tiles[b]
    blocks = table(a, b, np.where(a == b, tiles[a] * (tiles[a] + 1) // 2, full), full)
    a, b = a[a < b], b[a < b]
    groups = np.minimum((np.minimum(counts[a], counts[b]) // 2 + 255) // 256, 1024)
    return {"offsets": offsets, "counts": counts, "tiles": tiles, "blocks": blocks, "pairs": table(a, b, groups, groups)}


def _group_plan(condition):
    """The grouping of a condition array: :func:`_count_plan` of the rows per condition, and

    ``all_conditions``  ``np.unique(condition)`` (sorted), ``C`` of them
    ``index``           int64 ``[N]``: the rows of condition 0, then of condition 1, ...; within a condition ascending,
                        i.e. ``np.argwhere(condition == c).flatten()`` (one stable argsort)
    """
    condition = np.asarray(condition).reshape(-1)
    order = np.argsort(condition, kind='stable').astype(np.int64)
    ordered = condition[order]
    starts = np.concatenate([[0], np.flatnonzero(ordered[1:] != ordered[:-1]) + 1]) if len(ordered) else np.zeros(0)
    starts = starts.astype(np.int64)
    plan = _count_plan(np.diff(np.concatenate([starts, [len(ordered)]])))
    plan.update(all_conditions=ordered[starts], index=order)
    return plan


def _condition_latent(latent, plan):
    """the device latent of a condition array's callers: one row per entry of the array"""
    L = _latent_dev(latent)
    if len(L) != len(plan["index"]):
        raise ValueError("latent has %d rows, condition %d" % (len(L), len(plan["index"])))
    return L


def _launch_matrix(L, index, plan, sigma, linear):
    """One upload (``index``, the offsets and the table of ``plan`` in one tensor), one launch sequence, one download:
    ``(within [C] or None, cross / linear [C, C])``.  ``index``: int64 rows of the device latent ``L``, the lists of the
    plan's conditions one after the other."""
    C, n = len(plan["counts"]), len(index)
    lib = _lib.load()
    offsets = np.ascontiguousarray(plan["offsets"])
    table = plan["pairs"] if linear else plan["blocks"]
    host = np.concatenate([index, offsets, table.reshape(-1)])
    dev = torch.from_numpy(host).to(L.device)
    idx, off, tab = dev[:n], dev[n:n + C + 1], dev[n + C + 1:]
    nbytes = lib.ava_mmd2_matrix_workspace_bytes(offsets.ctypes.data, C, int(linear))
    if nbytes == 0:
        raise _lib.AvaHipError("ava_mmd2_matrix_workspace_bytes: unsupported grouping (%d conditions)" % C)
    ws = _lib.workspace(nbytes, L.device, "MMD matrix")
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


def _launch_pair(L, i1, i2, sigma, linear):
    """:func:`_launch_matrix` of two conditions, the rows ``i1`` and the rows ``i2`` of the device latent ``L``"""
    return _launch_matrix(L, _pair_index(i1, i2, len(L)), _count_plan([len(i1), len(i2)]), sigma, linear)


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
    within, cross = _launch_matrix(_condition_latent(latent, plan), plan["index"], plan, sigma, False)
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
    within, cross = _launch_matrix(_condition_latent(latent, plan), plan["index"], plan, sigma, alg == 'linear')
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


def _perm_table(o1, o2, n1, n2, pair):
    """The problem table of ``ava_mmd2_perm``: int64 ``[problems + 1, 8]`` rows ``{o1, o2, n1, n2, pair, first position,
    first row tile, 0}`` and the sentinel ``{0, 0, 0, 0, 0, all positions, all row tiles, 0}``."""
    n1, n2 = np.asarray(n1, dtype=np.int64).reshape(-1), np.asarray(n2, dtype=np.int64).reshape(-1)
    table = np.zeros((len(n1) + 1, 8), dtype=np.int64)
    table[:-1, 0], table[:-1, 1], table[:-1, 2], table[:-1, 3], table[:-1, 4] = o1, o2, n1, n2, pair
    table[1:, 5] = np.cumsum(n1 + n2)
    table[1:, 6] = np.cumsum((n1 + n2 + TILE - 1) // TILE)
    return table


def _perm_bytes(table, k):
    """Device bytes of a chunk of ``k`` splits: ``k`` membership bytes per pool position plus the workspace of
    ``ava_mmd2_perm_workspace_bytes`` (``k + 1`` columns of two doubles per row tile, and 256)."""
    return int(k * table[-1, 5] + table[-1, 6] * (k + 1) * 16 + 256)


def _perm_chunk(table, n_splits, max_bytes):
    """The most splits (at least 1, at most ``n_splits``) whose chunk stays within ``max_bytes``."""
    if max_bytes is None:
        max_bytes = PERM_MAX_BYTES
    per = int(table[-1, 5] + 16 * table[-1, 6])
    k = (int(max_bytes) - _perm_bytes(table, 0)) // per
    return int(max(1, min(k, n_splits, PERM_MAX_CHUNK, (2 ** 31 - 1) // max(len(table) - 1, 1))))


def _perm_check(n_perm, counts):
    if n_perm < 1:
        raise ValueError("n_perm must be at least 1")
    if n_perm > 2 ** 31 - 2:
        raise ValueError("n_perm must be below 2^31 - 1")
    if len(counts) and min(counts) < 2:
        raise ZeroDivisionError("division by zero")                       # the reference's 2/(n*(n-1))


def _run_perm(L, idx, table, n_perm, seed, sigma, max_bytes, want_null):
    """Splits 0 .. n_perm of every problem of ``table`` in chunks: ``(stat_0 [problems], counts [problems], null
    [problems, n_perm + 1, 4] or None)``, ``null[:, p]`` the three terms and the statistic of split ``p``.  ``idx``: the
    device index list the table's offsets point into."""
    lib = _lib.load()
    n_prob = len(table) - 1
    table = np.ascontiguousarray(table)
    tab_dev = torch.from_numpy(table).to(L.device)
    k = _perm_chunk(table, n_perm + 1, max_bytes)
    nbytes = lib.ava_mmd2_perm_workspace_bytes(table.ctypes.data, n_prob, k)
    if nbytes == 0:
        raise _lib.AvaHipError("ava_mmd2_perm_workspace_bytes: unsupported problem table (%d problems)" % n_prob)
    ws = _lib.workspace(nbytes, L.device, "MMD permutations")
    mem = torch.empty(k * int(table[-1, 5]), dtype=torch.uint8, device=L.device)
    terms = torch.empty(n_prob * k * 3, dtype=torch.float64, device=L.device)
    stats = torch.empty(n_prob * k, dtype=torch.float64, device=L.device)
    stat0 = torch.empty(n_prob, dtype=torch.float64, device=L.device)
    counts = torch.empty(n_prob, dtype=torch.int64, device=L.device)
    null = np.empty((n_prob, n_perm + 1, 4)) if want_null else None
    for p0 in range(0, n_perm + 1, k):
        p1 = min(p0 + k, n_perm + 1)
        _lib.check(lib.ava_mmd2_perm(L.data_ptr(), L.shape[1], idx.data_ptr(), idx.numel(), table.ctypes.data,
                                     tab_dev.data_ptr(), n_prob, p0, p1, int(seed) & 0xffffffff, float(sigma),
                                     mem.data_ptr(), terms.data_ptr(), stats.data_ptr(), stat0.data_ptr(),
                                     counts.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "ava_mmd2_perm")
        if want_null:
            null[:, p0:p1, :3] = terms[:n_prob * (p1 - p0) * 3].cpu().numpy().reshape(n_prob, p1 - p0, 3)
            null[:, p0:p1, 3] = stats[:n_prob * (p1 - p0)].cpu().numpy().reshape(n_prob, p1 - p0)
    return stat0.cpu().numpy(), counts.cpu().numpy(), null


def _perm_terms(latent, i1, i2, n_perm, seed, sigma, max_bytes=None, pair=0):
    """One problem: ``(terms [n_perm + 1, 4], count)``: the reference's three terms and their combination for splits
    0 .. n_perm, and ``#{p >= 1 : stat_p >= stat_0}`` as the device counted it."""
    n1, n2 = len(i1), len(i2)
    L = _latent_dev(latent)
    idx = torch.from_numpy(_pair_index(i1, i2, len(L))).to(L.device)
    _, counts, null = _run_perm(L, idx, _perm_table(0, n1, n1, n2, pair), n_perm, seed, sigma, max_bytes, True)
    return null[0], int(counts[0])


def mmd2_permutation_test(latent, i1, i2, n_perm=1000, seed=0, sigma=None, return_null=False, max_bytes=None):
    """Permutation test for the quadratic MMD^2 estimate (Gretton et al. 2012, section 5):
    ``(mmd2, pvalue)``, or ``(mmd2, pvalue, null [n_perm])`` with ``return_null=True``.

    The two sets are pooled and re-split ``n_perm`` times into ``len(i1)`` and ``len(i2)`` rows (the splits are a
    function of ``seed`` alone); ``null`` holds the statistic of every re-split, ``mmd2`` that of the caller's own split
    (from the same kernel; it agrees with :func:`_estimate_mmd2` to rounding) and ``pvalue = (1 + #{null >= mmd2}) /
    (n_perm + 1)``: one-sided, never 0.  The splits go to the device in chunks whose membership bytes plus workspace
    stay within ``max_bytes`` (default ``PERM_MAX_BYTES``, 256 MiB; never fewer than one split); no result depends on
    it.  ``sigma=None`` is ``estimate_median_sigma(latent)``.  A set of fewer than two rows raises
    ``ZeroDivisionError`` like :func:`_estimate_mmd2`, ``n_perm < 1`` ``ValueError``; both before the device is
    touched."""
    n1, n2 = len(i1), len(i2)
    _perm_check(n_perm, [n1, n2])
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    L = _latent_dev(latent)
    idx = torch.from_numpy(_pair_index(i1, i2, len(L))).to(L.device)
    stat0, counts, null = _run_perm(L, idx, _perm_table(0, n1, n1, n2, 0), n_perm, seed, sigma, max_bytes, return_null)
    out = (float(stat0[0]), (1 + int(counts[0])) / (n_perm + 1))
    return out + (null[0, 1:, 3].copy(),) if return_null else out


def mmd2_permutation_matrix(latent, condition, n_perm=1000, seed=0, sigma=None, max_bytes=None):
    """:func:`mmd2_permutation_test` for every pair of conditions in one launch sequence per chunk of splits:
    ``(mmd2 [C, C], pvalue [C, C], all_conditions)``, both symmetric, ``mmd2`` with a zero diagonal and ``pvalue`` with a
    diagonal of ones.  Entry ``(i, j)``, ``i < j``, is bit for bit what ``mmd2_permutation_test(latent, rows of
    condition i, rows of condition j, n_perm, seed + pair)`` gives, ``pair`` the index of ``(i, j)`` among the pairs in
    row-major order.  The p-values are not corrected for the C (C - 1) / 2 comparisons."""
    plan = _group_plan(condition)
    all_conditions, counts = plan["all_conditions"], plan["counts"]
    C = len(counts)
    _perm_check(n_perm, counts if C > 1 else [])
    mmd2, pvalue = np.zeros((C, C)), np.ones((C, C))
    if C < 2:
        return mmd2, pvalue, all_conditions
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    L = _condition_latent(latent, plan)
    a, b = np.triu_indices(C, 1)
    table = _perm_table(plan["offsets"][a], plan["offsets"][b], counts[a], counts[b], np.arange(len(a)))
    idx = torch.from_numpy(plan["index"]).to(L.device)
    stat0, cnt, _ = _run_perm(L, idx, table, n_perm, seed, sigma, max_bytes, False)
    mmd2[a, b] = mmd2[b, a] = stat0
    pvalue[a, b] = pvalue[b, a] = (1 + cnt) / (n_perm + 1)
    return mmd2, pvalue, all_conditions


def _calculate_mmd2_pvalues(dc, condition_from_fn, pvalue_fn=None, condition_fn=None, n_perm=1000, seed=0, sigma=None,
                            verbose=True):
    """The companion of :func:`_calculate_mmd2` for :func:`mmd2_permutation_matrix`: the same two ``dc.request`` calls,
    messages in the same style, ``np.save`` of the p-values (``pvalue_fn``, required) and of the conditions
    (``condition_fn``); returns ``(mmd2 [C, C], pvalue [C, C], conditions [C])``."""
    assert pvalue_fn is not None
    if verbose:
        print("Estimating an MMD p-value matrix...")
        print("\tn_perm:", n_perm)
        print("\tseed:", seed)
    latent = dc.request('latent_means')
    audio_fns = dc.request('audio_filenames')
    condition = np.array([condition_from_fn(str(i)) for i in audio_fns], dtype='int')
    n = len(np.unique(condition))
    if sigma is None:
        sigma = estimate_median_sigma(latent)
    if verbose:
        print("\tconditions found:", n)
        print("\tsigma:", sigma)
    mmd2, pvalue, all_conditions = mmd2_permutation_matrix(latent, condition, n_perm=n_perm, seed=seed, sigma=sigma)
    if verbose:
        print("\tSaving p-values to:", pvalue_fn)
    np.save(pvalue_fn, pvalue)
    if condition_fn is not None:
        if verbose:
            print("\tSaving conditions to:", condition_fn)
        np.save(condition_fn, all_conditions)
    if verbose:
        print("\tDone.")
    return mmd2, pvalue, all_conditions


def install(module=None, matrix=False, pvalues=False, tsne=False):
    """Point ``ava.plotting.mmd_plots``'s estimators at this module (call after importing the reference package).
    ``matrix=True`` also replaces its ``_calculate_mmd2``, the function behind ``mmd_matrix_plot_DC``, with the
    one-pass :func:`_calculate_mmd2` of this module; ``pvalues=True`` adds :func:`_calculate_mmd2_pvalues` (a name the
    reference does not have) beside it; ``tsne=True`` replaces its ``TSNE`` (sklearn's, whose exact fit of a
    precomputed matrix raises with scikit-learn 1.7) with :class:`ava_amd.tsne.TSNE`, so that ``mmd_tsne_plot_DC``
    runs unchanged (row f19)."""
    if module is None:
        import ava.plotting.mmd_plots as module
    module.estimate_median_sigma = estimate_median_sigma
    module._estimate_mmd2 = _estimate_mmd2
    module._estimate_mmd2_linear_time = _estimate_mmd2_linear_time
    if matrix:
        module._calculate_mmd2 = _calculate_mmd2
    if pvalues:
        module._calculate_mmd2_pvalues = _calculate_mmd2_pvalues
    if tsne:
        from .tsne import TSNE
        module.TSNE = TSNE
    return module
