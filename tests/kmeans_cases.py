"""The numpy restatement of the k-means model of ``ava_amd/kmeans.py`` / ``csrc/kmeans.hip`` and the deterministic cases of
its tests and of ``tests/golden/make_golden_kmeans.py``.

The restatement follows scikit-learn 1.7's ``_kmeans_plusplus``, ``_kmeans_single_lloyd``, ``_tolerance``,
``_relocate_empty_clusters_dense`` and the ``n_init`` loop of ``KMeans.fit`` with the orders the model states: direct fp64
squared differences with the features ascending, ``RandomState`` draws call for call, sums over 2048-row chunks (rows
ascending inside a chunk, chunks ascending), no centring of the rows.  numpy has no fused multiply-add, so a distance
differs from the device's by the rounding of its products: a relative 2^-53 per feature.

Each function takes an optional ``trace`` dict and records in it how far the run stayed from the model's discontinuous
rules (relative margins): ``'assign'`` the least gap between the best and second-best centre of any row at any iteration,
``'search'`` the least gap of a ``searchsorted`` threshold to its neighbouring scan entries, ``'potential'`` the least gap
between the two best candidate potentials, ``'shift'`` the least gap of ``shift`` to the tolerance.
"""
import numpy as np

CHUNK = 2048
_TINY = np.finfo(np.float64).tiny


def _note(trace, key, value):
    if trace is not None:
        trace[key] = min(trace.get(key, np.inf), float(value))


def sqd(X, C):
    """[len(X), len(C)] squared distances: direct differences, features ascending"""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    acc = np.zeros((X.shape[0], C.shape[0]), dtype=np.float64)
    for j in range(X.shape[1]):
        df = X[:, j:j + 1] - C[None, :, j]
        acc += df * df
    return acc


def chunk_sum(v):
    """the sum over axis 0: rows ascending inside 2048-row chunks, the chunk partials added ascending"""
    v = np.asarray(v, dtype=np.float64)
    total = np.zeros(v.shape[1:], dtype=np.float64)
    for c0 in range(0, len(v), CHUNK):
        total = total + np.cumsum(v[c0:c0 + CHUNK], axis=0)[-1]
    return total


def chunk_scan(v):
    """the inclusive scan of a vector: sequential inside the chunks, the ascending chunk offsets added"""
    v = np.asarray(v, dtype=np.float64)
    out = np.empty_like(v)
    off = 0.0
    for c0 in range(0, len(v), CHUNK):
        local = np.cumsum(v[c0:c0 + CHUNK])
        out[c0:c0 + CHUNK] = off + local
        off = off + local[-1]
    return out


def cluster_sums(X, labels, k):
    """(sums [k, d], counts [k]) in the chunk order; a label outside [0, k) is in no cluster"""
    X = np.asarray(X, dtype=np.float64)
    sums = np.zeros((k, X.shape[1]), dtype=np.float64)
    counts = np.zeros(k, dtype=np.int64)
    for c0 in range(0, len(X), CHUNK):
        lab = labels[c0:c0 + CHUNK]
        for j in np.unique(lab):
            if 0 <= j < k:
                rows = np.flatnonzero(lab == j)
                sums[j] = sums[j] + np.cumsum(X[c0:c0 + CHUNK][rows], axis=0)[-1]
                counts[j] += len(rows)
    return sums, counts


def mean_variance(X):
    """np.mean(np.var(X, axis=0)) in the chunk order"""
    X = np.asarray(X, dtype=np.float64)
    mean = chunk_sum(X) / len(X)
    var = chunk_sum((X - mean) ** 2) / len(X)
    return float(np.cumsum(var)[-1] / X.shape[1])


def n_trials(k):
    return 2 + int(np.log(k))


def plusplus_steps(X, k, first, rand, trace=None):
    """the rows k-means++ chooses from the first row and the uniform draws ``rand`` [k - 1, L]"""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    idx = [int(first)]
    closest = sqd(X, X[first:first + 1])[:, 0]
    for c in range(1, k):
        scan = chunk_scan(closest)
        pot = scan[-1]
        v = rand[c - 1] * pot
        cand = np.minimum(np.searchsorted(scan, v), n - 1)
        if trace is not None and pot > 0:
            for vi, ci in zip(v, cand):
                gaps = [abs(scan[ci] - vi)] + ([abs(vi - scan[ci - 1])] if ci > 0 else [])
                _note(trace, 'search', min(gaps) / pot)
        dc = np.minimum(closest[None, :], sqd(X[cand], X))
        pots = np.array([chunk_sum(row) for row in dc])
        b = int(np.argmin(pots))
        others = pots[cand != cand[b]]
        if len(others) and pot > 0:
            _note(trace, 'potential', (others.min() - pots[b]) / pot)
        closest = dc[b]
        idx.append(int(cand[b]))
    return np.asarray(idx, dtype=np.int64)


def plusplus(X, k, rs, trace=None):
    """sklearn's ``_kmeans_plusplus``: the chosen rows; the draws are taken from ``rs`` call for call"""
    n = len(X)
    first = int(rs.choice(n, p=np.full(n, 1.0 / n)))
    L = n_trials(k)
    # the draws do not depend on the data, so taking them first leaves the sequence as sklearn's
    rand = np.array([rs.uniform(size=L) for _ in range(k - 1)]).reshape(k - 1, L)
    return plusplus_steps(X, k, first, rand, trace)


def relocate(X, sums, counts, labels, d2):
    """sklearn's ``_relocate_empty_clusters_dense`` on the sums, in place: the empty clusters in ascending id take the
    rows in the order (d2 descending, row ascending)"""
    empty = np.flatnonzero(counts == 0)
    if len(empty) == 0:
        return
    order = np.lexsort((np.arange(len(d2)), -d2))
    for e, f in zip(empty, order[:len(empty)]):
        old = labels[f]
        sums[old] = sums[old] - X[f]
        sums[e] = X[f]
        counts[e] = 1
        counts[old] -= 1


def assign(X, C, trace=None):
    D = sqd(X, C)
    labels = np.argmin(D, axis=1)
    d2 = D[np.arange(len(D)), labels]
    if trace is not None and D.shape[1] > 1:
        two = np.partition(D, 1, axis=1)[:, :2]
        _note(trace, 'assign', ((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], _TINY)).min())
    return labels, d2


def update(X, labels, d2, C):
    """(new centres, shift) of one iteration from its labels"""
    k = len(C)
    sums, counts = cluster_sums(X, labels, k)
    relocate(np.asarray(X, dtype=np.float64), sums, counts, labels, d2)
    new = sums.copy()
    full = counts > 0
    new[full] = sums[full] / counts[full, None]
    shift = float(np.cumsum(np.cumsum((new - C) ** 2, axis=1)[:, -1])[-1])
    return new, shift


def lloyd(X, centres, tol_abs, max_iter, trace=None):
    """sklearn's ``_kmeans_single_lloyd``: (labels int32, inertia, centres, n_iter)"""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(centres, dtype=np.float64)
    old = np.full(len(X), -1, dtype=np.int64)
    for i in range(max_iter):
        labels, d2 = assign(X, C, trace)
        C, shift = update(X, labels, d2, C)
        if np.array_equal(labels, old):
            break
        if tol_abs > 0:
            _note(trace, 'shift', abs(shift - tol_abs) / tol_abs)
        if shift <= tol_abs:
            break
        old = labels
    labels, d2 = assign(X, C, trace)
    return labels.astype(np.int32), float(chunk_sum(d2)), C, i + 1


def same_clustering(a, b, k):
    return len(np.unique(a.astype(np.int64) * k + b)) == len(np.unique(a))


def fit(X, k, *, init='k-means++', n_init='auto', max_iter=300, tol=1e-4, random_state=None, trace=None):
    """sklearn's ``KMeans.fit``: a dict of labels, centres, inertia, n_iter"""
    X = np.asarray(X, dtype=np.float64)
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    kind = init if isinstance(init, str) else 'array'
    if n_init == 'auto':
        n_init = 10 if kind == 'random' else 1
    if kind == 'array':
        n_init = 1
    tol_abs = mean_variance(X) * tol
    best = None
    for _ in range(n_init):
        if kind == 'k-means++':
            start = X[plusplus(X, k, rs, trace)]
        elif kind == 'random':
            start = X[rs.choice(len(X), size=k, replace=False, p=np.full(len(X), 1.0 / len(X)))]
        else:
            start = np.asarray(init, dtype=np.float64)
        labels, inertia, C, n_iter = lloyd(X, start, tol_abs, max_iter, trace)
        if best is None or (inertia < best['inertia'] and not same_clustering(labels, best['labels'], k)):
            best = dict(labels=labels, inertia=inertia, centres=C, n_iter=n_iter)
    return best


# ---- the cases ---------------------------------------------------------------------------------------------------------
def blobs(n, d, k, sep, seed):
    """n rows around k centres that are ``sep`` standard deviations apart per feature, float64 [n, d]"""
    rng = np.random.RandomState(seed)
    centres = sep * rng.standard_normal((k, d))
    return centres[rng.randint(0, k, size=n)] + rng.standard_normal((n, d))


def far_init(X, k):
    """the first k - 1 rows and one centre far from every row: that cluster is empty in the first iteration"""
    init = np.array(X[:k], dtype=np.float64)
    init[k - 1] = X.max(axis=0) + 100.0
    return init


# name -> (n, d, blobs' k, sep, data seed, KMeans arguments); init 'far' is far_init(X, n_clusters)
FIT_CASES = {
    "n300_d5_k4_sep6":      (300, 5, 4, 6.0, 1, dict(n_clusters=4, random_state=0)),
    "n300_d5_k4_sep1":      (300, 5, 4, 1.0, 2, dict(n_clusters=4, random_state=42)),
    "n1000_d16_k2":         (1000, 16, 2, 2.0, 3, dict(n_clusters=2, random_state=0)),
    "n2049_d33_k8":         (2049, 33, 8, 1.5, 4, dict(n_clusters=8, random_state=42)),
    "n4100_d128_k64":       (4100, 128, 64, 0.5, 5, dict(n_clusters=64, random_state=0)),
    "n2049_d8_k256":        (2049, 8, 256, 3.0, 6, dict(n_clusters=256, random_state=42)),
    "random_n_init3":       (500, 10, 5, 2.0, 7, dict(n_clusters=5, init='random', n_init=3, random_state=0)),
    "max_iter1":            (300, 5, 4, 1.0, 2, dict(n_clusters=4, random_state=42, max_iter=1)),
    "tol0":                 (600, 6, 5, 1.0, 8, dict(n_clusters=5, random_state=0, tol=0.0)),
    "one_empty":            (400, 3, 4, 2.0, 9, dict(n_clusters=4, init='far')),
}


def fit_case(name):
    """(rows float64 [n, d], the KMeans arguments with ``init`` resolved)"""
    n, d, k, sep, seed, kw = FIT_CASES[name]
    X = blobs(n, d, k, sep, seed)
    kw = dict(kw)
    if kw.get('init') == 'far':
        kw['init'] = far_init(X, kw['n_clusters'])
    return X, kw


def empty_three_case():
    """three empty clusters at once and ties in the farthest distance: rows on a lattice (so the distances to a centre at
    the origin repeat exactly) and three centres far away.  (rows [n, 2], init [5, 2])"""
    g = np.arange(-4.0, 5.0)
    X = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2)
    X = np.concatenate([X, X + np.array([40.0, 0.0])])
    init = np.array([[0.0, 0.0], [40.0, 0.0], [500.0, 500.0], [600.0, 600.0], [700.0, 700.0]])
    return X, init


# ---- the edge cases (test_gpu_kmeans_edges.py; test_cpu_kmeans.py proves that each decides what it claims) -------------
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
# (n, d, K): K on both sides of the 16 | 17, 32 | 33 and 48 | 49 boundaries of the sums dispatch, d around the 16-feature slab,
# one chunk and two.  n = 2115 is a second chunk of one 64-row stage and three rows: a second chunk of one row (n = 2049)
# cannot hold rows of the four clusters 15, 16, K - 16 and K - 1.
EDGE_DISPATCH = [(130, 16, 16), (200, 17, 17), (130, 15, 32), (2115, 17, 33), (300, 2, 48), (2115, 16, 49)]
EDGE_BOUNDARIES = [(16, 17), (32, 33), (48, 49), (64, 65)]
EDGE_FOREIGN_K = [16, 20, 64, 65]
EDGE_FOREIGN_ROWS = (63, 64, 2047, 2048, 1, 2110)           # stage edges, chunk edges, both chunks
EDGE_RELOCATION_M = [5, 66]
EDGE_TRANSFORM = [(63, 31, 63), (65, 33, 64), (65, 1, 65), (130, 32, 129), (2049, 8, 256)]
EDGE_VARIANCE = [(1, 1), (2, 3), (2047, 1), (2048, 128), (2049, 17), (4097, 33)]
EDGE_SCAN_RAND = [0.0, 2047 / 4096, 2047.5 / 4096, 2048 / 4096, 4095 / 4096, 4095.5 / 4096, 1.0, 1.5]
EDGE_SCAN_ROWS = [0, 2047, 2048, 2048, 4095, 4096, 4096, 4096]
# (fit case, tol or None for the case's own): two strict stops, and the rows of tol0 stopped by a tolerance of 1e-3
EDGE_CONTROL = [("n300_d5_k4_sep6", None), ("tol0", None), ("tol0", 1e-3)]


def dispatch_case(n, d, k):
    """(float32 rows, centres float64 [k, d]): row r lies around mean r % k, the means 6 apart on a lattice in the first two
    features, the centres near the means; so every cluster has rows in every stretch of k rows"""
    rng = np.random.RandomState(1000 + n + d + k)
    j = np.arange(k)
    means = 2.0 * rng.standard_normal((k, d))
    means[:, 0] = 6.0 * (j % 8)
    means[:, min(1, d - 1)] = 6.0 * (j // 8) if d > 1 else means[:, 0] + 48.0 * (j // 8)
    X32 = (means[np.arange(n) % k] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    return X32, means + 0.1 * rng.standard_normal((k, d))


def boundary_case(k):
    """(float32 rows [2115, 17], labels int32 r % k): one label vector to run at k and at k + 1"""
    X32 = np.random.RandomState(2000 + k).standard_normal((2115, 17)).astype(np.float32)
    return X32, (np.arange(2115) % k).astype(np.int32)


def foreign_case(k, rot):
    """(float32 rows [2115, 17], labels int32, the foreign rows): labels r % k, and at EDGE_FOREIGN_ROWS the values -1, k,
    k + 15, -16, INT32_MAX, INT32_MIN rotated by ``rot``"""
    X32 = (1.0 + np.random.RandomState(3000 + k).standard_normal((2115, 17))).astype(np.float32)
    labels = np.arange(2115) % k
    rows = np.array(EDGE_FOREIGN_ROWS)
    labels[rows] = np.roll([-1, k, k + 15, -16, INT32_MAX, INT32_MIN], rot)
    return X32, labels.astype(np.int32), rows


def relocation_case(m, reverse=False):
    """(rows float64 [2314, 2], init [4 + m, 2]), all integers: the lattice g x g, g = -8 .. 8, and its copy shifted by
    (64, 0), the pair four times (2312 rows, across row 2048), then (1000, 0) and (0, 1000); centres at (0, 0), (64, 0),
    (900, 0), (0, 900) and m far away, empty.  ``reverse`` turns the rows round."""
    g = np.arange(-8.0, 9.0)
    L = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2)
    pair = np.concatenate([L, L + np.array([64.0, 0.0])])
    X = np.concatenate([np.tile(pair, (4, 1)), np.array([[1000.0, 0.0], [0.0, 1000.0]])])
    init = np.array([[0.0, 0.0], [64.0, 0.0], [900.0, 0.0], [0.0, 900.0]] + [[5000.0 + 100.0 * i, 5000.0] for i in range(m)])
    return (X[::-1].copy() if reverse else X), init


def relocation_picks(d2, m):
    """the first m rows in the order (d2 descending, row ascending)"""
    return np.lexsort((np.arange(len(d2)), -d2))[:m]


def many_tiles_case():
    """(float32 rows [16449, 2], init [2, 2]): 258 assign tiles.  Rows 0 .. 16383 alternate around -10 and +10 in feature 0;
    the rows 16384 .. 16448 (tiles 256 and 257) lie between, at 0.001 j, and are the only ones that change their label after
    the first iteration."""
    x0 = np.where(np.arange(16384) % 2 == 0, -10.0, 10.0) + 0.1 * np.random.RandomState(0).standard_normal(16384)
    X = np.zeros((16449, 2))
    X[:, 0] = np.concatenate([x0, 0.001 * np.arange(1, 66)])
    return X.astype(np.float32), np.array([[-10.0, 0.0], [10.5, 0.0]])


def transform_case(n, d, k):
    """(float32 rows, centres float64 [k, d]) as test_assign_and_update_against_the_restatement draws them"""
    X32 = np.random.RandomState(100 + n + d + k).standard_normal((n, d)).astype(np.float32)
    rng = np.random.RandomState(k)
    return X32, X32.astype(np.float64)[rng.choice(n, size=k, replace=k > n)] + 0.25 * rng.standard_normal((k, d))


def variance_case(n, d):
    """float32 rows around 3 with a spread of 2; for d >= 2 the column d // 2 is the constant 3"""
    X32 = (3.0 + 2.0 * np.random.RandomState(4000 + n + d).standard_normal((n, d))).astype(np.float32)
    if d >= 2:
        X32[:, d // 2] = 3.0
    return X32


def column_variances(X):
    """(the column means, the column variances) in the chunk order"""
    X = np.asarray(X, dtype=np.float64)
    mean = chunk_sum(X) / len(X)
    return mean, chunk_sum((X - mean) ** 2) / len(X)


def scan_case():
    """rows float64 [4097, 2]: row 0 at the origin, the odd rows at (-1, 0), the even rows from 2 at (1, 0).  From row 0
    closest is 0, 1, 1, ..., scan[r] = r and the potential 4096, all exact; from row 2047 closest is 1, 0, 4, 0, 4, ...: a
    scan of plateaus that run over both chunk boundaries, 1 + 4 j, the potential 8193."""
    X = np.zeros((4097, 2))
    X[1::2, 0] = -1.0
    X[2::2, 0] = 1.0
    return X


def plateau_thresholds():
    """(rand [T], the thresholds rand * 8193 [T]) for scan_case from row 2047.  The first are dyadic, so their products are
    exact and lie between two plateaus; the others are fitted so that the fp64 product is exactly a plateau value or the
    integer after it (8193 is odd: no dyadic number below 1 gives an integer)."""
    pot = 8193.0
    rand = [j / 2048.0 for j in (0, 1, 512, 1023, 1024, 1025, 2047, 2048)]
    for target in (1.0, 2.0, 5.0, 6.0, 4093.0, 4094.0, 4097.0, 4098.0, 8189.0, 8190.0):
        r = target / pot
        for _ in range(8):
            if r * pot == target:
                break
            r = np.nextafter(r, np.inf if r * pot < target else -np.inf)
        rand.append(float(r))
    rand = np.array(rand)
    return rand, rand * pot


def plusplus_trial(X, closest, rand):
    """one step of ``plusplus_steps`` from ``closest``: (the candidates [L], their potentials [L], the position of the
    chosen one, the new closest)"""
    X = np.asarray(X, dtype=np.float64)
    scan = chunk_scan(closest)
    cand = np.minimum(np.searchsorted(scan, np.asarray(rand) * scan[-1]), len(X) - 1)
    dc = np.minimum(closest[None, :], sqd(X[cand], X))
    pots = np.array([chunk_sum(row) for row in dc])
    b = int(np.argmin(pots))
    return cand, pots, b, dc[b]


def lloyd_steps(X, centres, tol_abs, max_iter, trace=None):
    """the iterations of ``lloyd`` one by one, up to and with the one that stops: dicts of labels, d2 (the assignment at
    the centres before), centres (after), shift, changed (the rows whose label changed), strict, stopped"""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(centres, dtype=np.float64)
    old = np.full(len(X), -1, dtype=np.int64)
    steps = []
    for _ in range(max_iter):
        labels, d2 = assign(X, C, trace)
        C, shift = update(X, labels, d2, C)
        strict = bool(np.array_equal(labels, old))
        if not strict and tol_abs > 0:
            _note(trace, 'shift', abs(shift - tol_abs) / tol_abs)
        steps.append(dict(labels=labels.astype(np.int32), d2=d2, centres=C.copy(), shift=shift,
                          changed=np.flatnonzero(labels != old), strict=strict, stopped=strict or shift <= tol_abs))
        if steps[-1]['stopped']:
            break
        old = labels
    return steps


def control_case(name, tol=None):
    """(rows, the k-means++ start of the fit case, tol, the absolute tolerance)"""
    X, kw = fit_case(name)
    start = X[plusplus(X, kw['n_clusters'], np.random.RandomState(kw['random_state']))]
    tol = kw.get('tol', 1e-4) if tol is None else tol
    return X, start, tol, mean_variance(X) * tol


def permuted_lattice_case():
    """(the 256 rows of a 16 x 16 lattice, the same rows permuted as init, the permutation)"""
    g = np.arange(16.0)
    X = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2)
    perm = np.random.RandomState(3).permutation(256)
    return X, X[perm].copy(), perm
