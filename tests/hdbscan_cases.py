"""Cases and the numpy restatement for ava_amd.hdbscan (row f23).

The restatement is scikit-learn 1.7.2's HDBSCAN (sklearn/cluster/_hdbscan: hdbscan.py, _reachability.pyx, _linkage.pyx,
_tree.pyx) with ONE stated deviation, the order of the edges.  With ``m(i, j)`` the pair measure (the squared distance
by direct differences, or the precomputed distance), ``core(i)`` the ``min_samples``-th smallest ``m(i, .)`` (the row
itself first) and ``w(i, j) = max(core(i), core(j), m(i, j))``, edges are compared by the key

    (w(i, j), m(i, j), min(i, j), max(i, j))

lexicographically.  That is a strict total order, so the minimum spanning tree is unique: a Kruskal over all pairs
sorted by the key gives it, already in the order in which ``make_single_linkage`` wants it.  (sklearn breaks ties in
``w`` by Prim's visiting order followed by an unstable argsort.)  From there ``make_single_linkage``, ``_condense_tree``,
``_compute_stability``, ``_get_clusters`` ('eom' and 'leaf'), ``_do_labelling`` and ``get_probabilities`` are
transcribed line by line, with ``allow_single_cluster=False``, ``cluster_selection_epsilon=0`` and
``max_cluster_size=None``.  Reported distances are ``sqrt(w)`` (euclidean) or ``w`` (precomputed).  Clusters are
numbered in ascending order of their smallest row.

Inputs are exact.  Every euclidean case lies on a grid of 2^-12 and is stored as float32, with coordinates small enough
that every difference, square and sum is exact in fp64 in any order, with or without fma: the device's d2, numpy's and
longdouble's are the same numbers (tests/test_cpu_hdbscan.py checks it), every key comparison is decidable and edges and
labels compare with ``==``.  The one place where rounding decides is ``subtree_stability > stability[node]`` in the
'eom' selection, sums of reciprocals of square roots: ``stability_gap`` is the smallest relative gap of those
comparisons, and the blob cases are generated with a gap of at least ``GAP`` = 1e-9.

It is the oracle of the GPU tests; tests/test_cpu_hdbscan.py holds it against sklearn itself and
tests/golden/hdbscan.npz."""
import functools

import numpy as np

import dbscan_cases as DC

GAP = 1e-9
U = 2.0 ** -53
GRID = 4096.0


# ---- the restatement -------------------------------------------------------------------------------------------------
def measures(X, metric='euclidean', dtype=np.float64, reverse=False):
    """[N, N] pair measures: squared distances by direct differences (features ascending, or descending with
    ``reverse``) in ``dtype``, or the precomputed matrix itself"""
    X = np.asarray(X, dtype=dtype)
    if metric == 'precomputed':
        return X.copy()
    out = np.zeros((len(X), len(X)), dtype=dtype)
    cols = range(X.shape[1])
    for c in (reversed(cols) if reverse else cols):
        diff = X[:, c][:, None] - X[:, c][None, :]
        out += diff * diff
    return out


def core_measures(M, min_samples):
    """the ``min_samples``-th smallest of every row, the row itself (0) counted first"""
    M = M.copy()
    np.fill_diagonal(M, 0.0)
    return np.sort(M, axis=1)[:, min_samples - 1]


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def kruskal(M, core):
    """the N - 1 edges of the minimum spanning tree under the key, in key order: (i, j, w, m) arrays, i < j"""
    n = len(M)
    I, J = np.triu_indices(n, 1)
    m = M[I, J]
    w = np.maximum(np.maximum(core[I], core[J]), m)
    order = np.lexsort((J, I, m, w))
    I, J, m, w = I[order], J[order], m[order], w[order]
    parent = list(range(n))
    lab = np.arange(n)
    out = []
    for lo in range(0, len(I), 8192):
        if len(out) == n - 1:
            break
        live = np.flatnonzero(lab[I[lo:lo + 8192]] != lab[J[lo:lo + 8192]]) + lo
        for p in live.tolist():
            a, b = _find(parent, int(I[p])), _find(parent, int(J[p]))
            if a != b:
                parent[max(a, b)] = min(a, b)
                out.append(p)
        lab = np.asarray([_find(parent, x) for x in range(n)])
    out = np.asarray(out, dtype=np.int64)
    assert len(out) == n - 1
    return I[out].astype(np.int64), J[out].astype(np.int64), w[out], m[out]


def single_linkage(I, J, dist):
    """make_single_linkage: [N - 1, 4] float64, node N + e the union of the clusters of edge e's rows"""
    n = len(I) + 1
    up = [-1] * (2 * n - 1)
    size = [1] * (2 * n - 1)

    def find(x):
        r = x
        while up[r] >= 0:
            r = up[r]
        while up[x] >= 0:
            up[x], x = r, up[x]
        return r
    out = np.zeros((n - 1, 4))
    for e in range(n - 1):
        a, b = find(int(I[e])), find(int(J[e]))
        assert a != b
        up[a] = up[b] = n + e
        size[n + e] = size[a] + size[b]
        out[e] = (a, b, dist[e], size[n + e])
    return out


def _bfs(tree, start, n):
    out, queue = [], [start]
    while queue:
        out.extend(queue)
        queue = [x - n for x in queue if x >= n]
        queue = [int(c) for x in queue for c in (tree[x, 0], tree[x, 1])]
    return out


def condense(tree, min_cluster_size):
    """_condense_tree: a list of (parent, child, lambda, size)"""
    n = len(tree) + 1
    root = 2 * (n - 1)
    relabel = {root: n}
    next_label = n + 1
    ignore = set()
    out = []
    with np.errstate(divide='ignore'):
        for node in _bfs(tree, root, n):
            if node in ignore or node < n:
                continue
            left, right, distance = int(tree[node - n, 0]), int(tree[node - n, 1]), tree[node - n, 2]
            lam = 1.0 / distance if distance > 0.0 else np.inf
            lc = int(tree[left - n, 3]) if left >= n else 1
            rc = int(tree[right - n, 3]) if right >= n else 1
            if lc >= min_cluster_size and rc >= min_cluster_size:
                relabel[left] = next_label
                next_label += 1
                out.append((relabel[node], relabel[left], lam, lc))
                relabel[right] = next_label
                next_label += 1
                out.append((relabel[node], relabel[right], lam, rc))
                continue
            shed = []
            if lc < min_cluster_size:
                shed.append(left)
            else:
                relabel[left] = relabel[node]
            if rc < min_cluster_size:
                shed.append(right)
            else:
                relabel[right] = relabel[node]
            for start in shed:
                for sub in _bfs(tree, start, n):
                    if sub < n:
                        out.append((relabel[node], sub, lam, 1))
                    ignore.add(sub)
    return out


def select(cond, n, method):
    """_compute_stability, _get_clusters, _do_labelling, get_probabilities on a condensed tree: labels in sklearn's
    numbering, probabilities, and the smallest relative gap of the 'eom' comparisons"""
    births = {child: lam for _, child, lam, _ in cond}
    births[n] = 0.0
    stab = {p: 0.0 for p, _, _, _ in cond}
    with np.errstate(invalid='ignore'):
        for p, _, lam, size in cond:
            stab[p] += (lam - births[p]) * size
    ctree = [(p, c) for p, c, _, size in cond if size > 1]
    kids = {}
    for p, c in ctree:
        kids.setdefault(p, []).append(c)
    nodes = sorted(stab, reverse=True)[:-1]
    is_cluster = {c: True for c in nodes}
    gap = np.inf

    def below(node):
        out, queue = [], list(kids.get(node, []))
        while queue:
            out.extend(queue)
            queue = [c for x in queue for c in kids.get(x, [])]
        return out
    if method == 'eom':
        for node in nodes:
            subtree = float(np.sum([stab[c] for c in kids.get(node, [])]))
            big = max(abs(subtree), abs(stab[node]))
            if np.isfinite(big):
                gap = min(gap, abs(subtree - stab[node]) / big if big > 0.0 else 0.0)
            if subtree > stab[node]:
                is_cluster[node] = False
                stab[node] = subtree
            else:
                for sub in below(node):
                    is_cluster[sub] = False
    else:
        for c in nodes:
            is_cluster[c] = c not in kids
    clusters = sorted(c for c in is_cluster if is_cluster[c])
    number = {c: k for k, c in enumerate(clusters)}
    # _do_labelling: a union of every child that is no selected cluster with its parent; the representative is the top
    top = {n: n}
    for p, c in ctree:                                                     # parents come before their children
        top[c] = c if c in number else top[p]
    labels = np.full(n, -1, dtype=np.int64)
    for p, c, _, _ in cond:
        if c < n and top[p] != n:
            labels[c] = number[top[p]]
    # max_lambdas: the largest lambda of the LAST run of consecutive rows of a parent (as sklearn computes it)
    deaths = {p: 0.0 for p in stab}
    current, max_lambda = cond[0][0], cond[0][2]
    for p, _, lam, _ in cond[1:]:
        if p == current:
            max_lambda = max(max_lambda, lam)
        else:
            deaths[current] = max_lambda
            current, max_lambda = p, lam
    deaths[current] = max_lambda
    prob = np.zeros(n)
    for p, c, lam, _ in cond:
        if c >= n or labels[c] == -1:
            continue
        max_lambda = deaths[clusters[labels[c]]]
        prob[c] = 1.0 if max_lambda == 0.0 or np.isinf(lam) else min(lam, max_lambda) / max_lambda
    return labels, prob, float(gap)


def renumber(labels):
    """clusters numbered in ascending order of their smallest row; noise stays -1"""
    out = np.full(len(labels), -1, dtype=np.int64)
    number = {}
    for i, l in enumerate(np.asarray(labels).tolist()):
        if l >= 0:
            out[i] = number.setdefault(l, len(number))
    return out


def restate(X, min_cluster_size, min_samples=None, metric='euclidean', method='eom'):
    """dict of labels, probabilities, mst [N - 1, 3] (i, j, distance), weights / raw (the edges' w and m), core (the
    core measures, squared for euclidean), core_distances, linkage, n_clusters, n_noise, stability_gap, hub_rows"""
    k = min_cluster_size if min_samples is None else min_samples
    M = measures(X, metric)
    core = core_measures(M, k)
    I, J, w, m = kruskal(M, core)
    dist = np.sqrt(w) if metric == 'euclidean' else w.copy()
    tree = single_linkage(I, J, dist)
    labels, prob, gap = select(condense(tree, min_cluster_size), len(M), method)
    labels = renumber(labels)
    # informative only: rows that carry two or more tree edges at exactly their own core measure (they join two
    # sides at one level, and an order without the key's tiebreak may attach them to either)
    at_core = np.concatenate([I[w == core[I]], J[w == core[J]]])
    hub = np.flatnonzero(np.bincount(at_core, minlength=len(M)) >= 2)
    return dict(labels=labels, probabilities=prob, mst=np.stack([I.astype(np.float64), J.astype(np.float64), dist], 1),
                edges=(I, J), weights=w, raw=m, core=core,
                core_distances=np.sqrt(core) if metric == 'euclidean' else core.copy(), linkage=tree,
                n_clusters=int(labels.max()) + 1, n_noise=int((labels == -1).sum()), stability_gap=gap, hub_rows=hub)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def on_grid(X, limit=64.0):
    """rounded to the grid of 2^-12 inside [-limit, limit], as float32"""
    out = np.clip(np.round(np.asarray(X, dtype=np.float64) * GRID) / GRID, -limit, limit).astype(np.float32)
    assert np.all(out.astype(np.float64) * GRID == np.round(out.astype(np.float64) * GRID))
    return out


def blob_rows(n, d, c, seed):
    return on_grid(DC.blobs(n, d, c, seed))


# name: (N, d, centres, first seed, min_cluster_size, min_samples)
BLOBS = {
    "n63_d31": (63, 31, 2, 2301, 5, None),
    "n64_d32": (64, 32, 2, 2302, 5, None),
    "n65_d33": (65, 33, 2, 2303, 8, 4),
    "n65_d65": (65, 65, 2, 2304, 5, None),
    "n128_d2": (128, 2, 3, 2305, 8, 4),
    "n129_d1": (129, 1, 3, 2306, 10, 5),
    "n257_d32": (257, 32, 4, 2307, 15, 3),
    "n1650_d32": (1650, 32, 5, 2308, 25, 10),
}
# the seed each blob case settles on (find_seed; tests/test_cpu_hdbscan.py and the golden file hold it)
SEEDS = {
    "n63_d31": 2301,
    "n64_d32": 2302,
    "n65_d33": 2303,
    "n65_d65": 2304,
    "n128_d2": 2305,
    "n129_d1": 2306,
    "n257_d32": 2307,
    "n1650_d32": 2308,
}
SKLEARN_ALGORITHMS = ("brute", "kd_tree", "ball_tree")


def sklearn_fit(X, min_cluster_size, min_samples, algorithm, method='eom'):
    from sklearn.cluster import HDBSCAN
    return HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, algorithm=algorithm,
                   cluster_selection_method=method, copy=True).fit(np.asarray(X, dtype=np.float64))


def generator_condition(X, min_cluster_size, min_samples):
    """the restatement's partition equals sklearn's under every algorithm, at least two clusters, some noise, and a
    stability gap of at least GAP"""
    r = restate(X, min_cluster_size, min_samples)
    if r["n_clusters"] < 2 or r["n_noise"] == 0 or not r["stability_gap"] >= GAP:
        return False
    mine = DC.by_smallest_member(r["labels"])
    return all(np.array_equal(mine, DC.by_smallest_member(sklearn_fit(X, min_cluster_size, min_samples, a).labels_))
               for a in SKLEARN_ALGORITHMS)


def find_seed(name):
    """the first seed, in steps of 1000 from the case's own, whose draw meets the generator condition"""
    n, d, c, seed, mcs, ms = BLOBS[name]
    for s in range(seed, seed + 20000, 1000):
        if generator_condition(blob_rows(n, d, c, s), mcs, ms):
            return s
    raise AssertionError("no draw meets the generator condition")


def _blob_case(name):
    def make():
        n, d, c, _, mcs, ms = BLOBS[name]
        return blob_rows(n, d, c, SEEDS[name]), mcs, ms, 'eom'
    return make


def _with(name, **changes):
    def make():
        X, mcs, ms, method = _blob_case(name)()
        return X, changes.get("mcs", mcs), changes.get("ms", ms), changes.get("method", method)
    return make


def _pair_case():
    return np.asarray([[0.25, 1.0], [0.25, 2.0]], dtype=np.float32), 2, 1, 'eom'


def _chain_case(order):
    def make():
        X = on_grid(DC.chain_rows(), limit=512.0)
        if order == "desc":
            X = X[::-1].copy()
        elif order == "shuf":
            X = X[np.random.default_rng(2311).permutation(len(X))]
        return X, 5, 3, 'eom'
    return make


def _lattice_case():
    """a 12 x 12 integer lattice with two 3 x 3 patches at half the spacing, shuffled: most keys tie in (w, m)"""
    g = np.stack(np.divmod(np.arange(144), 12), axis=1).astype(np.float64)
    fine = np.stack(np.divmod(np.arange(9), 3), axis=1) * 0.5
    X = np.concatenate([g, fine + [2.25, 2.25], fine + [8.25, 7.25]])
    return on_grid(X[np.random.default_rng(2312).permutation(len(X))]), 5, 4, 'eom'


def _duplicates_case():
    """four copies of one row and three of another beside a blob: merge distance 0, lambda = inf"""
    X = blob_rows(40, 3, 1, 2313).copy()
    X[5:9] = X[5]
    X[20:23] = X[20]
    return X, 3, 3, 'eom'


HUB = 5


def _hub_case():
    """rows 0..4 (group B, around x = 10) and rows 6..10 (group A, around x = 0) with one sparse row between them,
    row 5 at x = 5.  Its nearest rows are row 4 at x = 9 and row 6 at x = 1, both at squared distance 16, so with
    min_samples = 3 its core measure is 16 and the edges (4, 5) and (5, 6) have the same (w, m) = (16, 16); every
    other row's core measure is at most 1 and A and B are 64 apart (squared).  Under the key (4, 5) comes first: the hub joins B,
    the group of row 0, so its label is 0, and A is cluster 1."""
    xs = [10.0, 10.5, 11.0, 9.5, 9.0, 5.0, 1.0, 0.5, 0.0, -0.5, -1.0]
    ys = [0.0, 0.25, 0.0, 0.25, 0.0, 0.0, 0.0, 0.25, 0.0, 0.25, 0.0]
    return on_grid(np.stack([xs, ys], axis=1)), 5, 3, 'eom'


CASES = dict([(name, _blob_case(name)) for name in BLOBS] + [
    ("n2", _pair_case),
    ("chain_asc", _chain_case("asc")),
    ("chain_desc", _chain_case("desc")),
    ("chain_shuf", _chain_case("shuf")),
    ("lattice", _lattice_case),
    ("duplicates", _duplicates_case),
    ("hub", _hub_case),
    ("leaf_n257_d32", _with("n257_d32", method='leaf')),
    ("leaf_n129_d1", _with("n129_d1", method='leaf')),
    ("ms64_n257_d32", _with("n257_d32", ms=64)),
])
BLOB_CASES = tuple(BLOBS)
PRECOMPUTED_CASES = ("n65_d33", "n257_d32", "hub", "chain_shuf")


@functools.lru_cache(maxsize=None)
def case(name):
    """(X float32 [N, d], min_cluster_size, min_samples or None, method)"""
    X, mcs, ms, method = CASES[name]()
    X.setflags(write=False)
    return X, mcs, ms, method


@functools.lru_cache(maxsize=None)
def expected(name):
    X, mcs, ms, method = case(name)
    return restate(X, mcs, ms, method=method)


def permutation(name):
    return np.random.default_rng(5).permutation(len(case(name)[0]))


def same_partition(labels, permuted_labels, perm):
    """whether the labels of the permuted rows, taken back to the original rows, are the same partition"""
    back = np.empty(len(perm), dtype=np.int64)
    back[perm] = permuted_labels
    return bool(np.array_equal(DC.by_smallest_member(back), DC.by_smallest_member(labels)))


@functools.lru_cache(maxsize=None)
def permutation_invariant(name):
    """whether the restatement gives the same partition on the rows in the order of ``permutation(name)``: the key's
    last two entries are rows, so a case whose tree hangs on a row tiebreak need not be"""
    X, mcs, ms, method = case(name)
    perm = permutation(name)
    return same_partition(expected(name)["labels"], restate(X[perm], mcs, ms, method=method)["labels"], perm)


# the cases for which permutation_invariant holds (tests/test_cpu_hdbscan.py asserts exactly these)
INVARIANT_CASES = tuple(name for name in CASES if name != "lattice")


@functools.lru_cache(maxsize=None)
def precomputed(name):
    """the case's own matrix of squared distances (exact, symmetric, zero diagonal) and its restatement under
    metric='precomputed': the same keys, so the same tree and labels, with distances w in place of sqrt(w)"""
    X, mcs, ms, method = case(name)
    D = measures(X)
    return D, restate(D, mcs, ms, metric='precomputed', method=method)
