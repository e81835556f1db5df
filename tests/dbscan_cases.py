"""Cases and the numpy restatement for ava_amd.dbscan (row f22).

Inputs are generated from ``np.random.default_rng(seed)`` and rounded to float32, so a float32 and a float64 copy mean the
same data.  The restatement states scikit-learn 1.7's DBSCAN (sklearn/cluster/_dbscan.py, _dbscan_inner.pyx) as four
rules, with every squared distance in ``np.longdouble`` by direct differences and compared with ``longdouble(eps)^2``:

* row i is a core row when #{j : dist(i, j) <= eps} >= min_samples, itself included;
* the clusters are the connected components of the core rows under dist <= eps (a host union-find), numbered
  0, 1, .. in ascending order of their smallest row;
* a non-core row with core rows within eps takes the smallest cluster number among them;
* every other row is -1.

It is the oracle of the GPU tests; tests/test_cpu_dbscan.py holds it against sklearn itself (all four ``algorithm``
settings) and tests/golden/dbscan.npz.

Margin.  A case's margin is ``min over pairs |d2 - eps^2| / eps^2`` (``|D - eps| / eps`` for a precomputed matrix).  The
device's d2 is d fused multiply-adds of exact differences of float32 values (exact in fp64 whenever the exponents are
within 29 binades, once-rounded otherwise), within (d + 2) 2^-53 ~ 7e-15 relative of exact for d <= 65; sklearn's own
arithmetic is within about 1e-13 on data of this scale.  Every case that is not a tie case is generated with a margin of
at least ``MARGIN`` = 1e-9 (the generator moves on to the next seed until a draw has it), so no arithmetic can flip a
pair and labels compare with ``==``.  Tie cases have integer coordinates |x| <= 2^20 and an integer eps: every sum is
exact in every arithmetic, and ``<=`` against ``<`` is decidable."""
import functools

import numpy as np

LD = np.longdouble
MARGIN = 1e-9
U = 2.0 ** -53


# ---- the restatement -------------------------------------------------------------------------------------------------
def sqdist(X):
    """[N, N] longdouble squared distances by direct differences, features ascending"""
    X = np.asarray(X, dtype=LD)
    out = np.zeros((len(X), len(X)), dtype=LD)
    for c in range(X.shape[1]):
        diff = X[:, c][:, None] - X[:, c][None, :]
        out += diff * diff
    return out


def within(X, eps, metric='euclidean'):
    """the boolean [N, N] neighbourhood matrix and the case's margin"""
    if metric == 'precomputed':
        D, lim = np.asarray(X, dtype=LD), LD(eps)
    else:
        D, lim = sqdist(X), LD(eps) * LD(eps)
    return D <= lim, float((np.abs(D - lim) / lim).min())


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def restate(W, min_samples):
    """the four rules on a neighbourhood matrix: dict of labels, core (bool), core_idx, counts, n_clusters, n_border,
    n_noise and ambiguous (the number of border rows with core neighbours in more than one cluster)"""
    n = len(W)
    counts = W.sum(axis=1).astype(np.int64)
    core = counts >= min_samples
    parent = list(range(n))
    rows, cols = np.nonzero(np.triu(W & core[:, None] & core[None, :], 1))
    for i, j in zip(rows.tolist(), cols.tolist()):
        a, b = _find(parent, i), _find(parent, j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    labels = np.full(n, -1, dtype=np.int64)
    number = {}
    for i in range(n):                                                 # ascending: a component's smallest row comes first
        if core[i]:
            labels[i] = number.setdefault(_find(parent, i), len(number))
    ambiguous = 0
    core_labels = labels.copy()
    for i in np.flatnonzero(~core):
        near = core_labels[W[i] & core]
        if len(near):
            labels[i] = near.min()
            ambiguous += len(np.unique(near)) > 1
    border = ~core & (labels >= 0)
    return dict(labels=labels, core=core, core_idx=np.flatnonzero(core).astype(np.int64), counts=counts,
                n_clusters=len(number), n_border=int(border.sum()), n_noise=int((labels == -1).sum()),
                ambiguous=int(ambiguous))


def kth_distances(X, k):
    """sorted float64 distances to the k-th nearest row, the row itself counted first"""
    D = np.sort(sqdist(X), axis=1)[:, k - 1]
    return np.sort(np.sqrt(D)).astype(np.float64)


def by_smallest_member(labels, rows=None):
    """the partition of ``rows`` (default: the rows with a label >= 0) renumbered by each part's smallest member"""
    labels = np.asarray(labels)
    keep = labels >= 0 if rows is None else rows
    out = np.full(len(labels), -1, dtype=np.int64)
    first = {}
    for i in np.flatnonzero(keep):
        out[i] = first.setdefault(labels[i], i)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------
def blobs(n, d, c, seed, noise=0.2, spread=6.0):
    """``c`` unit Gaussian blobs with centres ``spread`` N(0, 1) apart and about ``noise`` n uniform rows in the box
    around them, in shuffled order, float32"""
    rng = np.random.default_rng(seed)
    n_noise = int(round(noise * n)) if n >= 8 else 0
    centres = spread * rng.standard_normal((c, d))
    X = centres[np.arange(n - n_noise) % c] + rng.standard_normal((n - n_noise, d))
    lo, hi = X.min(axis=0) - 2.0, X.max(axis=0) + 2.0
    X = np.concatenate([X, lo + (hi - lo) * rng.random((n_noise, d))])
    return X[rng.permutation(n)].astype(np.float32)


def radius_at(X, min_samples, quantile):
    """a radius between two neighbouring values of the sorted ``min_samples``-th distances: about ``quantile`` of the
    rows are core rows.  Two rows that are each other's ``min_samples``-th neighbour share that distance, and their
    midpoint would be a distance of the data: the position moves up until the radius keeps the margin."""
    D2 = sqdist(X)
    kd = np.sort(np.sqrt(np.sort(D2, axis=1)[:, min_samples - 1])).astype(np.float64)
    for q in range(min(int(quantile * len(kd)), len(kd) - 2), len(kd) - 1):
        r = float(0.5 * (kd[q] + kd[q + 1]))
        lim = LD(r) * LD(r)
        if float((np.abs(D2 - lim) / lim).min()) >= MARGIN:
            return r
    raise AssertionError("no radius at the margin")


def _blob_case(n, d, c, seed, min_samples=4, quantile=0.6):
    """blobs whose restatement has core rows, border rows and noise at a margin >= MARGIN; the seed moves on in steps
    of 1000 until a draw has all of that"""
    def make():
        for s in range(seed, seed + 20000, 1000):
            X = blobs(n, d, c, s)
            eps = radius_at(X, min_samples, quantile)
            W, margin = within(X, eps)
            r = restate(W, min_samples)
            if margin >= MARGIN and len(r["core_idx"]) and r["n_border"] and r["n_noise"]:
                return X, eps, min_samples
        raise AssertionError("no draw with core rows, border rows and noise at the margin")
    return make


def _pair_case():
    """two rows 1 apart"""
    return np.asarray([[0.25, 1.0], [0.25, 2.0]], dtype=np.float32), 1.5, 2


def _single_case():
    return np.asarray([[3.5]], dtype=np.float32), 0.5, 1


def chain_rows(seed=2200):
    """600 rows along a noisy line in d = 3, about 0.8 eps apart (eps = 1), in ascending order along the line"""
    rng = np.random.default_rng(seed)
    X = 0.04 * (rng.random((600, 3)) - 0.5)
    X[:, 0] += 0.8 * np.arange(600)
    return X.astype(np.float32)


def _chain_case(order):
    def make():
        X = chain_rows()
        if order == "desc":
            X = X[::-1].copy()
        elif order == "shuf":
            X = X[np.random.default_rng(2201).permutation(len(X))]
        return X, 1.0, 3
    return make


def _bridge_case():
    """two dense groups, A around (0, 0) and B around (3, 0), and a bridge row (row 11) within eps = 1 of exactly one
    core row of each: row 1 of B and row 10 of A.  A owns row 0, so A is cluster 0 and B cluster 1: the bridge's
    smallest-index core neighbour (row 1) is in the HIGHER cluster, and the bridge's label is 0."""
    rng = np.random.default_rng(2210)
    jitter = lambda m: 0.1 * (rng.random((m, 2)) - 0.5)                 # noqa: E731
    X = np.zeros((13, 2))
    X[0] = [0.0, 0.0]
    X[1] = [2.4, 0.0]
    X[2:6] = np.asarray([3.0, 0.0]) + jitter(4)
    X[6:10] = jitter(4)
    X[10] = [0.6, 0.0]
    X[11] = [1.5, 0.0]
    X[12] = [40.0, 40.0]
    return X.astype(np.float32), 1.0, 4


def _ties_case():
    """integers on a line with gaps, eps = 1, min_samples = 3: pairs at distance exactly eps, rows with exactly
    min_samples neighbours (1, 2, 11: core), border rows (0, 3, 10, 12), rows with fewer and no core row near (noise)"""
    pos = np.asarray([0, 1, 2, 3, 5, 6, 8, 10, 11, 12, 20], dtype=np.float64) + (2 ** 20 - 40)
    X = np.stack([pos, np.full(len(pos), -(2.0 ** 20))], axis=1)
    return X.astype(np.float32), 1.0, 3


def _duplicates_case():
    """min_samples = 4 copies of one isolated row are a cluster of their own (distance exactly 0); 3 copies of another
    are noise; a blob beside them"""
    X = blobs(40, 3, 1, 2230, noise=0.0)
    X[5:9] = X[5] + np.float32(30.0)
    X[20:23] = X[20] - np.float32(30.0)
    return X, 1.0, 4


def _degenerate(which):
    def make():
        X = blobs(65, 2, 2, 2240)
        return {"ms1": (X, 0.4, 1), "msN1": (X, 0.8, len(X) + 1), "huge": (X, 1.0e6, 5),
                "tiny": (X, 1.0e-6, 2)}[which]
    return make


CASES = {
    "n1_d1": _single_case,
    "n2_d2": _pair_case,
    "n63_d31": _blob_case(63, 31, 2, 2001),
    "n63_d1": _blob_case(63, 1, 2, 2002),
    "n64_d32": _blob_case(64, 32, 2, 2003),
    "n65_d33": _blob_case(65, 33, 2, 2004),
    "n65_d65": _blob_case(65, 65, 2, 2005),
    "n128_d65": _blob_case(128, 65, 3, 2006),
    "n128_d2": _blob_case(128, 2, 3, 2007),
    "n129_d1": _blob_case(129, 1, 3, 2008),
    "n129_d31": _blob_case(129, 31, 3, 2009),
    "n257_d2": _blob_case(257, 2, 4, 2010),
    "n257_d32": _blob_case(257, 32, 4, 2011),
    "chain_asc": _chain_case("asc"),
    "chain_desc": _chain_case("desc"),
    "chain_shuf": _chain_case("shuf"),
    "bridge": _bridge_case,
    "ties": _ties_case,
    "duplicates": _duplicates_case,
    "deg_ms1": _degenerate("ms1"),
    "deg_msN1": _degenerate("msN1"),
    "deg_huge": _degenerate("huge"),
    "deg_tiny": _degenerate("tiny"),
    "blobs1500_d32": _blob_case(1650, 32, 5, 2050, min_samples=10, quantile=0.5),
}
TIE_CASES = ("ties",)
# core rows, border rows and noise are all present (impossible below 4 rows: a border row needs a core row with a
# neighbour the border row lacks, and the noise a fourth row)
MIXED_CASES = tuple(n for n in CASES if n.startswith("n") and n not in ("n1_d1", "n2_d2")) + ("blobs1500_d32",)
SWEEP_CASE = "n257_d32"


@functools.lru_cache(maxsize=None)
def case(name):
    """(X float32 [N, d], eps, min_samples)"""
    X, eps, min_samples = CASES[name]()
    X.setflags(write=False)
    return X, float(eps), int(min_samples)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement of a case, with its ``margin``"""
    X, eps, min_samples = case(name)
    W, margin = within(X, eps)
    out = restate(W, min_samples)
    out["margin"] = margin
    return out


@functools.lru_cache(maxsize=None)
def sweep_radii(count):
    """``count`` radii for SWEEP_CASE from all noise (below the smallest ``min_samples``-th distance) to one cluster
    (above the largest pair distance), each at a margin >= MARGIN"""
    X, _, min_samples = case(SWEEP_CASE)
    if count < 3:
        radii = [radius_at(X, min_samples, q) for q in (0.6, 0.3)[:count]]
    else:
        kd = kth_distances(X, min_samples)
        top = float(np.sqrt(sqdist(X).max()))
        radii = [0.5 * kd[0]] + [radius_at(X, min_samples, q) for q in np.linspace(0.1, 0.95, count - 2)] + [1.5 * top]
    radii = [float(r) for r in radii]
    for r in radii:
        assert within(X, r)[1] >= MARGIN, r
    return tuple(radii)


def precomputed(name):
    """the case's distances: the longdouble squared distances' square roots rounded to float64, and the margin of the
    case's eps against them"""
    X, eps, _ = case(name)
    D = np.sqrt(sqdist(X)).astype(np.float64)
    D = np.maximum(D, D.T)
    np.fill_diagonal(D, 0.0)
    return D, within(D, eps, 'precomputed')[1]
