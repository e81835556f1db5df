"""Cases and the numpy restatement for ava_amd.knn_predict (row f24).

Inputs are generated from ``np.random.default_rng(seed)`` and rounded to float32, so a float32 and a float64 copy mean the
same data.  The restatement states scikit-learn 1.7's ``cross_val_predict(KNeighbors*(algorithm='brute'),
cv=PredefinedSplit(fold))`` in ``np.longdouble``:

* squared distances by direct differences, features ascending;
* the neighbours of row i are the first k of ``lexsort((index, d2))`` among the rows of other folds;
* weights: 1, or ``1 / sqrt(d2)``, except in a row whose first neighbour is at distance 0, where they are ``d2 == 0``
  (sklearn's ``_get_weights``);
* the class is the arg-max of the summed weights by (score descending, class ascending); the regression value is
  ``sum w Y / sum w``.

It is the oracle of the GPU tests; tests/test_cpu_knnpred.py holds it against sklearn itself and
tests/golden/knnpred.npz.

Margin.  The device's d2 is d fused multiply-adds of exact differences of float32 values, within (d + 2) 2^-53 ~ 4e-15
relative of exact for d <= 33; sklearn expands |x|^2 + |y|^2 - 2xy, within about 1e-13 on rows of this scale (standard
normal rows: |x|^2 is of the order of the squared distances).  Every case is generated so that for every row (the
generator moves on to the next seed until a draw has it)

* the first kmax + 1 eligible squared distances have consecutive relative gaps >= ``MARGIN`` = 1e-9, so no arithmetic can
  reorder a neighbour list and indices compare with ``==``;
* under ``'distance'`` weights the best two class scores at every k of the sweep differ by >= 1e-9 relative, so classes
  compare with ``==``.  Under ``'uniform'`` the scores are integers, exact in every arithmetic: ties are kept and the
  class rule decides them.  A row with a neighbour at distance 0 has weights 0 / 1 and is exact in the same way.

The duplicate case is the exception on purpose: rows 5 and 77 are equal and in different folds, so they are at exactly
equal distance (the same bits in every arithmetic) from every third row and the index decides; sklearn leaves that tie
undefined, and the case is compared with the restatement only.

Regression bound.  For every element |device - restatement| <= (2k + 6) 2^-53 sum_s |w_s Y_s| / sum_s w_s: k fused
multiply-adds, k adds, one division, and one rounding each for the square root and the reciprocal of a weight."""
import functools

import numpy as np

LD = np.longdouble
MARGIN = 1e-9
U = 2.0 ** -53
N_CLASSES = 4
N_OUT = 3
WEIGHTS = ('uniform', 'distance')


# ---- the restatement -------------------------------------------------------------------------------------------------
def sqdist(X):
    """[N, N] longdouble squared distances by direct differences, features ascending"""
    X = np.asarray(X, dtype=LD)
    out = np.zeros((len(X), len(X)), dtype=LD)
    for c in range(X.shape[1]):
        diff = X[:, c][:, None] - X[:, c][None, :]
        out += diff * diff
    return out


def neighbours(D2, fold, k):
    """(idx int64 [N, k], d2 longdouble [N, k]): the first k rows of other folds by (d2, index)"""
    n = len(D2)
    idx = np.empty((n, k), dtype=np.int64)
    d2 = np.empty((n, k), dtype=LD)
    for i in range(n):
        elig = np.flatnonzero(fold != fold[i])
        order = elig[np.lexsort((elig, D2[i, elig]))][:k]
        idx[i] = order
        d2[i] = D2[i, order]
    return idx, d2


def slot_weights(d2, weighted):
    """[N, k] longdouble weights of a sorted table of squared distances"""
    if not weighted:
        return np.ones(d2.shape, dtype=LD)
    dist = np.sqrt(d2)
    zero_row = dist[:, 0] == 0
    with np.errstate(divide='ignore'):
        w = LD(1) / dist
    w[zero_row] = (dist[zero_row] == 0).astype(LD)
    return w


def class_scores(idx, w, y, k, n_classes):
    """[N, n_classes] longdouble: the summed weights of the first k slots per class"""
    scores = np.zeros((len(idx), n_classes), dtype=LD)
    rows = np.arange(len(idx))
    for s in range(k):
        np.add.at(scores, (rows, y[idx[:, s]]), w[:, s])
    return scores


def vote(idx, w, y, k, n_classes):
    """int64 [N]: arg-max by (score descending, class ascending) -- np.argmax takes the first maximum"""
    return np.argmax(class_scores(idx, w, y, k, n_classes), axis=1).astype(np.int64)


def regress(idx, w, Y, k):
    """(value float64 [N, n_out], bound float64 [N, n_out]) at k"""
    Yn = np.asarray(Y, dtype=LD)[idx[:, :k]]                             # [N, k, n_out]
    wk = w[:, :k, None]
    den = wk.sum(axis=1)
    value = (wk * Yn).sum(axis=1) / den
    bound = (2 * k + 6) * LD(U) * np.abs(wk * Yn).sum(axis=1) / den
    return value.astype(np.float64), bound.astype(np.float64)


def accuracy(pred, y, fold):
    """(per_fold [n_folds], pooled): accuracy_score per fold in ascending fold order"""
    hit = np.asarray(pred) == np.asarray(y)
    return np.asarray([hit[fold == f].mean() for f in np.unique(fold)], dtype=np.float64), float(hit.mean())


def r2(Y, pred):
    """r2_score(multioutput='uniform_average') in longdouble"""
    Y, pred = np.asarray(Y, dtype=LD).reshape(len(Y), -1), np.asarray(pred, dtype=LD).reshape(len(Y), -1)
    res = ((Y - pred) ** 2).sum(axis=0)
    tot = ((Y - Y.mean(axis=0)) ** 2).sum(axis=0)
    return float((1 - res / tot).mean())


def r2_folds(Y, pred, fold):
    return np.asarray([r2(Y[fold == f], pred[fold == f]) for f in np.unique(fold)], dtype=np.float64), r2(Y, pred)


# ---- the margins -----------------------------------------------------------------------------------------------------
def distance_margin(D2, fold, kmax, allow_equal=False):
    """the smallest relative gap between consecutive entries of any row's first kmax + 1 eligible squared distances
    (fewer when a row has only kmax); with ``allow_equal`` exactly equal entries (decided by the index) do not count"""
    worst = np.inf
    for i in range(len(D2)):
        row = np.sort(D2[i, fold != fold[i]])[:kmax + 1]
        gap, top = np.diff(row), row[1:]
        keep = top > 0
        if allow_equal:
            keep &= gap > 0
        if keep.any():
            worst = min(worst, float((gap[keep] / top[keep]).min()))
        if not allow_equal and (top == 0).any():
            return 0.0
    return worst


def score_margin(idx, d2, y, ks, n_classes):
    """the smallest relative gap between the best two class scores under 'distance' weights over all rows and all k of
    the sweep; rows whose first neighbour is at distance 0 have weights 0 / 1 and are skipped"""
    w = slot_weights(d2, True)
    rows = d2[:, 0] > 0
    worst = np.inf
    for k in ks:
        top = np.sort(class_scores(idx, w, y, k, n_classes)[rows], axis=1)[:, -2:]
        worst = min(worst, float(((top[:, 1] - top[:, 0]) / top[:, 1]).min()))
    return worst


# ---- inputs ----------------------------------------------------------------------------------------------------------
def sweep(kmax):
    """the k of the sweep: (1, 2, 5, 9, kmax) up to kmax"""
    return tuple(sorted({k for k in (1, 2, 5, 9, kmax) if k <= kmax}))


def draw(n, d, seed):
    """standard normal rows rounded to float32, 4 classes that follow the first features with 15 % of the labels
    redrawn, and 3 regression targets that are smooth in the rows plus noise"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    a, b = X[:, 0], X[:, min(1, d - 1)]
    y = (a > 0).astype(np.int64) + 2 * ((b > 0) if d > 1 else (np.abs(a) > 0.7)).astype(np.int64)
    redraw = rng.random(n) < 0.15
    y[redraw] = rng.integers(0, N_CLASSES, int(redraw.sum()))
    Y = np.stack([a + 0.1 * rng.standard_normal(n), np.sin(2.0 * b) + 0.1 * rng.standard_normal(n),
                  a * b + 3.0 + 0.1 * rng.standard_normal(n)], axis=1)
    return X, y, Y


def folds(kind, n, seed):
    rng = np.random.default_rng(seed + 7)
    if kind == "two":                                                     # 2 interleaved folds
        return np.arange(n, dtype=np.int64) % 2
    if kind == "seven":                                                   # 7 interleaved folds
        return np.arange(n, dtype=np.int64) % 7
    if kind == "runs":      # 7 folds of uneven sizes in shuffled order; sorted they end at 64, 128, 140, 150, 170, 192, n
        sizes = [64, 64, 12, 10, 20, 22, n - 192]
        return rng.permutation(np.repeat(np.arange(7, dtype=np.int64), sizes))
    if kind == "loo":
        return np.arange(n, dtype=np.int64)
    if kind == "exact":                                                   # n - largest fold == 9
        return rng.permutation(np.repeat(np.arange(2, dtype=np.int64), [n - 9, 9]))
    raise KeyError(kind)


# name -> (N, d, kmax, fold kind, first seed)
SHAPES = {
    "n64_d1_k1_two": (64, 1, 1, "two", 2401),
    "n65_d33_k9_exact": (65, 33, 9, "exact", 2402),
    "n65_d1_k9_seven": (65, 1, 9, "seven", 2403),
    "n203_d8_k9_seven": (203, 8, 9, "seven", 2404),
    "n203_d8_k9_runs": (203, 8, 9, "runs", 2405),
    "n203_d33_k64_two": (203, 33, 64, "two", 2406),
    "n203_d8_k64_runs": (203, 8, 64, "runs", 2407),
    "n203_d33_k9_loo": (203, 33, 9, "loo", 2408),
    "n64_d8_k9_loo": (64, 8, 9, "loo", 2409),
    "dup_n128_d8_k9_seven": (128, 8, 9, "seven", 2410),
}
DUPLICATE_CASE = "dup_n128_d8_k9_seven"
DUP_ROWS = (5, 77)
SKLEARN_CASES = tuple(n for n in SHAPES if n != DUPLICATE_CASE)
RUNS_CASES = ("n203_d8_k9_runs", "n203_d8_k64_runs")
EXACT_CASE = "n65_d33_k9_exact"


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: X float32 [N, d], y int64 [N], Y float64 [N, 3], fold int64 [N], kmax, ks, seed"""
    n, d, kmax, kind, seed0 = SHAPES[name]
    ks = sweep(kmax)
    for seed in range(seed0, seed0 + 50000, 1000):
        X, y, Y = draw(n, d, seed)
        fold = folds(kind, n, seed)
        dup = name == DUPLICATE_CASE
        if dup:
            X[DUP_ROWS[1]] = X[DUP_ROWS[0]]
            assert fold[DUP_ROWS[0]] != fold[DUP_ROWS[1]]
        D2 = sqdist(X)
        if distance_margin(D2, fold, kmax, allow_equal=dup) < MARGIN:
            continue
        idx, d2 = neighbours(D2, fold, kmax)
        if score_margin(idx, d2, y, ks, N_CLASSES) < MARGIN:
            continue
        for a in (X, y, Y, fold):
            a.setflags(write=False)
        return dict(X=X, y=y, Y=Y, fold=fold, kmax=kmax, ks=ks, seed=seed)
    raise AssertionError("no draw at the margin")


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement of a case: idx int64 [N, kmax], dist float64 [N, kmax] (the longdouble square roots rounded),
    and per weighting: classes int64 [n_k, N], values / bounds float64 [n_k, N, 3]; the two margins"""
    c = case(name)
    D2 = sqdist(c["X"])
    idx, d2 = neighbours(D2, c["fold"], c["kmax"])
    out = dict(idx=idx, dist=np.sqrt(d2).astype(np.float64), d2=d2,
               distance_margin=distance_margin(D2, c["fold"], c["kmax"], allow_equal=name == DUPLICATE_CASE),
               score_margin=score_margin(idx, d2, c["y"], c["ks"], N_CLASSES))
    for weighted, weights in enumerate(WEIGHTS):
        w = slot_weights(d2, weighted)
        out[weights + "_classes"] = np.stack([vote(idx, w, c["y"], k, N_CLASSES) for k in c["ks"]])
        pairs = [regress(idx, w, c["Y"], k) for k in c["ks"]]
        out[weights + "_values"] = np.stack([p[0] for p in pairs])
        out[weights + "_bounds"] = np.stack([p[1] for p in pairs])
    return out


def sorted_by_fold(name):
    """the case with its rows in ascending fold order (a stable sort): (X, y, Y, fold, perm), row j of the sorted case
    is row perm[j] of the case"""
    c = case(name)
    perm = np.argsort(c["fold"], kind='stable')
    return c["X"][perm], c["y"][perm], c["Y"][perm], c["fold"][perm], perm
