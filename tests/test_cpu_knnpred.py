"""ava_amd.knn_predict without a GPU: the restatement of tests/knnpred_cases.py against scikit-learn's own
cross_val_predict / cross_val_score over KNeighborsClassifier / KNeighborsRegressor (algorithm='brute',
cv=PredefinedSplit(fold)) under both weightings, the margins of every case, the content of tests/golden/knnpred.npz,
kfold against KFold, the argument checks that need no device and the C ABI's mirror and refusals.

Classes compare with ``==`` (the margins of knnpred_cases.py decide every comparison); regression values within the
per-element bound of knnpred_cases.py."""

import numpy as np
import pytest
import torch

import knnpred_cases as KC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import knn_predict as KP

equal = np.testing.assert_array_equal


@pytest.fixture(scope="module")
def golden():
    return load_golden("knnpred.npz")


# ---- the restatement, the margins, the golden file -------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.SKLEARN_CASES)
def test_restatement_is_sklearns(golden, name):
    from sklearn.model_selection import PredefinedSplit, cross_val_predict
    from sklearn.neighbors import KNeighborsClassifier, KNeighborsRegressor
    c, want = KC.case(name), KC.expected(name)
    X = c["X"].astype(np.float64)
    cv = PredefinedSplit(c["fold"])
    for w in KC.WEIGHTS:
        for a, k in enumerate(c["ks"]):
            got = cross_val_predict(KNeighborsClassifier(k, weights=w, algorithm='brute'), X, c["y"], cv=cv)
            equal(want[w + "_classes"][a], got, err_msg="%s k=%d" % (w, k))
            equal(golden["%s_%s_classes" % (name, w)][a], got)
            val = cross_val_predict(KNeighborsRegressor(k, weights=w, algorithm='brute'), X, c["Y"], cv=cv)
            err, bound = np.abs(val - want[w + "_values"][a]), want[w + "_bounds"][a]
            print("%s %s k=%d: max |sklearn - restatement| / bound %.3f" % (name, w, k, float((err / bound).max())))
            assert np.all(err <= bound)
            equal(golden["%s_%s_values" % (name, w)][a], val)


@pytest.mark.parametrize("name", KC.SKLEARN_CASES)
def test_per_fold_scores_are_sklearns(golden, name):
    """accuracy and R^2 per fold of the restatement's predictions == sklearn's cross_val_score, and the golden file"""
    from sklearn.model_selection import PredefinedSplit, cross_val_score
    from sklearn.neighbors import KNeighborsClassifier, KNeighborsRegressor
    c, want = KC.case(name), KC.expected(name)
    X = c["X"].astype(np.float64)
    cv = PredefinedSplit(c["fold"])
    loo = len(np.unique(c["fold"])) == len(X)
    for w in KC.WEIGHTS:
        for a, k in enumerate(c["ks"]):
            sk = cross_val_score(KNeighborsClassifier(k, weights=w, algorithm='brute'), X, c["y"], cv=cv)
            equal(KC.accuracy(want[w + "_classes"][a], c["y"], c["fold"])[0], sk)
            equal(golden["%s_%s_accuracy" % (name, w)][:, a], sk)
            if loo:
                assert "%s_%s_r2" % (name, w) not in golden
                continue
            sk = cross_val_score(KNeighborsRegressor(k, weights=w, algorithm='brute'), X, c["Y"], cv=cv)
            # R^2 = 1 - res / tot of sums of at most 203 squares: longdouble and fp64 agree far inside 1e-12
            mine = KC.r2_folds(c["Y"], want[w + "_values"][a], c["fold"])[0]
            np.testing.assert_allclose(mine, sk, rtol=0, atol=1e-12)
            equal(golden["%s_%s_r2" % (name, w)][:, a], sk)


def test_golden_holds_the_cases_and_nothing_else(golden):
    keys = ["%s_%s_%s" % (n, w, q) for n in KC.SKLEARN_CASES for w in KC.WEIGHTS
            for q in ("classes", "values", "accuracy") + (() if n.endswith("loo") else ("r2",))]
    assert sorted(golden) == sorted(keys)


def test_margins_and_cases():
    for name in KC.SHAPES:
        c, e = KC.case(name), KC.expected(name)
        print("%-22s seed %5d distance margin %.2e score margin %.2e" % (name, c["seed"], e["distance_margin"],
                                                                       e["score_margin"]))
        assert e["distance_margin"] >= KC.MARGIN and e["score_margin"] >= KC.MARGIN
        n, d, kmax, _, _ = KC.SHAPES[name]
        assert c["X"].shape == (n, d) and c["X"].dtype == np.float32 and c["ks"][-1] == kmax == c["kmax"]
        assert len(np.unique(c["y"])) == KC.N_CLASSES and c["Y"].shape == (n, KC.N_OUT)
        assert n - np.bincount(c["fold"]).max() >= kmax
        # no row's list holds a row of its own fold, and every list is full
        assert np.all(c["fold"][e["idx"]] != c["fold"][:, None])
        if name != KC.DUPLICATE_CASE:
            assert len(np.unique(c["X"], axis=0)) == n
    c = KC.case(KC.EXACT_CASE)
    assert len(c["X"]) - np.bincount(c["fold"]).max() == c["kmax"]
    # uniform weights meet exact ties between classes, which the class rule decides
    c, e = KC.case("n203_d8_k9_seven"), KC.expected("n203_d8_k9_seven")
    scores = KC.class_scores(e["idx"], KC.slot_weights(e["d2"], 0), c["y"], 2, KC.N_CLASSES)
    top = np.sort(scores, axis=1)
    assert (top[:, -1] == top[:, -2]).sum() > 10
    # the runs cases: sorted, the folds end at 64, 128 (tile edges) and 140, 150, 170, 192 (inside a tile)
    for name in KC.RUNS_CASES:
        fold = KC.sorted_by_fold(name)[3]
        equal(np.flatnonzero(np.diff(fold)) + 1, [64, 128, 140, 150, 170, 192])
    # the duplicate case: equal rows in different folds, each the other's first neighbour at distance 0
    c, e = KC.case(KC.DUPLICATE_CASE), KC.expected(KC.DUPLICATE_CASE)
    i, j = KC.DUP_ROWS
    equal(c["X"][i], c["X"][j])
    assert c["fold"][i] != c["fold"][j]
    assert e["idx"][i, 0] == j and e["idx"][j, 0] == i and e["dist"][i, 0] == 0.0 == e["dist"][j, 0]
    both = [(r, list(e["idx"][r])) for r in range(len(c["X"])) if i in e["idx"][r] and j in e["idx"][r]]
    assert len(both) > 0                                                  # third rows that see the pair: index order
    for r, row in both:
        assert row.index(i) + 1 == row.index(j) and e["d2"][r, row.index(i)] == e["d2"][r, row.index(j)]


def test_kfold_is_sklearns():
    from sklearn.model_selection import KFold
    for n, s in ((10, 2), (10, 3), (203, 5), (203, 7), (64, 64), (65, 64), (7, 7)):
        want = np.empty(n, dtype=np.int64)
        for f, (_, test) in enumerate(KFold(s).split(np.zeros((n, 1)))):
            want[test] = f
        got = KP.kfold(n, s)
        assert got.dtype == np.int64
        equal(got, want)
    for bad in (1, 0, -2, 2.0, True, None):
        with pytest.raises(ValueError, match="n_splits"):
            KP.kfold(10, bad)
    with pytest.raises(ValueError, match="greater than the number of samples"):
        KP.kfold(3, 4)


def test_group_folds():
    from sklearn.model_selection import LeaveOneGroupOut
    groups = np.asarray(["b", "a", "c", "a", "b", "b"])
    fold = KP.group_folds(groups)
    equal(fold, [1, 0, 2, 0, 1, 1])
    assert fold.dtype == np.int64
    tests = [t for _, t in LeaveOneGroupOut().split(np.zeros((6, 1)), groups=groups)]
    for f, t in enumerate(tests):
        equal(np.flatnonzero(fold == f), t)
    equal(KP.group_folds(torch.tensor([7, 3, 7])), [1, 0, 1])
    with pytest.raises(ValueError, match="fewer than 2 unique groups"):
        KP.group_folds([1, 1, 1])
    with pytest.raises(ValueError, match="integers or strings"):
        KP.group_folds([0.5, 1.5])


# ---- argument checks that need no device -----------------------------------------------------------------------------
def test_checks_run_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(KP, "_device", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    c = KC.case("n65_d33_k9_exact")
    X, y, Y, fold = c["X"], c["y"], c["Y"], c["fold"]
    holes = np.arange(X.size).reshape(X.shape) == 7

    def every(exc, match, **kw):
        args = dict(X=X, y=y, fold=fold, n_neighbors=5, weights='uniform', task='classify')
        args.update(kw)
        Xa, ya, fa = args.pop("X"), args.pop("y"), args.pop("fold")
        for fn in (KP.cross_val_predict, KP.cross_val_score):
            with pytest.raises(exc, match=match):
                fn(Xa, ya, fa, **args)

    for weights in ("Uniform", "inverse", None, 3):
        every(ValueError, "'weights' parameter", weights=weights)
        with pytest.raises(ValueError, match="'weights' parameter"):
            KP.KNeighborsClassifier(weights=weights).fit(X, y)
    every(NotImplementedError, "callable", weights=lambda d: 1.0 / d)
    with pytest.raises(NotImplementedError, match="callable"):
        KP.KNeighborsRegressor(weights=np.reciprocal).fit(X, Y)
    for kw in (dict(metric="cosine"), dict(metric="manhattan"), dict(metric="minkowski", p=1), dict(p=3),
               dict(algorithm="kd_tree"), dict(algorithm="ball_tree"), dict(radius=1.0)):
        with pytest.raises(NotImplementedError):
            KP.KNeighborsClassifier(**kw).fit(X, y)
        with pytest.raises(NotImplementedError):
            KP.KNeighborsRegressor(**kw).fit(X, Y)
    every(ValueError, "task must be", task="cluster")
    for bad in (0, -1, [0, 1], 65, [5, 65]):
        every(ValueError, "n_neighbors", n_neighbors=bad)
    for bad in (2.0, True, "5", None, [1, 2.5], [], ()):
        every(ValueError, "n_neighbors", n_neighbors=bad)
    every(ValueError, "at most 16", n_neighbors=list(range(1, 18)))
    for bad in ([2, 1], [1, 5, 5], [1, 3, 2, 9]):
        every(ValueError, "strictly ascending", n_neighbors=bad)
    every(ValueError, "too few eligible rows", n_neighbors=10)           # N - largest fold == 9
    every(ValueError, "too few eligible rows", n_neighbors=[1, 9, 10])
    every(ValueError, "at least 2 folds", fold=np.zeros(len(X), dtype=np.int64))
    every(ValueError, "fold must be integers", fold=fold.astype(np.float64))
    every(ValueError, "inconsistent numbers of samples", fold=fold[:-1])
    every(ValueError, "inconsistent numbers of samples", y=y[:-1])
    every(ValueError, "Unknown label type", y=Y[:, 0])
    every(ValueError, "1d array", y=Y[:, :2].astype(np.int64))
    every(ValueError, "NaN or infinity", y=np.where(np.arange(len(Y)) == 3, np.nan, Y[:, 0]), task='regress')
    every(ValueError, "between 1 and 256", y=np.zeros((len(X), 257)), task='regress')
    for bad, message in ((X[:, 0], "Expected 2D array"), (np.where(holes, np.nan, X), "Input X contains NaN."),
                         (np.where(holes, np.inf, X), "Input X contains infinity"),
                         (torch.from_numpy(np.where(holes, np.nan, X)), "Input X contains NaN.")):
        every(ValueError, message, X=bad)
        with pytest.raises(ValueError, match=message):
            KP.masked_kneighbors(bad, fold, 3)
        with pytest.raises(ValueError, match=message):
            KP.KNeighborsClassifier().fit(bad, y)
    for k in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            KP.masked_kneighbors(X, fold, k)
    with pytest.raises(ValueError, match="too few eligible rows"):
        KP.masked_kneighbors(X, fold, 10)
    with pytest.raises(ValueError, match="confusion=True"):
        KP.cross_val_score(X, Y, fold, task='regress', confusion=True)
    with pytest.raises(ValueError, match="one int"):
        KP.KNeighborsClassifier([1, 2]).fit(X, y)
    with pytest.raises(ValueError, match="not fitted"):
        KP.KNeighborsClassifier().predict(X)


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    c = KC.case("n65_d33_k9_exact")
    with pytest.raises(_lib.AvaHipError):
        KP.masked_kneighbors(c["X"], c["fold"], 3)
    with pytest.raises(_lib.AvaHipError):
        KP.cross_val_predict(c["X"], c["y"], c["fold"])
    with pytest.raises(_lib.AvaHipError):
        KP.cross_val_score(c["X"], c["Y"], c["fold"], task='regress')
    with pytest.raises(_lib.AvaHipError):
        KP.KNeighborsClassifier().fit(c["X"], c["y"])
    with pytest.raises(_lib.AvaHipError):
        KP.KNeighborsRegressor().fit(c["X"], c["Y"])


def test_constructors_keep_their_parameters():
    m = KP.KNeighborsClassifier()
    assert (m.n_neighbors, m.weights, m.algorithm, m.p) == (5, 'uniform', 'auto', 2)
    assert (m.metric, m.radius) == ('euclidean', None)
    m = KP.KNeighborsRegressor(7, weights='distance')
    assert (m.n_neighbors, m.weights) == (7, 'distance')
    with pytest.raises(TypeError):
        KP.KNeighborsClassifier(5, 'distance')                            # keyword-only, as sklearn's


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_library_argument_checks():
    """ava_kp_* return their limits / AVA_EINVAL before any HIP call (the test runs without a device, where a HIP call
    would return AVA_ELAUNCH instead)"""
    lib = _lib.load()
    assert lib.ava_kp_max_sweep() == KP.MAX_SWEEP == 16
    assert lib.ava_kp_max_classes() == KP.MAX_CLASSES == 4096
    assert lib.ava_kp_max_outputs() == KP.MAX_OUTPUTS == 256
    buf = np.zeros(256, dtype=np.float64)
    p = buf.ctypes.data

    def sweep(*ks):
        return np.asarray(ks, dtype=np.int32)

    def refuses(fn, ok, bad_args):
        for i, bad in bad_args:
            a = list(ok)
            a[i] = bad.ctypes.data if isinstance(bad, np.ndarray) else bad
            assert fn(*a, None) == -1, (fn.__name__, i, bad)

    # x, dtype, n, d, k, fold, q0, nq, out_idx, out_dist
    refuses(lib.ava_kp_knn_masked, [p, 1, 8, 2, 3, p, 0, 8, p, p],
            ((0, None), (1, 2), (1, -1), (2, 0), (2, 2 ** 30 + 1), (3, 0), (3, 65537), (4, 0), (4, 65), (4, 9), (5, None),
             (6, -1), (7, 0), (7, 9), (8, None), (9, None)))
    refuses(lib.ava_kp_knn_masked, [p, 1, 8, 2, 3, p, 4, 4, p, p], ((7, 5),))
    good = sweep(1, 2, 5)
    bad_sweeps = [(5, sweep(0, 1, 2)), (5, sweep(1, 2, 10)), (5, sweep(2, 1, 5)), (5, sweep(1, 2, 2)), (5, None)]
    # idx, dist, nq, kmax, y, ks, n_k, weighted, out
    refuses(lib.ava_kp_vote, [p, p, 4, 9, p, good.ctypes.data, 3, 0, p],
            [(0, None), (1, None), (2, 0), (3, 0), (3, 65), (3, 4), (4, None), (6, 0), (7, 2), (7, -1), (8, None)]
            + bad_sweeps)
    long = sweep(*range(1, 18))
    assert lib.ava_kp_vote(p, p, 4, 64, p, long.ctypes.data, 17, 0, p, None) == -1
    # idx, dist, nq, k, y, n_classes, weighted, out
    refuses(lib.ava_kp_proba, [p, p, 4, 9, p, 4, 0, p],
            ((0, None), (1, None), (2, 0), (3, 0), (3, 65), (4, None), (5, 0), (5, 4097), (6, 2), (7, None)))
    # idx, dist, nq, kmax, Y, n_out, ks, n_k, weighted, out
    refuses(lib.ava_kp_regress, [p, p, 4, 9, p, 3, good.ctypes.data, 3, 1, p],
            [(0, None), (1, None), (2, 0), (3, 0), (3, 65), (4, None), (5, 0), (5, 257), (7, 0), (8, 2), (9, None)]
            + [(6, s) for _, s in bad_sweeps])
    assert lib.ava_kp_regress(p, p, 4, 64, p, 3, long.ctypes.data, 17, 0, p, None) == -1
