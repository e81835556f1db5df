"""The kernels of csrc/knn_predict.hip and ava_amd.knn_predict on the MI355X: the masked neighbour table against
projection's query kernel on the gathered rows of the other folds (indices and the bits of the distances), against
columns 1 .. k of ava_pj_knn under leave-one-out folds and under a row permutation; the votes and the weighted means of
a whole sweep against the restatement of tests/knnpred_cases.py and scikit-learn's recorded results
(tests/golden/knnpred.npz), at N = 64, 65, 203 (tile SQD_T = 64), d = 1, 8, 33 (stage SQD_KC = 32), kmax = 1, 9, 64, for
float32 and float64 rows, with 2 folds, 7 interleaved folds, 7 folds in runs that end on and off tile edges (the tile
skip), leave-one-out, and a case that leaves exactly kmax eligible rows; the duplicate rows, the estimators, the scores,
the refused inputs and repeat runs that must not change a bit.

Indices, distances' bits and classes compare with ``==``: the margins of knnpred_cases.py decide every comparison.
Regression values: the per-element bound of knnpred_cases.py, (2k + 6) 2^-53 sum |w Y| / sum w."""
import functools

import numpy as np
import pytest
import torch

import knnpred_cases as KC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import knn_predict as KP
from ava_amd import projection as PJ

pytestmark = pytest.mark.gpu
equal = np.testing.assert_array_equal
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def golden():
    return load_golden("knnpred.npz")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def table(name, dtype=np.float32):
    """(dist, idx) of the case at its kmax"""
    c = KC.case(name)
    return KP.masked_kneighbors(c["X"].astype(dtype), c["fold"], c["kmax"])


# ---- the masked table: the bit contract ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(KC.SHAPES))
def test_masked_table_is_the_query_kernels(name, dtype):
    """every fold's rows against the gathered rows of the other folds through ava_pj_knn_query, indices mapped back:
    the same indices and the same bits; and the restatement's indices"""
    c = KC.case(name)
    X, fold, k = c["X"].astype(dtype), c["fold"], c["kmax"]
    dist, idx = table(name, dtype)
    assert dist.dtype == np.float64 and idx.dtype == np.int64 and dist.shape == idx.shape == (len(X), k)
    for f in np.unique(fold):
        others = np.flatnonzero(fold != f)
        qi, qd = PJ.knn_query(X[fold == f], X[others], k)
        equal(idx[fold == f], others[qi])
        equal(bits(dist[fold == f]), bits(qd))
    want = KC.expected(name)
    equal(idx, want["idx"])
    err = np.abs(dist - want["dist"])
    assert np.all(err <= (X.shape[1] + 4) * KC.U * want["dist"])       # d fmas, the square root, two roundings to fp64
    assert np.all(fold[idx] != fold[:, None])
    equal(bits(dist), bits(table(name, DTYPES[1 - DTYPES.index(dtype)])[0]))   # float32 rows and their float64 copies


@pytest.mark.parametrize("name, k", [("n203_d33_k9_loo", 9), ("n64_d8_k9_loo", 9), ("n64_d8_k9_loo", 63),
                                     ("n203_d33_k9_loo", 63), ("n65_d1_k9_seven", 1)])
def test_arange_folds_are_the_knn_table(name, k):
    X = KC.case(name)["X"]
    dist, idx = KP.masked_kneighbors(X, np.arange(len(X)), k)
    ki, kd = PJ.knn(X, k + 1)
    equal(idx, ki[:, 1:])
    equal(bits(dist), bits(kd[:, 1:]))
    m = KP.KNeighborsClassifier(k).fit(X, KC.case(name)["y"])
    d2, i2 = m.kneighbors()
    equal(i2, idx)
    equal(bits(d2), bits(dist))


@pytest.mark.parametrize("name", KC.RUNS_CASES)
def test_sorted_folds_give_the_same_table(name):
    """the folds in runs (tiles inside one fold are skipped; the query tile of rows 128 .. 191 straddles five folds)
    against the same rows in shuffled order"""
    c = KC.case(name)
    Xs, _, _, fs, perm = KC.sorted_by_fold(name)
    dist, idx = table(name)
    ds, is_ = KP.masked_kneighbors(Xs, fs, c["kmax"])
    equal(perm[is_], idx[perm])
    equal(bits(ds), bits(dist[perm]))


def test_row_chunks_do_not_change_the_table(monkeypatch):
    name = "n203_d8_k9_runs"
    c = KC.case(name)
    monkeypatch.setattr(KP, "_KNN_CHUNK", 64)
    dist, idx = KP.masked_kneighbors(c["X"], c["fold"], c["kmax"])
    equal(idx, table(name)[1])
    equal(bits(dist), bits(table(name)[0]))
    Xs, _, _, fs, perm = KC.sorted_by_fold(name)                          # a chunk that is one skipped tile's queries
    ds, is_ = KP.masked_kneighbors(Xs, fs, c["kmax"])
    equal(perm[is_], table(name)[1][perm])


# ---- classification --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(KC.SHAPES))
def test_classes_of_a_sweep(golden, name, dtype):
    c, want = KC.case(name), KC.expected(name)
    X = c["X"].astype(dtype)
    for w in KC.WEIGHTS:
        got = KP.cross_val_predict(X, c["y"], c["fold"], n_neighbors=list(c["ks"]), weights=w)
        assert got.dtype == c["y"].dtype and got.shape == (len(c["ks"]), len(X))
        equal(got, want[w + "_classes"])
        if name in KC.SKLEARN_CASES:
            equal(got, golden["%s_%s_classes" % (name, w)])
        for a, k in enumerate(c["ks"]):                                   # single-k calls drop the axis
            equal(KP.cross_val_predict(X, c["y"], c["fold"], n_neighbors=k, weights=w), got[a])
        equal(KP.cross_val_predict(X, c["y"], c["fold"], n_neighbors=list(c["ks"]), weights=w), got)   # a second run


def test_classes_are_the_callers_labels():
    """strings, a tensor, and as many classes as rows (no cap): with k = 1 the class of the nearest row"""
    c, want = KC.case("n203_d8_k9_seven"), KC.expected("n203_d8_k9_seven")
    names = np.asarray(["wt", "het", "ko", "mut"])                         # sorted: het, ko, mut, wt
    rank = np.argsort(np.argsort(names))
    got = KP.cross_val_predict(c["X"], names[c["y"]], c["fold"], n_neighbors=[2, 9])
    assert got.dtype.kind == "U"
    # the tie rule follows the sorted classes: restate with the ranks as codes
    w = KC.slot_weights(want["d2"], 0)
    for a, k in enumerate((2, 9)):
        equal(got[a], np.sort(names)[KC.vote(want["idx"], w, rank[c["y"]], k, 4)])
    got = KP.cross_val_predict(c["X"], torch.from_numpy(c["y"]), torch.from_numpy(c["fold"]), n_neighbors=9,
                               weights='distance')
    equal(got, want["distance_classes"][-1])
    own = 1000 * np.arange(len(c["X"]))[::-1].copy()
    for w in KC.WEIGHTS:
        got = KP.cross_val_predict(c["X"], own, c["fold"], n_neighbors=[1, 9], weights=w)
        equal(got[0], own[want["idx"][:, 0]])
    equal(got[1], own[want["idx"][:, 0]])      # distance weights, all classes different: the nearest row's
    got = KP.cross_val_predict(c["X"], own, c["fold"], n_neighbors=9)     # uniform, all scores 1: the smallest class
    equal(got, own[want["idx"]].min(axis=1))


@pytest.mark.parametrize("weights", KC.WEIGHTS)
def test_classifier(weights):
    """fit on the other folds and predict a fold: the rows of cross_val_predict; predict_proba sums to 1 and its
    arg-max is predict; without rows the leave-one-out predictions"""
    name = "n203_d8_k9_seven"
    c, want = KC.case(name), KC.expected(name)
    X, y, fold = c["X"], c["y"], c["fold"]
    for a, k in enumerate(c["ks"]):
        for f in (0, 6):
            m = KP.KNeighborsClassifier(k, weights=weights).fit(X[fold != f], y[fold != f])
            equal(m.classes_, np.arange(4))
            pred = m.predict(X[fold == f])
            equal(pred, want[weights + "_classes"][a][fold == f])
            proba = m.predict_proba(X[fold == f])
            assert proba.shape == (int((fold == f).sum()), 4) and proba.dtype == np.float64
            # the scores partition the k weights (k adds), C divisions, C adds
            assert np.all(np.abs(proba.sum(axis=1) - 1.0) <= (k + 2 * 4) * KC.U)
            equal(np.argmax(proba, axis=1), pred)
            assert m.score(X[fold == f], y[fold == f]) == float(np.mean(pred == y[fold == f]))
            others = np.flatnonzero(fold != f)
            dist, idx = m.kneighbors(X[fold == f])
            equal(others[idx], want["idx"][fold == f][:, :k])
    if weights == 'uniform':
        counts = np.stack([(y[want["idx"][fold == 6][:, :9]] == cl).sum(axis=1) for cl in range(4)], axis=1)
        equal(proba, counts / 9.0)
    loo_name = "n64_d8_k9_loo"
    c, want = KC.case(loo_name), KC.expected(loo_name)
    m = KP.KNeighborsClassifier(5, weights=weights).fit(c["X"].astype(np.float64), c["y"])
    equal(m.predict(), want[weights + "_classes"][c["ks"].index(5)])
    equal(np.argmax(m.predict_proba(), axis=1), m.predict())


# ---- regression ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(KC.SHAPES))
def test_values_of_a_sweep(golden, name, dtype):
    c, want = KC.case(name), KC.expected(name)
    X = c["X"].astype(dtype)
    for w in KC.WEIGHTS:
        got = KP.cross_val_predict(X, c["Y"], c["fold"], n_neighbors=list(c["ks"]), weights=w, task='regress')
        assert got.dtype == np.float64 and got.shape == (len(c["ks"]), len(X), KC.N_OUT)
        err, bound = np.abs(got - want[w + "_values"]), want[w + "_bounds"]
        for a, k in enumerate(c["ks"]):
            print("%s %s k=%d: max |device - restatement| / bound %.3f"
                  % (name, w, k, float((err[a] / bound[a]).max())))
        assert np.all(err <= bound)
        if name in KC.SKLEARN_CASES:                                      # sklearn is within the bound of the restatement
            assert np.all(np.abs(got - golden["%s_%s_values" % (name, w)]) <= 2 * bound)
        for a, k in enumerate(c["ks"]):
            one = KP.cross_val_predict(X, c["Y"], c["fold"], n_neighbors=k, weights=w, task='regress')
            equal(bits(one), bits(got[a]))
        flat = KP.cross_val_predict(X, c["Y"][:, 1], c["fold"], n_neighbors=list(c["ks"]), weights=w, task='regress')
        equal(bits(flat), bits(got[:, :, 1]))
        again = KP.cross_val_predict(X, c["Y"], c["fold"], n_neighbors=list(c["ks"]), weights=w, task='regress')
        equal(bits(again), bits(got))


@pytest.mark.parametrize("weights", KC.WEIGHTS)
def test_regressor(weights):
    name = "n203_d8_k9_runs"
    c, want = KC.case(name), KC.expected(name)
    X, Y, fold = c["X"], c["Y"], c["fold"]
    cv = KP.cross_val_predict(X, Y, fold, n_neighbors=list(c["ks"]), weights=weights, task='regress')
    for a, k in enumerate(c["ks"]):
        for f in (0, 3):
            m = KP.KNeighborsRegressor(k, weights=weights).fit(X[fold != f], Y[fold != f])
            pred = m.predict(X[fold == f])
            equal(bits(pred), bits(cv[a][fold == f]))
            assert abs(m.score(X[fold == f], Y[fold == f]) - KC.r2(Y[fold == f], pred)) <= 1e-12
            flat = KP.KNeighborsRegressor(k, weights=weights).fit(X[fold != f], Y[fold != f][:, 2])
            equal(bits(flat.predict(X[fold == f])), bits(pred[:, 2]))
    loo_name = "n64_d8_k9_loo"
    c, want = KC.case(loo_name), KC.expected(loo_name)
    a = c["ks"].index(5)
    pred = KP.KNeighborsRegressor(5, weights=weights).fit(c["X"], c["Y"]).predict()
    assert np.all(np.abs(pred - want[weights + "_values"][a]) <= want[weights + "_bounds"][a])


# ---- the duplicate rows ----------------------------------------------------------------------------------------------
def test_duplicate_rows():
    """rows 5 and 77 are equal, in different folds: each is the other's first neighbour at distance exactly 0, under
    'distance' weights it alone decides their predictions, and every third row lists 5 before 77"""
    c, want = KC.case(KC.DUPLICATE_CASE), KC.expected(KC.DUPLICATE_CASE)
    i, j = KC.DUP_ROWS
    dist, idx = table(KC.DUPLICATE_CASE)
    equal(idx, want["idx"])
    assert idx[i, 0] == j and idx[j, 0] == i and dist[i, 0] == 0.0 and dist[j, 0] == 0.0
    assert np.all(dist[:, 1:] > 0.0)
    cls = KP.cross_val_predict(c["X"], c["y"], c["fold"], n_neighbors=list(c["ks"]), weights='distance')
    val = KP.cross_val_predict(c["X"], c["Y"], c["fold"], n_neighbors=list(c["ks"]), weights='distance', task='regress')
    for a in range(len(c["ks"])):
        assert cls[a, i] == c["y"][j] and cls[a, j] == c["y"][i]
        equal(val[a, i], c["Y"][j])
        equal(val[a, j], c["Y"][i])
    m = KP.KNeighborsClassifier(9, weights='distance').fit(c["X"], c["y"])
    proba = m.predict_proba(c["X"][[i]])                                   # both copies at distance 0: weights 1, 1, 0, ..
    want_p = np.zeros(4)
    want_p[c["y"][i]] += 0.5
    want_p[c["y"][j]] += 0.5
    equal(proba[0], want_p)


# ---- the scores ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n203_d8_k9_seven", "n203_d8_k9_runs", "n203_d33_k64_two", "n65_d33_k9_exact"])
def test_scores(golden, name):
    c, want = KC.case(name), KC.expected(name)
    n_k = len(c["ks"])
    for w in KC.WEIGHTS:
        r = KP.cross_val_score(c["X"], c["y"], c["fold"], n_neighbors=list(c["ks"]), weights=w, confusion=True)
        equal(r["n_neighbors"], c["ks"])
        equal(r["classes"], np.arange(4))
        per = np.stack([KC.accuracy(want[w + "_classes"][a], c["y"], c["fold"])[0] for a in range(n_k)], axis=1)
        equal(r["per_fold"], per)
        equal(r["per_fold"], golden["%s_%s_accuracy" % (name, w)])
        equal(r["pooled"], [KC.accuracy(want[w + "_classes"][a], c["y"], c["fold"])[1] for a in range(n_k)])
        assert r["confusion"].dtype == np.int64 and r["confusion"].shape == (n_k, 4, 4)
        for a in range(n_k):
            conf = np.zeros((4, 4), dtype=np.int64)
            np.add.at(conf, (c["y"], want[w + "_classes"][a]), 1)
            equal(r["confusion"][a], conf)
        r = KP.cross_val_score(c["X"], c["Y"], c["fold"], n_neighbors=list(c["ks"]), weights=w, task='regress')
        # R^2 = 1 - res / tot of sums of at most 203 squares: within 1e-12 of the longdouble restatement
        for a in range(n_k):
            per, pooled = KC.r2_folds(c["Y"], want[w + "_values"][a], c["fold"])
            assert np.all(np.abs(r["per_fold"][:, a] - per) <= 1e-12) and abs(r["pooled"][a] - pooled) <= 1e-12
        assert np.all(np.abs(r["per_fold"] - golden["%s_%s_r2" % (name, w)]) <= 1e-12)
    one = KP.cross_val_score(c["X"], c["y"], c["fold"], n_neighbors=c["ks"][-1])
    assert one["per_fold"].shape == (len(np.unique(c["fold"])), 1) and "confusion" not in one


# ---- refused inputs, input forms -------------------------------------------------------------------------------------
def test_refused_inputs():
    c = KC.case(KC.EXACT_CASE)
    X, y, fold = c["X"], c["y"], c["fold"]
    equal(KP.cross_val_predict(X, y, fold, n_neighbors=9), KC.expected(KC.EXACT_CASE)["uniform_classes"][-1])
    with pytest.raises(ValueError, match="too few eligible rows"):
        KP.cross_val_predict(X, y, fold, n_neighbors=10)
    with pytest.raises(ValueError, match="too few eligible rows"):
        KP.masked_kneighbors(torch.from_numpy(X).cuda(), fold, 10)
    bad = X.copy()
    bad[3, 1] = np.nan
    for rows in (bad, torch.from_numpy(bad).cuda()):
        with pytest.raises(ValueError, match="Input X contains NaN."):
            KP.cross_val_predict(rows, y, fold)
        with pytest.raises(ValueError, match="Input X contains NaN."):
            KP.masked_kneighbors(rows, fold, 2)
    with pytest.raises(ValueError, match="at most 16"):
        KP.cross_val_predict(X, y, KC.case("n203_d8_k9_seven")["fold"][:65], n_neighbors=list(range(1, 18)))
    for ks in ([2, 1], [1, 5, 5]):
        with pytest.raises(ValueError, match="strictly ascending"):
            KP.cross_val_predict(X, y, fold, n_neighbors=ks)
    with pytest.raises(ValueError, match="features"):
        KP.KNeighborsClassifier(5).fit(X, y).predict(X[:, :5])
    small = KP.KNeighborsClassifier(9).fit(X[:8], y[:8])
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        small.predict(X)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        small.kneighbors(n_neighbors=8)                                   # without rows a row is not its own neighbour
    # the library refuses an unsorted or over-long sweep itself
    lib = _lib.load()
    idx = torch.zeros((4, 9), dtype=torch.int64, device="cuda")
    dist = torch.ones((4, 9), dtype=torch.float64, device="cuda")
    yd = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros((17, 4), dtype=torch.int32, device="cuda")
    for ks in ([2, 1], [1, 1], [0, 1], [1, 10], list(range(1, 18))):
        ks = np.asarray(ks, dtype=np.int32)
        assert lib.ava_kp_vote(idx.data_ptr(), dist.data_ptr(), 4, 9, yd.data_ptr(), ks.ctypes.data, len(ks), 0,
                               out.data_ptr(), _lib.stream()) == -1


def test_input_forms_give_the_same_bits():
    name = "n203_d8_k9_runs"
    c = KC.case(name)
    X, fold = c["X"], c["fold"]
    dist, idx = table(name)
    for rows in (torch.from_numpy(X), torch.from_numpy(X).cuda(), torch.from_numpy(X.astype(np.float64)).cuda(), X):
        for fl in (fold.astype(np.int32), fold.astype(np.uint8), torch.from_numpy(fold), 10 * fold - 30):
            d2, i2 = KP.masked_kneighbors(rows, fl, c["kmax"])
            equal(i2, idx)
            equal(bits(d2), bits(dist))
