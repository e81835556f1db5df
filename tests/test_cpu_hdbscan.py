"""ava_amd.hdbscan without a GPU: the restatement of tests/hdbscan_cases.py against scikit-learn's own HDBSCAN and
tests/golden/hdbscan.npz, the exactness of every case's sums, the spanning tree's weights against scipy's, the cases
that do not depend on the row order, the host tree tail ``ava_hd_tree`` against the restatement, the argument checks
that need no device and the C ABI's mirror and refusals.

Labels, edges and linkage matrices compare with ``==``: the inputs are exact (hdbscan_cases.py), so every key comparison
is decided.  Probabilities are one square root, one reciprocal and one division away from exact keys: 4 * 2^-53."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dbscan_cases as DC
import hdbscan_cases as HC
from conftest import ROOT, load_golden
from ava_amd import _lib
from ava_amd import hdbscan as HD
from ava_amd import projection as PJ

equal = np.testing.assert_array_equal
PROB_RTOL = 4 * HC.U


@pytest.fixture(scope="module")
def golden():
    return load_golden("hdbscan.npz")


# ---- the restatement, sklearn, the golden file -------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.BLOB_CASES)
def test_restatement_is_sklearns_on_blob_cases(golden, name):
    """the generator condition at the case's seed (and at no earlier one), sklearn's results as the golden file holds
    them, and the probabilities within 8 x the error measured when the file was written"""
    assert HC.find_seed(name) == HC.SEEDS[name] == int(golden[name + "_seed"])
    X, mcs, ms, method = HC.case(name)
    want = HC.expected(name)
    assert want["n_clusters"] >= 2 and want["n_noise"] > 0 and want["stability_gap"] >= HC.GAP
    assert float(golden[name + "_stability_gap"]) == want["stability_gap"]
    prob_err = float(golden[name + "_prob_err"])
    mine = DC.by_smallest_member(want["labels"])
    for algorithm in HC.SKLEARN_ALGORITHMS:
        sk = HC.sklearn_fit(X, mcs, ms, algorithm, method)
        equal(DC.by_smallest_member(sk.labels_), mine, err_msg=algorithm)
        if algorithm == "brute":
            equal(golden[name + "_labels"], sk.labels_)
            err = float(np.abs(want["probabilities"] - sk.probabilities_).max())
            print("%s: max |restatement - sklearn| over probabilities_ %.2e, prob_err %.2e" % (name, err, prob_err))
            assert err <= 8 * prob_err
    assert float(np.abs(want["probabilities"] - golden[name + "_probabilities"]).max()) <= 8 * prob_err
    assert golden[name + "_labels"].dtype == np.int64 and golden[name + "_probabilities"].dtype == np.float64


@pytest.mark.parametrize("name", ["leaf_n257_d32", "leaf_n129_d1", "ms64_n257_d32"])
def test_restatement_is_sklearns_on_the_variants(name):
    X, mcs, ms, method = HC.case(name)
    sk = HC.sklearn_fit(X, mcs, ms, "brute", method)
    equal(DC.by_smallest_member(sk.labels_), DC.by_smallest_member(HC.expected(name)["labels"]))


def test_golden_holds_the_blob_cases_and_nothing_else(golden):
    fields = ("labels", "probabilities", "seed", "stability_gap", "prob_err")
    assert sorted(golden) == sorted("%s_%s" % (n, q) for n in HC.BLOB_CASES for q in fields)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "hdbscan.npz")) < 64 * 1024


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_sums_are_exact(name):
    """float32 rows on the 2^-12 grid: the longdouble, float64 and reversed-order float64 sums are the same numbers"""
    X = HC.case(name)[0]
    assert X.dtype == np.float32
    g = X.astype(np.float64) * HC.GRID
    assert np.all(g == np.round(g))
    span = float((g.max(axis=0) - g.min(axis=0)).max())
    assert X.shape[1] * span * span < 2.0 ** 53                          # every sum of squares fits the significand
    a, b = HC.measures(X), HC.measures(X, reverse=True)
    equal(a, b)
    equal(a.astype(np.longdouble), HC.measures(X, dtype=np.longdouble))
    equal(a, a.T)


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_tree_weights_are_scipys(name):
    """every minimum spanning tree of a graph has the same sorted list of weights"""
    from scipy.sparse.csgraph import minimum_spanning_tree
    X, mcs, ms, _ = HC.case(name)
    want = HC.expected(name)
    M = HC.measures(X)
    core = HC.core_measures(M, mcs if ms is None else ms)
    equal(core, want["core"])
    W = np.maximum(np.maximum(core[:, None], core[None, :]), M)
    tiny = 0.5 * float(W[W > 0.0].min())                                  # scipy reads a dense 0 as "no edge"
    W = np.where(W == 0.0, tiny, W)
    np.fill_diagonal(W, 0.0)
    got = np.sort(minimum_spanning_tree(W).data)
    equal(np.where(got == tiny, 0.0, got), np.sort(want["weights"]))
    I, J = want["edges"]
    assert np.all(I < J) and len(I) == len(X) - 1
    keys = list(zip(want["weights"].tolist(), want["raw"].tolist(), I.tolist(), J.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    equal(want["mst"][:, 2], np.sqrt(want["weights"]))


def test_cases_exercise_what_they_are_for():
    assert np.all(HC.expected("n2")["labels"] == -1) and HC.expected("n2")["n_clusters"] == 0
    for order in ("asc", "desc", "shuf"):
        r = HC.expected("chain_" + order)
        assert len(r["labels"]) == 600 and r["n_clusters"] >= 2
    # the lattice: most edges tie with another in (w, m)
    r = HC.expected("lattice")
    pairs = np.stack([r["weights"], r["raw"]], axis=1)
    assert len(np.unique(pairs, axis=0)) < len(pairs) // 4
    # duplicates: merges at distance exactly 0, so lambda = inf, and those rows are certain members
    r = HC.expected("duplicates")
    assert (r["mst"][:, 2] == 0.0).sum() == 5
    assert len(set(r["labels"][5:9])) == 1 and r["labels"][5] >= 0 and np.all(r["probabilities"][5:9] == 1.0)
    # the hub: its two edges tie in (w, m) and the rows decide; it joins the group of row 0
    X, mcs, ms, _ = HC.case("hub")
    r = HC.expected("hub")
    assert r["core"][HC.HUB] == 16.0 and np.all(np.delete(r["core"], HC.HUB) <= 1.0)
    at = [(int(i), int(j), w, m) for i, j, w, m in zip(*r["edges"], r["weights"], r["raw"]) if HC.HUB in (i, j)]
    assert at == [(4, 5, 16.0, 16.0), (5, 6, 16.0, 16.0)]
    equal(r["labels"], [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1])
    assert r["probabilities"][HC.HUB] < 1.0
    # the rows in reverse order: the hub's edge to the other group comes first, and it goes there
    rev = HC.restate(X[::-1].copy(), mcs, ms)
    equal(rev["labels"], [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1])
    assert rev["labels"][len(X) - 1 - HC.HUB] != rev["labels"][len(X) - 1 - 4]
    # 'leaf' selects the leaves of the cluster tree; min_samples = 64 leaves nothing to select
    assert HC.expected("leaf_n257_d32")["n_clusters"] >= 2 and HC.expected("leaf_n129_d1")["n_clusters"] >= 2
    assert HC.case("ms64_n257_d32")[2] == 64 == PJ.MAX_K
    r = HC.expected("n1650_d32")
    assert len(r["labels"]) == 1650 and r["n_clusters"] == 5


def test_which_cases_do_not_depend_on_the_row_order():
    found = tuple(name for name in HC.CASES if HC.permutation_invariant(name))
    print("row-permutation invariant:", found)
    assert found == HC.INVARIANT_CASES
    assert "lattice" not in found and set(HC.BLOB_CASES) <= set(found)


# ---- the host tree tail ------------------------------------------------------------------------------------------------
def tree(I, J, dist, n, min_cluster_size, method):
    lib = _lib.load()
    I, J = np.ascontiguousarray(I, dtype=np.int64), np.ascontiguousarray(J, dtype=np.int64)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    labels, prob, linkage = np.full(n, -7, dtype=np.int64), np.full(n, -7.0), np.full((n - 1, 4), -7.0)
    count = ctypes.c_int(-7)
    rc = lib.ava_hd_tree(I.ctypes.data, J.ctypes.data, dist.ctypes.data, n, min_cluster_size, method,
                         labels.ctypes.data, prob.ctypes.data, ctypes.addressof(count), linkage.ctypes.data)
    return rc, labels, prob, count.value, linkage


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_tree_tail_against_the_restatement(name):
    """ava_hd_tree fed the restatement's edges: the same labels, linkage matrix and counts, probabilities within
    4 * 2^-53; the precomputed form of the same rows (distances w) likewise"""
    X, mcs, ms, method = HC.case(name)
    forms = [HC.expected(name)] + ([HC.precomputed(name)[1]] if name in HC.PRECOMPUTED_CASES else [])
    for want in forms:
        I, J = want["edges"]
        rc, labels, prob, count, linkage = tree(I, J, want["mst"][:, 2], len(X), mcs, 0 if method == 'eom' else 1)
        assert rc == 0
        equal(labels, want["labels"])
        equal(linkage, want["linkage"])
        assert count == want["n_clusters"] and int((labels == -1).sum()) == want["n_noise"]
        err = np.abs(prob - want["probabilities"])
        print("%s: max relative probability error %.2e, bound %.2e"
              % (name, float((err / np.maximum(want["probabilities"], 1e-300)).max()), PROB_RTOL))
        assert np.all(err <= PROB_RTOL * want["probabilities"])
        assert np.all((prob >= 0.0) & (prob <= 1.0)) and np.all(prob[labels == -1] == 0.0)


def test_tree_tail_refusals():
    want = HC.expected("n65_d33")
    I, J = want["edges"]
    dist, n = want["mst"][:, 2], 65
    assert tree(I, J, dist, n, 8, 0)[0] == 0
    assert tree(I, J, dist, n, 1, 0)[0] == -1                              # min_cluster_size < 2
    assert tree(I, J, dist, n, 8, 2)[0] == -1 and tree(I, J, dist, n, 8, -1)[0] == -1
    assert tree(I[:0], J[:0], dist[:0], 1, 8, 0)[0] == -1                  # n < 2
    bad = J.copy()
    bad[3] = n
    assert tree(I, bad, dist, n, 8, 0)[0] == -1                            # a row that does not exist
    bad = J.copy()
    bad[-1], loop = J[0], I.copy()
    loop[-1] = I[0]
    assert tree(loop, bad, dist, n, 8, 0)[0] == -1                         # an edge twice: no spanning tree
    nan = dist.copy()
    nan[5] = np.nan
    assert tree(I, J, nan, n, 8, 0)[0] == -1
    lib = _lib.load()
    p = np.zeros(1024).ctypes.data
    ok = [p, p, p, 2, 2, 0, p, p, p, p]
    for i in (0, 1, 2, 6, 7, 8, 9):
        a = list(ok)
        a[i] = None
        assert lib.ava_hd_tree(*a) == -1, i


# ---- argument checks that need no device -----------------------------------------------------------------------------
def test_checks_run_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(HD, "_device", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    X = HC.case("n63_d31")[0]
    holes = np.arange(X.size).reshape(X.shape) == 7
    for mcs in (1, 0, -3, 2.5, 5.0, "4", None, True):
        with pytest.raises(ValueError, match="'min_cluster_size' parameter of HDBSCAN must be an int in the range "
                                             r"\[2, inf\)"):
            HD.HDBSCAN(min_cluster_size=mcs).fit(X)
    for ms in (0, -3, 2.5, 5.0, "4", True):
        with pytest.raises(ValueError, match=r"'min_samples' parameter of HDBSCAN must be an int in the range \[1, inf\)"
                                             " or None"):
            HD.HDBSCAN(min_samples=ms).fit(X)
        with pytest.raises(ValueError, match="'min_samples' parameter"):
            HD.mutual_reachability_mst(X, ms)
    with pytest.raises(ValueError, match="'min_samples' parameter"):
        HD.mutual_reachability_mst(X, None)
    for fn in (lambda: HD.HDBSCAN(min_samples=len(X) + 1).fit(X), lambda: HD.HDBSCAN(len(X) + 1).fit(X),
               lambda: HD.mutual_reachability_mst(X, len(X) + 1)):
        with pytest.raises(ValueError, match=r"min_samples \(64\) must be at most the number of samples in X \(63\)"):
            fn()
    wide = HC.case("n257_d32")[0]
    for fn in (lambda: HD.HDBSCAN(min_samples=PJ.MAX_K + 1).fit(wide), lambda: HD.HDBSCAN(PJ.MAX_K + 1).fit(wide),
               lambda: HD.mutual_reachability_mst(wide, PJ.MAX_K + 1)):
        with pytest.raises(ValueError, match="must be at most %d" % PJ.MAX_K):
            fn()
    with pytest.raises(ValueError, match="n_samples=1 while HDBSCAN requires more than one sample"):
        HD.HDBSCAN(2, min_samples=1).fit(X[:1])
    with pytest.raises(ValueError, match="'cluster_selection_method' parameter"):
        HD.HDBSCAN(cluster_selection_method="best").fit(X)
    for metric in ("cosine", "manhattan", None):
        with pytest.raises(NotImplementedError):
            HD.HDBSCAN(metric=metric).fit(X)
        with pytest.raises(NotImplementedError):
            HD.mutual_reachability_mst(X, 3, metric=metric)
    rows = [(X[:, 0], "Expected 2D array"), (np.where(holes, np.nan, X), "Input X contains NaN."),
            (np.where(holes, np.inf, X), "Input X contains infinity"),
            (torch.from_numpy(np.where(holes, np.nan, X)), "Input X contains NaN."),
            (np.zeros((0, 3)), "minimum of 1 is required")]
    for bad, message in rows:
        with pytest.raises(ValueError, match=message):
            HD.HDBSCAN().fit(bad)
        with pytest.raises(ValueError, match=message):
            HD.mutual_reachability_mst(bad, 3)
    with pytest.raises(ValueError, match="square distance matrix"):
        HD.HDBSCAN(metric="precomputed").fit(X)
    with pytest.raises(ValueError, match="at most %d" % HD.MAX_N):
        HD.HDBSCAN().fit(np.zeros((HD.MAX_N + 1, 1), dtype=np.float32))


def test_parameters_that_are_not_accepted():
    for extra in ({"allow_single_cluster": True}, {"cluster_selection_epsilon": 0.5}, {"alpha": 2.0},
                  {"max_cluster_size": 10}, {"algorithm": "brute"}):
        with pytest.raises(TypeError):
            HD.HDBSCAN(**extra)


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X = HC.case("n63_d31")[0]
    with pytest.raises(_lib.AvaHipError):
        HD.HDBSCAN().fit(X)
    with pytest.raises(_lib.AvaHipError):
        HD.HDBSCAN().fit_predict(X)
    with pytest.raises(_lib.AvaHipError):
        HD.HDBSCAN(metric='precomputed').fit(HC.measures(X))
    with pytest.raises(_lib.AvaHipError):
        HD.mutual_reachability_mst(X, 4)


def test_constructor_keeps_its_parameters():
    m = HD.HDBSCAN()
    assert (m.min_cluster_size, m.min_samples, m.metric, m.cluster_selection_method) == (5, None, 'euclidean', 'eom')
    m = HD.HDBSCAN(9, min_samples=3, metric='precomputed', cluster_selection_method='leaf')
    assert (m.min_cluster_size, m.min_samples, m.metric, m.cluster_selection_method) == (9, 3, 'precomputed', 'leaf')
    with pytest.raises(TypeError):
        HD.HDBSCAN(5, 3)                                                  # keyword-only, as sklearn's


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def up256(x):
    return (x + 255) // 256 * 256


def test_library_argument_checks():
    """ava_hd_* return sizes / AVA_EINVAL / AVA_EWORKSPACE before any HIP call (the test runs without a device, where a
    HIP call would return AVA_ELAUNCH instead)"""
    lib = _lib.load()
    for n, d in ((1, 4), (0, 4), (-1, 4), (10, 0), (10, 65537), (HD.MAX_N + 1, 4)):
        assert lib.ava_hd_workspace_bytes(n, d) == 0, (n, d)
    for n, d in ((2, 1), (65, 33), (1650, 32), (5000, 65536), (100000, 32), (HD.MAX_N, 1)):
        tiles = -(-n // 64)
        segs = max(1, min(8, 4096 // tiles, tiles))
        want = (2 * up256(4 * n) + up256(4 * segs * n) + up256(4) + up256(8 * tiles) + 3 * up256(8 * n)
                + 2 * up256(8 * segs * n) + 256)
        assert lib.ava_hd_workspace_bytes(n, d) == want, (n, d)
    for n, want in ((1, 0), (2, 1), (3, 2), (64, 6), (65, 7), (1650, 11), (HD.MAX_N, 21), (HD.MAX_N + 1, 0)):
        assert lib.ava_hd_max_rounds(n) == want
    p = np.zeros(256, dtype=np.float64).ctypes.data
    big = 1 << 30

    def refuses(fn, ok, bad_args):
        for i, bad in bad_args:
            a = list(ok)
            a[i] = bad
            assert fn(*a, None) == -1, (fn.__name__, i, bad)

    # x, dtype, n, d, kth, core
    refuses(lib.ava_hd_core, [p, 1, 8, 2, p, p],
            ((0, None), (1, 2), (1, -1), (2, 1), (2, 0), (2, HD.MAX_N + 1), (3, 0), (3, 65537), (4, None), (5, None)))
    # dist, dtype, n, k, core
    refuses(lib.ava_hd_core_pre, [p, 1, 8, 3, p],
            ((0, None), (1, 2), (2, 1), (2, HD.MAX_N + 1), (3, 0), (3, 9), (3, 65), (4, None)))
    # x, dtype, n, d, core, ei, ej, ew, em, rounds, rowmin_ms, ws, ws_bytes
    ok = [p, 1, 8, 2, p, p, p, p, p, p, None, p, big]
    refuses(lib.ava_hd_mst, ok, ((0, None), (1, 2), (2, 1), (2, HD.MAX_N + 1), (3, 0), (3, 65537), (4, None), (5, None),
                                 (6, None), (7, None), (8, None), (9, None), (11, None)))
    assert lib.ava_hd_mst(*(ok[:12] + [8]), None) == -3
    # dist, dtype, n, core, ...
    ok = [p, 1, 8, p, p, p, p, p, p, None, p, big]
    refuses(lib.ava_hd_mst_pre, ok, ((0, None), (1, 2), (2, 1), (2, HD.MAX_N + 1), (3, None), (4, None), (5, None),
                                     (6, None), (7, None), (8, None), (10, None)))
    assert lib.ava_hd_mst_pre(*(ok[:11] + [8]), None) == -3
