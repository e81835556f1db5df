"""The kernels of csrc/hdbscan.hip and ava_amd.hdbscan on the MI355X: the spanning tree's edges and weights, the core
distances, labels, probabilities, counts and the single-linkage matrix against the restatement of
tests/hdbscan_cases.py, and on the blob cases against scikit-learn's own results (tests/golden/hdbscan.npz), at tile and
stage edges (SQD_T = 64 rows, SQD_KC = 32 features), with one to eight column segments per strip, on a chain of ten
tiles in three row orders (long hook chains, deep pointer jumping), on a lattice where the row tiebreak decides, on
duplicate rows (distance 0, lambda = inf), on the hand-built hub row, under 'leaf' and at min_samples = 64; the input
forms and repeat runs that must not change a bit, the precomputed metric, row permutations, mutual_reachability_mst and
the error paths.

Edges, weights, core distances, labels and linkage matrices compare with ``==``: the inputs are exact
(hdbscan_cases.py; tests/test_cpu_hdbscan.py checks it), so the device's d2 is the restatement's number and every key
comparison is decided.  Probabilities are one square root, one reciprocal and one division from there: 4 * 2^-53."""
import math

import numpy as np
import pytest
import torch

import dbscan_cases as DC
import hdbscan_cases as HC
from conftest import load_golden
from ava_amd import hdbscan as HD

pytestmark = pytest.mark.gpu
equal = np.testing.assert_array_equal
PROB_RTOL = 4 * HC.U


@pytest.fixture(scope="module")
def golden():
    return load_golden("hdbscan.npz")


def fit(X, mcs, ms, method='eom', metric='euclidean'):
    return HD.HDBSCAN(mcs, min_samples=ms, metric=metric, cluster_selection_method=method).fit(X)


def check(m, want, n):
    assert m.mst_.dtype == np.float64 and m.mst_.shape == (n - 1, 3)
    equal(m.mst_, want["mst"])
    assert m.core_distances_.dtype == np.float64
    equal(m.core_distances_, want["core_distances"])
    assert m.labels_.dtype == np.int64 and m.probabilities_.dtype == np.float64
    equal(m.labels_, want["labels"])
    err = np.abs(m.probabilities_ - want["probabilities"])
    print("max relative probability error %.2e, bound %.2e"
          % (float((err / np.maximum(want["probabilities"], 1e-300)).max()), PROB_RTOL))
    assert np.all(err <= PROB_RTOL * want["probabilities"])
    assert m.n_clusters_ == want["n_clusters"] and m.n_noise_ == want["n_noise"]
    equal(m.single_linkage_tree_, want["linkage"])
    assert 1 <= m.n_boruvka_rounds_ <= math.ceil(math.log2(n))


# ---- every case against the restatement and sklearn --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_case_against_restatement_and_sklearn(golden, name):
    X, mcs, ms, method = HC.case(name)
    want = HC.expected(name)
    m = fit(X, mcs, ms, method)
    check(m, want, len(X))
    assert m.n_features_in_ == X.shape[1]
    if name in HC.BLOB_CASES:                                             # sklearn's own
        equal(DC.by_smallest_member(m.labels_), DC.by_smallest_member(golden[name + "_labels"]))
        err = float(np.abs(m.probabilities_ - golden[name + "_probabilities"]).max())
        print("max |device - sklearn| over probabilities_ %.2e, prob_err %.2e" % (err, float(golden[name + "_prob_err"])))
        assert err <= 8 * float(golden[name + "_prob_err"])
    # float32 rows and their float64 copies, host arrays and device tensors, and a second run: the same bits
    assert X.dtype == np.float32
    for rows in (X.astype(np.float64), torch.from_numpy(X), torch.from_numpy(X).cuda(),
                 torch.from_numpy(X.astype(np.float64)).cuda(), X):
        again = HD.HDBSCAN(mcs, min_samples=ms, cluster_selection_method=method)
        equal(again.fit_predict(rows), m.labels_)
        equal(again.mst_, m.mst_)
        equal(again.probabilities_, m.probabilities_)
        equal(again.core_distances_, m.core_distances_)
        equal(again.single_linkage_tree_, m.single_linkage_tree_)
        assert again.n_boruvka_rounds_ == m.n_boruvka_rounds_
    mst, core = HD.mutual_reachability_mst(X, mcs if ms is None else ms)
    equal(mst, m.mst_)
    equal(core, m.core_distances_)


def test_hub_row_follows_the_key_order():
    X, mcs, ms, _ = HC.case("hub")
    m = fit(X, mcs, ms)
    equal(m.labels_, [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1])                    # asserted by hand: hdbscan_cases._hub_case
    assert m.core_distances_[HC.HUB] == 4.0 and m.probabilities_[HC.HUB] < 1.0
    at = [tuple(e) for e in m.mst_.tolist() if HC.HUB in e[:2]]
    assert at == [(4.0, 5.0, 4.0), (5.0, 6.0, 4.0)]
    rev = fit(X[::-1].copy(), mcs, ms)                                    # reversed rows: it goes to the other group
    equal(rev.labels_, [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1])


def test_duplicates_merge_at_distance_zero():
    X, mcs, ms, _ = HC.case("duplicates")
    m = fit(X, mcs, ms)
    assert (m.mst_[:, 2] == 0.0).sum() == 5 and np.all(m.core_distances_[5:9] == 0.0)
    assert len(set(m.labels_[5:9])) == 1 and m.labels_[5] >= 0 and np.all(m.probabilities_[5:9] == 1.0)


# ---- precomputed distances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.PRECOMPUTED_CASES)
def test_precomputed(name):
    X, mcs, ms, method = HC.case(name)
    D, want = HC.precomputed(name)
    m = fit(D, mcs, ms, method, metric='precomputed')
    check(m, want, len(D))
    equal(m.mst_[:, :2], HC.expected(name)["mst"][:, :2])                  # the same keys, so the same tree
    assert m.n_features_in_ == len(D)
    again = fit(torch.from_numpy(D).cuda(), mcs, ms, method, metric='precomputed')
    equal(again.labels_, m.labels_)
    equal(again.mst_, m.mst_)
    equal(again.probabilities_, m.probabilities_)
    # float32 distances are read as they are: (double)D[i][j] is exact, so the restatement of the rounded matrix holds
    D32 = D.astype(np.float32)
    check(fit(D32, mcs, ms, method, metric='precomputed'),
          HC.restate(D32.astype(np.float64), mcs, ms, metric='precomputed', method=method), len(D))
    mst, core = HD.mutual_reachability_mst(D, mcs if ms is None else ms, metric='precomputed')
    equal(mst, m.mst_)
    equal(core, m.core_distances_)


def test_precomputed_refusals():
    X, mcs, ms, _ = HC.case("n65_d33")
    D = HC.precomputed("n65_d33")[0]
    skew = D.copy()
    skew[3, 7] = np.nextafter(skew[3, 7], 0.0)
    for fn in (lambda A: fit(A, mcs, ms, metric='precomputed'),
               lambda A: HD.mutual_reachability_mst(A, ms, metric='precomputed')):
        with pytest.raises(ValueError, match="must be symmetric"):
            fn(skew)
        with pytest.raises(ValueError, match="must be symmetric"):
            fn(torch.from_numpy(skew).cuda())
        with pytest.raises(ValueError, match="square distance matrix"):
            fn(D[:, :-1])
        with pytest.raises(ValueError, match="square distance matrix"):
            fn(X)


# ---- row permutations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n128_d2", "n257_d32", "hub", "duplicates", "chain_asc"])
def test_row_permutation(name):
    assert name in HC.INVARIANT_CASES
    X, mcs, ms, method = HC.case(name)
    perm = HC.permutation(name)
    base, m = fit(X, mcs, ms, method), fit(X[perm], mcs, ms, method)
    assert m.n_clusters_ == base.n_clusters_ and m.n_noise_ == base.n_noise_
    assert HC.same_partition(base.labels_, m.labels_, perm)
    equal(np.sort(m.mst_[:, 2]), np.sort(base.mst_[:, 2]))
    equal(m.core_distances_, base.core_distances_[perm])


# ---- error paths -------------------------------------------------------------------------------------------------------
def test_error_paths():
    X = HC.case("n63_d31")[0]
    Xd = torch.from_numpy(X).cuda()
    for rows in (X, Xd):
        with pytest.raises(ValueError, match="'min_cluster_size' parameter"):
            fit(rows, 1, None)
        with pytest.raises(ValueError, match="'min_samples' parameter"):
            fit(rows, 5, 0)
        with pytest.raises(ValueError, match=r"min_samples \(64\) must be at most the number of samples in X \(63\)"):
            fit(rows, 5, 64)
        with pytest.raises(NotImplementedError):
            fit(rows, 5, None, metric="cosine")
        with pytest.raises(ValueError, match="'cluster_selection_method' parameter"):
            fit(rows, 5, None, method="best")
        with pytest.raises(ValueError, match="'min_samples' parameter"):
            HD.mutual_reachability_mst(rows, 2.5)
    with pytest.raises(ValueError, match="must be at most 64"):
        fit(torch.from_numpy(HC.case("n257_d32")[0]).cuda(), 5, 65)
    bad = X.copy()
    bad[5, 3] = np.nan
    for rows in (bad, torch.from_numpy(bad).cuda()):
        with pytest.raises(ValueError, match="Input X contains NaN."):
            fit(rows, 5, None)
        with pytest.raises(ValueError, match="Input X contains NaN."):
            HD.mutual_reachability_mst(rows, 3)
    with pytest.raises(ValueError, match="Expected 2D array"):
        fit(Xd[:, 0], 5, None)
    with pytest.raises(ValueError, match="n_samples=1"):
        fit(Xd[:1], 2, 1)
