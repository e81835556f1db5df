"""The kernels of csrc/dbscan.hip and ava_amd.dbscan on the MI355X: labels, core rows, neighbour counts and cluster
counts against the restatement of tests/dbscan_cases.py and scikit-learn's own results (tests/golden/dbscan.npz) at tile
and stage edges (SQD_T = 64 rows, SQD_KC = 32 features), on a chain of ten tiles in three row orders (the descending one
builds long parent chains under min-root hooking and makes the compare-and-swap retry), on a border row whose
smallest-index core neighbour is in the higher cluster, on pairs exactly at eps, on duplicate rows, in the degenerate
settings and on a realistic 1650 x 32 cloud; the input forms and repeat runs that must not change a label, the
precomputed metric, the radius sweep with its silhouette scores, row permutations, k_distances and the error paths.

Every label comparison is exact (``assert_array_equal``): tests/test_cpu_dbscan.py shows that the restatement is
sklearn's and that no pair of a non-tie case is within 1e-9 (relative, of eps^2) of the radius, where the device's
squared distance is within (d + 2) 2^-53.  N = 1 and N = 2 cannot hold core rows, border rows and noise at once (a border
row needs a core row with a neighbour it lacks, and the noise a fourth row); every other tile-edge case does."""
import numpy as np
import pytest
import torch

import dbscan_cases as DC
from conftest import load_golden
from ava_amd import cluster_metrics as CM
from ava_amd import dbscan as DB

pytestmark = pytest.mark.gpu
equal = np.testing.assert_array_equal


@pytest.fixture(scope="module")
def golden():
    return load_golden("dbscan.npz")


def fit(X, eps, min_samples, metric='euclidean'):
    return DB.DBSCAN(eps, min_samples=min_samples, metric=metric).fit(X)


# ---- every case against the restatement and sklearn --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_case_against_restatement_and_sklearn(golden, name):
    X, eps, min_samples = DC.case(name)
    want = DC.expected(name)
    if name in DC.MIXED_CASES:
        assert len(want["core_idx"]) and want["n_border"] and want["n_noise"]
    m = fit(X, eps, min_samples)
    assert m.labels_.dtype == np.int64 and m.core_sample_indices_.dtype == np.int64
    equal(m.labels_, want["labels"])
    equal(m.core_sample_indices_, want["core_idx"])
    assert m.n_clusters_ == want["n_clusters"] and m.n_noise_ == want["n_noise"]
    assert m.components_.shape == (len(want["core_idx"]), X.shape[1]) and m.components_.dtype == X.dtype
    equal(m.components_, X[want["core_idx"]])
    counts = DB.neighbor_counts(X, eps)
    assert counts.dtype == np.int64 and counts.shape == (len(X),)
    equal(counts, want["counts"])
    # sklearn's own
    equal(m.labels_, golden[name + "_labels"])
    equal(m.core_sample_indices_, golden[name + "_core"])
    assert m.n_clusters_ == int(golden[name + "_n_clusters"])
    # float32 rows and their float64 copies, host arrays and device tensors, and a second run: the same labels
    assert X.dtype == np.float32
    for rows in (X.astype(np.float64), torch.from_numpy(X), torch.from_numpy(X).cuda(),
                 torch.from_numpy(X.astype(np.float64)).cuda(), X):
        again = DB.DBSCAN(eps, min_samples=min_samples)
        equal(again.fit_predict(rows), m.labels_)
        equal(again.core_sample_indices_, m.core_sample_indices_)
    equal(DB.neighbor_counts(torch.from_numpy(X).cuda().double(), eps), counts)


def test_degenerate_settings():
    X, eps, min_samples = DC.case("deg_msN1")
    m = fit(X, eps, min_samples)
    assert min_samples == len(X) + 1 and np.all(m.labels_ == -1) and m.n_clusters_ == 0 and m.n_noise_ == len(X)
    assert m.components_.shape == (0, X.shape[1]) and m.core_sample_indices_.shape == (0,)
    X, eps, min_samples = DC.case("deg_ms1")
    m = fit(X, eps, min_samples)
    assert len(m.core_sample_indices_) == len(X) and m.n_noise_ == 0
    alone = DB.neighbor_counts(X, eps) == 1
    assert alone.any() and np.all(np.bincount(m.labels_)[m.labels_[alone]] == 1)     # isolated rows: clusters of one
    X, eps, min_samples = DC.case("deg_huge")
    m = fit(X, eps, min_samples)
    assert np.all(m.labels_ == 0) and m.n_clusters_ == 1
    X, eps, min_samples = DC.case("deg_tiny")
    assert np.all(DB.neighbor_counts(X, eps) == 1) and np.all(fit(X, eps, min_samples).labels_ == -1)


def test_bridge_takes_the_smaller_cluster_number():
    X, eps, min_samples = DC.case("bridge")
    m = fit(X, eps, min_samples)
    assert m.labels_[1] == 1 and m.labels_[10] == 0 and 11 not in m.core_sample_indices_
    assert m.labels_[11] == 0 and m.labels_[12] == -1


def test_chain_is_one_cluster_in_every_row_order():
    for order in ("asc", "desc", "shuf"):
        X, eps, min_samples = DC.case("chain_" + order)
        for _ in range(3):                                                # the union's result does not depend on the run
            m = fit(X, eps, min_samples)
            assert m.n_clusters_ == 1 and np.all(m.labels_ == 0)
            equal(m.core_sample_indices_, DC.expected("chain_" + order)["core_idx"])


# ---- precomputed distances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n65_d33", "n257_d32", "bridge", "chain_shuf"])
def test_precomputed(name):
    X, eps, min_samples = DC.case(name)
    want = DC.expected(name)
    D, margin = DC.precomputed(name)
    assert margin >= DC.MARGIN
    m = fit(D, eps, min_samples, metric='precomputed')
    equal(m.labels_, want["labels"])
    equal(m.core_sample_indices_, want["core_idx"])
    equal(m.components_, D[want["core_idx"]])
    equal(DB.neighbor_counts(D, eps, metric='precomputed'), want["counts"])
    equal(fit(torch.from_numpy(D).cuda(), eps, min_samples, metric='precomputed').labels_, want["labels"])
    # float32 distances are accepted as they are: (double)D[i][j] <= eps is exact in every arithmetic, margin or not
    D32 = D.astype(np.float32)
    equal(fit(D32, eps, min_samples, metric='precomputed').labels_,
          DC.restate(DC.within(D32, eps, 'precomputed')[0], min_samples)["labels"])
    out = DB.dbscan_sweep(D, [eps, 2.0 * eps], min_samples=min_samples, metric='precomputed')
    equal(out["labels"][0], want["labels"])


def test_precomputed_refusals():
    X, eps, min_samples = DC.case("n65_d33")
    D = DC.precomputed("n65_d33")[0]
    skew = D.copy()
    skew[3, 7] = np.nextafter(skew[3, 7], 0.0)
    for fn in (lambda A: fit(A, eps, min_samples, metric='precomputed'),
               lambda A: DB.neighbor_counts(A, eps, metric='precomputed'),
               lambda A: DB.dbscan_sweep(A, [eps], metric='precomputed')):
        with pytest.raises(ValueError, match="must be symmetric"):
            fn(skew)
        with pytest.raises(ValueError, match="must be symmetric"):
            fn(torch.from_numpy(skew).cuda())
        with pytest.raises(ValueError, match="square distance matrix"):
            fn(D[:, :-1])
        with pytest.raises(ValueError, match="square distance matrix"):
            fn(X)


# ---- the radius sweep --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [8, 9, 1])
def test_sweep(count):
    X, _, min_samples = DC.case(DC.SWEEP_CASE)
    radii = DC.sweep_radii(count)
    out = DB.dbscan_sweep(X, radii, min_samples=min_samples, scores=True)
    assert out["labels"].shape == out["core"].shape == (count, len(X)) and out["labels"].dtype == np.int64
    assert out["core"].dtype == np.bool_ and out["n_clusters"].dtype == out["n_noise"].dtype == np.int64
    equal(out["eps"], np.asarray(radii))
    counts = DB.neighbor_counts(X, list(radii))
    assert counts.shape == (count, len(X))
    finite = 0
    for e, r in enumerate(radii):
        single = fit(X, r, min_samples)
        want = DC.restate(DC.within(X, r)[0], min_samples)
        equal(out["labels"][e], single.labels_)
        equal(out["labels"][e], want["labels"])
        equal(np.flatnonzero(out["core"][e]), single.core_sample_indices_)
        equal(counts[e], want["counts"])
        equal(counts[e], DB.neighbor_counts(X, r))
        lab = out["labels"][e]
        assert out["n_clusters"][e] == single.n_clusters_ == lab.max() + 1 == len(np.unique(lab[lab >= 0]))
        assert out["n_noise"][e] == single.n_noise_ == (lab == -1).sum()
        keep = lab != -1
        if 2 <= out["n_clusters"][e] < keep.sum():
            assert out["silhouette"][e] == CM.silhouette_score(X[keep], lab[keep])        # the same bits
            finite += 1
        else:
            assert np.isnan(out["silhouette"][e])
    if count >= 8:
        assert out["n_noise"][0] == len(X) and out["n_clusters"][-1] == 1 and out["n_noise"][-1] == 0
        assert np.isnan(out["silhouette"][0]) and np.isnan(out["silhouette"][-1]) and finite >= 2
    assert "silhouette" not in DB.dbscan_sweep(X, radii[:1], min_samples=min_samples)


def test_sweep_silhouette_is_nan_where_it_is_undefined():
    X, eps, _ = DC.case("deg_ms1")
    out = DB.dbscan_sweep(X, [1e-6, eps], min_samples=1, scores=True)
    assert out["n_clusters"][0] == len(X) and np.isnan(out["silhouette"][0])           # every row alone
    assert 2 <= out["n_clusters"][1] < len(X) and np.isfinite(out["silhouette"][1])
    grid = 10.0 * np.stack(np.divmod(np.arange(CM.MAX_K + 76), 40), axis=1)
    pairs = np.repeat(grid, 2, axis=0).astype(np.float32)                               # 1100 clusters of two copies
    out = DB.dbscan_sweep(pairs, [1.0], min_samples=2, scores=True)
    assert out["n_clusters"][0] == CM.MAX_K + 76 and out["n_noise"][0] == 0 and np.isnan(out["silhouette"][0])
    equal(out["labels"][0], np.arange(2 * (CM.MAX_K + 76)) // 2)


# ---- row permutations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n128_d2", "n257_d32", "bridge", "duplicates", "chain_asc"])
def test_row_permutation(name):
    X, eps, min_samples = DC.case(name)
    want = DC.expected(name)
    base = fit(X, eps, min_samples)
    perm = np.random.default_rng(5).permutation(len(X))
    m = fit(X[perm], eps, min_samples)
    equal(np.sort(perm[m.core_sample_indices_]), base.core_sample_indices_)
    back = np.empty(len(X), dtype=np.int64)
    back[perm] = m.labels_
    assert m.n_clusters_ == base.n_clusters_
    equal(DC.by_smallest_member(back, want["core"]), DC.by_smallest_member(base.labels_, want["core"]))
    if want["ambiguous"] == 0:
        equal(DC.by_smallest_member(back), DC.by_smallest_member(base.labels_))
    else:
        assert name == "bridge"


# ---- k_distances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n65_d33", "n129_d1", "n257_d32", "n128_d65"])
def test_k_distances(name):
    X, eps, min_samples = DC.case(name)
    d = X.shape[1]
    for k in (1, min_samples, 7):
        got = DB.k_distances(X, k)
        want = DC.kth_distances(X, k)
        assert got.dtype == np.float64 and got.shape == (len(X),) and np.all(np.diff(got) >= 0)
        err = np.abs(got - want)
        print("k = %d: max rel err %.2e, bound %.2e" % (k, float((err / np.maximum(want, 1e-300)).max()), (d + 3) * DC.U))
        assert np.all(err <= (d + 3) * DC.U * want)
    assert (DB.k_distances(X, min_samples) <= eps).sum() == len(DC.expected(name)["core_idx"])
    equal(DB.k_distances(torch.from_numpy(X).cuda().double(), min_samples), DB.k_distances(X, min_samples))


# ---- error paths -------------------------------------------------------------------------------------------------------
def test_error_paths():
    X = DC.case("n63_d31")[0]
    for eps in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="'eps' parameter"):
            fit(X, eps, 5)
        with pytest.raises(ValueError, match="'eps' parameter"):
            DB.dbscan_sweep(X, [1.0, eps])
    for min_samples in (0, 2.5):
        with pytest.raises(ValueError, match="'min_samples' parameter"):
            fit(X, 1.0, min_samples)
    with pytest.raises(NotImplementedError):
        fit(X, 1.0, 5, metric="cosine")
    bad = X.copy()
    bad[5, 3] = np.nan
    for rows in (bad, torch.from_numpy(bad).cuda()):
        with pytest.raises(ValueError, match="Input X contains NaN."):
            fit(rows, 1.0, 5)
        with pytest.raises(ValueError, match="Input X contains NaN."):
            DB.k_distances(rows, 3)
    with pytest.raises(ValueError, match="Expected 2D array"):
        fit(X[:, 0], 1.0, 5)
    with pytest.raises(ValueError, match="eps_list is empty"):
        DB.dbscan_sweep(X, [])
    with pytest.raises(ValueError, match="k must be"):
        DB.k_distances(X, 65)
