"""ava_amd.dbscan without a GPU: the restatement of tests/dbscan_cases.py against scikit-learn's own DBSCAN in all four
``algorithm`` settings, the margin of every case, the tie cases' exactness, the content of tests/golden/dbscan.npz, the
argument checks that need no device and the C ABI's mirror and refusals.

All label comparisons are exact: the labels are determined by the data (dbscan_cases.py), so there is no tolerance."""

import numpy as np
import pytest
import torch

import dbscan_cases as DC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import dbscan as DB

ALGORITHMS = ("brute", "kd_tree", "ball_tree", "auto")


@pytest.fixture(scope="module")
def golden():
    return load_golden("dbscan.npz")


# ---- the restatement, the margin, the golden file ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_restatement_is_sklearns(golden, name):
    """labels and core indices of the four rules == sklearn 1.7's on the float64 copy, under every algorithm, and the
    golden file holds exactly those"""
    from sklearn.cluster import DBSCAN
    X, eps, min_samples = DC.case(name)
    want = DC.expected(name)
    for algorithm in ALGORITHMS:
        sk = DBSCAN(eps=eps, min_samples=min_samples, algorithm=algorithm).fit(X.astype(np.float64))
        np.testing.assert_array_equal(want["labels"], sk.labels_, err_msg=algorithm)
        np.testing.assert_array_equal(want["core_idx"], sk.core_sample_indices_, err_msg=algorithm)
    np.testing.assert_array_equal(golden[name + "_labels"], sk.labels_)
    np.testing.assert_array_equal(golden[name + "_core"], sk.core_sample_indices_)
    assert golden[name + "_labels"].dtype == golden[name + "_core"].dtype == np.int64
    assert int(golden[name + "_n_clusters"]) == want["n_clusters"] == int(sk.labels_.max()) + 1
    assert float(golden[name + "_margin"]) == want["margin"]


def test_golden_holds_the_cases_and_nothing_else(golden):
    assert sorted(golden) == sorted("%s_%s" % (n, q) for n in DC.CASES for q in ("labels", "core", "n_clusters", "margin"))


def test_margins():
    """every case that is not a tie case keeps every pair at least 1e-9 (relative, of eps^2) from the radius, its
    precomputed form and the sweep's radii too; a tie case has a pair exactly on it"""
    for name in DC.CASES:
        margin = DC.expected(name)["margin"]
        print("%-14s margin %.2e" % (name, margin))
        assert (margin == 0.0) if name in DC.TIE_CASES else (margin >= DC.MARGIN), name
    for name in ("n65_d33", "n257_d32", "bridge", "chain_shuf"):
        assert DC.precomputed(name)[1] >= DC.MARGIN, name
    for count in (1, 8, 9):
        assert len(DC.sweep_radii(count)) == count                        # asserts each radius' margin


def test_tie_cases_are_exact():
    """integer coordinates |x| <= 2^20 and an integer eps: float32, float64 and longdouble sums are the same numbers"""
    for name in DC.TIE_CASES:
        X, eps, _ = DC.case(name)
        assert np.all(X == np.round(X)) and np.abs(X).max() <= 2 ** 20 and eps == round(eps)
        d2 = DC.sqdist(X)
        assert np.all(d2 == np.round(d2)) and float(d2.max()) < 2.0 ** 53
        assert (d2 == eps * eps).sum() > 0


def test_cases_exercise_what_they_are_for():
    for name in DC.MIXED_CASES:
        r = DC.expected(name)
        assert len(r["core_idx"]) and r["n_border"] and r["n_noise"], name
    for order in ("asc", "desc", "shuf"):
        r = DC.expected("chain_" + order)
        assert r["n_clusters"] == 1 and r["n_noise"] == 0 and len(r["labels"]) == 600
    # the bridge: its smallest-index core neighbour is in the higher cluster, its label is the lower
    X, eps, min_samples = DC.case("bridge")
    r = DC.expected("bridge")
    W = DC.within(X, eps)[0]
    near = np.flatnonzero(W[11] & r["core"])
    assert not r["core"][11] and list(near) == [1, 10] and r["ambiguous"] == 1
    assert r["labels"][near[0]] == 1 and r["labels"][near[1]] == 0 and r["labels"][11] == 0
    # ties: rows with exactly min_samples neighbours are core rows
    r = DC.expected("ties")
    np.testing.assert_array_equal(r["core_idx"], [1, 2, 8])
    assert np.all(r["counts"][r["core_idx"]] == 3)
    np.testing.assert_array_equal(r["labels"], [0, 0, 0, 0, -1, -1, -1, 1, 1, 1, -1])
    # duplicates: min_samples copies are a cluster, one fewer are noise
    r = DC.expected("duplicates")
    assert len(set(r["labels"][5:9])) == 1 and r["labels"][5] >= 0 and np.all(r["counts"][5:9] == 4)
    assert np.all(r["labels"][20:23] == -1) and np.all(r["counts"][20:23] == 3)
    # the degenerate settings
    r = DC.expected("deg_ms1")
    assert r["core"].all() and (np.bincount(r["labels"]) == 1).any()
    assert DC.expected("deg_msN1")["n_clusters"] == 0 and np.all(DC.expected("deg_msN1")["labels"] == -1)
    assert DC.expected("deg_huge")["n_clusters"] == 1 and DC.expected("deg_huge")["core"].all()
    assert np.all(DC.expected("deg_tiny")["counts"] == 1)
    r = DC.expected("blobs1500_d32")
    assert r["n_clusters"] == 5 and r["n_border"] >= 200 and len(r["labels"]) == 1650
    # the sweep goes from all noise to one cluster
    X, _, min_samples = DC.case(DC.SWEEP_CASE)
    radii = DC.sweep_radii(8)
    first = DC.restate(DC.within(X, radii[0])[0], min_samples)
    last = DC.restate(DC.within(X, radii[-1])[0], min_samples)
    assert first["n_noise"] == len(X) and last["n_clusters"] == 1 and last["n_noise"] == 0


# ---- argument checks that need no device -----------------------------------------------------------------------------
def test_checks_run_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(DB, "_device", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    X = DC.case("n63_d31")[0]
    holes = np.arange(X.size).reshape(X.shape) == 7
    for eps in (0, 0.0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="'eps' parameter"):
            DB.DBSCAN(eps=eps).fit(X)
        with pytest.raises(ValueError, match="'eps' parameter"):
            DB.neighbor_counts(X, eps) if not isinstance(eps, str) and eps is not None else DB.DBSCAN(eps).fit_predict(X)
        with pytest.raises(ValueError, match="'eps' parameter"):
            DB.dbscan_sweep(X, [1.0, eps])
    for min_samples in (0, -3, 2.5, 5.0, "4", None, True):
        with pytest.raises(ValueError, match="'min_samples' parameter"):
            DB.DBSCAN(eps=1.0, min_samples=min_samples).fit(X)
        with pytest.raises(ValueError, match="'min_samples' parameter"):
            DB.dbscan_sweep(X, [1.0], min_samples=min_samples)
    for metric in ("cosine", "manhattan", None):
        with pytest.raises(NotImplementedError):
            DB.DBSCAN(eps=1.0, metric=metric).fit(X)
        with pytest.raises(NotImplementedError):
            DB.neighbor_counts(X, 1.0, metric=metric)
        with pytest.raises(NotImplementedError):
            DB.dbscan_sweep(X, [1.0], metric=metric)
    rows = [(X[:, 0], "Expected 2D array"), (np.where(holes, np.nan, X), "Input X contains NaN."),
            (np.where(holes, np.inf, X), "Input X contains infinity"),
            (torch.from_numpy(np.where(holes, np.nan, X)), "Input X contains NaN."),
            (np.zeros((0, 3)), "minimum of 1 is required")]
    for bad, message in rows:
        with pytest.raises(ValueError, match=message):
            DB.DBSCAN(eps=1.0).fit(bad)
        with pytest.raises(ValueError, match=message):
            DB.neighbor_counts(bad, 1.0)
        with pytest.raises(ValueError, match=message):
            DB.dbscan_sweep(bad, [1.0])
        with pytest.raises(ValueError, match=message):
            DB.k_distances(bad, 1)
    with pytest.raises(ValueError, match="square distance matrix"):
        DB.DBSCAN(eps=1.0, metric="precomputed").fit(X)
    for empty in ([], (), np.zeros(0)):
        with pytest.raises(ValueError, match="eps_list is empty"):
            DB.dbscan_sweep(X, empty)
    with pytest.raises(ValueError, match="sequence of radii"):
        DB.dbscan_sweep(X, 1.0)
    for k in (0, -1, 65, len(X) + 1, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            DB.k_distances(X, k)
    with pytest.raises(ValueError, match="at most %d" % DB.MAX_N):
        DB.DBSCAN(eps=1.0).fit(np.zeros((DB.MAX_N + 1, 1), dtype=np.float32))


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X = DC.case("n63_d31")[0]
    with pytest.raises(_lib.AvaHipError):
        DB.DBSCAN(eps=1.0).fit(X)
    with pytest.raises(_lib.AvaHipError):
        DB.DBSCAN(eps=1.0).fit_predict(X)
    with pytest.raises(_lib.AvaHipError):
        DB.neighbor_counts(X, [1.0, 2.0])
    with pytest.raises(_lib.AvaHipError):
        DB.dbscan_sweep(X, [1.0, 2.0], scores=True)
    with pytest.raises(_lib.AvaHipError):
        DB.k_distances(X, 4)


def test_constructor_keeps_its_parameters():
    m = DB.DBSCAN()
    assert (m.eps, m.min_samples, m.metric) == (0.5, 5, 'euclidean')
    m = DB.DBSCAN(0.25, min_samples=3, metric='precomputed')
    assert (m.eps, m.min_samples, m.metric) == (0.25, 3, 'precomputed')
    with pytest.raises(TypeError):
        DB.DBSCAN(0.5, 3)                                                 # keyword-only, as sklearn's


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def up256(x):
    return (x + 255) // 256 * 256


def test_library_argument_checks():
    """ava_db_* return sizes / AVA_EINVAL / AVA_EWORKSPACE before any HIP call (the test runs without a device, where a
    HIP call would return AVA_ELAUNCH instead)"""
    lib = _lib.load()
    assert lib.ava_db_max_eps() == DB.MAX_EPS == 8
    for n, d, e in ((0, 4, 1), (-1, 4, 1), (10, 0, 1), (10, 65537, 1), (10, 4, 0), (10, 4, 9), (DB.MAX_N + 1, 4, 1)):
        assert lib.ava_db_workspace_bytes(n, d, e) == 0, (n, d, e)
    for n, d, e in ((1, 1, 1), (5000, 33, 7), (2048, 16, 2), (2049, 65536, 8), (DB.MAX_N, 1, 8)):
        chunks = -(-n // 2048)
        assert lib.ava_db_workspace_bytes(n, d, e) == 4 * up256(4 * e * n) + up256(4 * e * chunks) + 256
    buf = np.zeros(256, dtype=np.float64)
    p = buf.ctypes.data
    eps = np.asarray([0.5, 1.0], dtype=np.float64)
    q = eps.ctypes.data
    big = 1 << 30

    def refuses(fn, ok, bad_args, eps_at):
        for i, bad in bad_args:
            a = list(ok)
            a[i] = bad
            assert fn(*a, None) == -1, (fn.__name__, i, bad)
        for bad in (0.0, -1.0, float("nan"), float("inf")) + (() if "pre" in fn.__name__ else (1e200,)):   # eps^2 = inf
            radii = np.asarray([0.5, bad], dtype=np.float64)
            a = list(ok)
            a[eps_at] = radii.ctypes.data
            assert fn(*a, None) == -1, (fn.__name__, bad)

    # x, dtype, n, d, eps, n_eps, counts
    refuses(lib.ava_db_counts, [p, 1, 8, 2, q, 2, p],
            ((0, None), (1, 2), (1, -1), (2, 0), (2, DB.MAX_N + 1), (3, 0), (3, 65537), (4, None), (5, 0), (5, 9),
             (6, None)), 4)
    tail = [p, p, p, p, big]                                              # core, labels, n_clusters, ws, ws_bytes
    for fn in (lib.ava_db_labels, lib.ava_db_assign):
        ok = [p, 1, 8, 2, q, 2, 3, p] + tail
        refuses(fn, ok, ((0, None), (1, 2), (2, 0), (3, 0), (4, None), (5, 0), (5, 9), (6, 0), (6, -1), (7, None),
                         (8, None), (9, None), (10, None), (11, None)), 4)
        assert fn(*(ok[:12] + [8]), None) == -3
    ok = [p, 1, 8, 2, q, 2, 3, p, p, big]
    refuses(lib.ava_db_union, ok, ((0, None), (1, 2), (2, 0), (3, 0), (4, None), (5, 9), (6, 0), (7, None), (8, None)), 4)
    assert lib.ava_db_union(*(ok[:9] + [8]), None) == -3
    # the precomputed forms: dist, dtype, n, eps, n_eps, ...
    refuses(lib.ava_db_counts_pre, [p, 1, 8, q, 2, p], ((0, None), (1, 3), (2, 0), (3, None), (4, 0), (4, 9), (5, None)),
            3)
    for fn in (lib.ava_db_labels_pre, lib.ava_db_assign_pre):
        ok = [p, 1, 8, q, 2, 3, p] + tail
        refuses(fn, ok, ((0, None), (1, 2), (2, 0), (3, None), (4, 9), (5, 0), (6, None), (7, None), (8, None),
                         (9, None), (10, None)), 3)
        assert fn(*(ok[:11] + [8]), None) == -3
    ok = [p, 1, 8, q, 2, 3, p, p, big]
    refuses(lib.ava_db_union_pre, ok, ((0, None), (1, 2), (2, 0), (3, None), (4, 9), (5, 0), (6, None), (7, None)), 3)
    assert lib.ava_db_union_pre(*(ok[:8] + [8]), None) == -3
