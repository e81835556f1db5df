"""ava_amd.cluster_metrics without a GPU: the numpy restatement of tests/silhouette_cases.py against scikit-learn's own
values (tests/golden/cluster_metrics.npz), the conditioning of the golden cases, the argument checks that need no
device, the ``sample_size`` draw and the C ABI's mirror and refusals.

Bounds: the golden file stores, per case and quantity, the reference-side noise ``floor`` (the larger of |sklearn -
restatement| where the file was written and |sklearn - sklearn on the rows in reversed order|, relative to
max |sklearn|).  The restatement is held within 4 x that floor plus the rounding bound derived in silhouette_cases.py,
relative to the largest wanted value."""

import numpy as np
import pytest
import torch

import silhouette_cases as SC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import cluster_metrics as CM
from ava_amd import mixture as M


@pytest.fixture(scope="module")
def golden():
    return load_golden("cluster_metrics.npz")


def close(got, want, bound, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: max err %.2e, bound %.2e" % (what, err, bound * scale))
    assert np.isfinite(got).all() and err <= bound * scale, what


def s_bound(d, labels):
    """the absolute bound of a silhouette coefficient from the relative bound of the sums (silhouette_cases.py)"""
    return 3.0 * (SC.sums_bound(d, labels) + SC.U) + 2.0 * SC.U


# ---- the restatement against sklearn ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.GOLDEN_CASES)
def test_restatement_against_sklearn(golden, name):
    X, labels = SC.case(name)
    mine = SC.silhouette(name)
    sb = s_bound(X.shape[1], labels)
    cb = SC.centroid_bound(X, labels)
    close(mine["s"], golden[name + "_s"], 4 * golden[name + "_floor_s"] + sb, "s")
    close(mine["score"], golden[name + "_score"], 4 * golden[name + "_floor_score"] + sb + len(X) * SC.U, "score")
    close(SC.calinski_harabasz(X, labels), golden[name + "_ch"], 4 * golden[name + "_floor_ch"] + cb, "ch")
    close(SC.davies_bouldin(X, labels), golden[name + "_db"], 4 * golden[name + "_floor_db"] + cb, "db")


def test_golden_cases_are_well_conditioned():
    """no row of a golden case has a = b = 0 or sits within 1e-4 of the largest distance of a row of another cluster
    (sklearn's Gram form leaves about sqrt(eps) |x| = 1.5e-8 |x| of noise in a small distance, which turns 0 / 0 into
    +-1), max(a, b) is far from 0, and the centroid scores' condition is moderate"""
    for name in SC.GOLDEN_CASES:
        X, labels = SC.case(name)
        r = SC.silhouette(name)
        enc = SC.encode(labels)[0]
        assert np.nanmin(np.fmax(r["a"], r["b"])) > 1e-2 * r["D"].max(), name
        other = enc[:, None] != enc[None, :]
        assert r["D"][other].min() > 1e-4 * r["D"].max(), name
        assert SC.centroid_condition(X, labels) < 100.0, name
    assert not set(SC.GOLDEN_CASES) & set(SC.SPECIAL)


def test_restatement_special_rows():
    """duplicate rows in different clusters: a = b = 0 gives s = 0; a cluster of identical rows: a = 0, s = 1; a
    cluster of one row: a is NaN, s = 0"""
    X, labels = SC.case("duplicates")
    r = SC.silhouette("duplicates")
    assert np.all(r["a"][:10] == 0.0) and np.all(r["b"][:10] == 0.0) and np.all(r["s"][:10] == 0.0)
    assert np.all(r["s"][10:] > 0.0)
    r = SC.silhouette("identical")
    assert np.all(r["a"][:7] == 0.0) and np.all(r["s"][:7] == 1.0)
    X, labels = SC.case("sizes_1_2_65")
    r = SC.silhouette("sizes_1_2_65")
    assert np.isnan(r["a"][10]) and r["s"][10] == 0.0 and np.isfinite(np.delete(r["a"], 10)).all()


# ---- argument checks that need no device -----------------------------------------------------------------------------
def test_checks_run_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(CM, "_device", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    X, labels = SC.case("n63_k3")
    n = len(X)
    holes = np.arange(n * 5).reshape(n, 5) == 7
    cases = [
        (X[:, 0], labels, "Expected 2D array"),
        (np.where(holes, np.nan, X), labels, "Input X contains NaN."),
        (np.where(holes, np.inf, X), labels, "Input X contains infinity"),
        (X, labels[:-1], r"inconsistent numbers of samples: \[63, 62\]"),
        (X, np.zeros(n, dtype=int), "Number of labels is 1. Valid values are 2 to n_samples - 1"),
        (X, np.arange(n), "Number of labels is 63. Valid values are 2 to n_samples - 1"),
        (X, labels.astype(np.float64), "labels must be integers or strings"),
    ]
    for fn in (CM.silhouette_samples, CM.silhouette_score, CM.calinski_harabasz_score, CM.davies_bouldin_score,
               CM.cluster_sums):
        for rows, lab, message in cases:
            with pytest.raises(ValueError, match=message):
                fn(rows, lab)
        with pytest.raises(ValueError, match="Input X contains NaN."):
            fn(torch.from_numpy(np.where(holes, np.nan, X)), labels)
    for fn in (CM.silhouette_samples, CM.silhouette_score):
        with pytest.raises(NotImplementedError):
            fn(X, labels, metric="cosine")
        with pytest.raises(ValueError, match="square distance matrix"):
            fn(X, labels, metric="precomputed")
        D = np.array(SC.silhouette("n63_k3")["D"])
        D[5, 5] = 1e-13                                                  # sklearn's tolerance: 100 eps of the dtype
        with pytest.raises(ValueError, match="non-zero elements on the diagonal. Use np.fill_diagonal"):
            fn(D, labels, metric="precomputed")
        D32 = D.astype(np.float32)
        D32[5, 5] = 2e-5
        with pytest.raises(ValueError, match="non-zero elements on the diagonal"):
            fn(torch.from_numpy(D32), labels, metric="precomputed")
    with pytest.raises(ValueError, match="at most %d" % CM.MAX_K):
        CM.silhouette_samples(np.zeros((CM.MAX_K + 2, 1)), np.arange(CM.MAX_K + 2) % (CM.MAX_K + 1))
    with pytest.raises(ValueError, match="centroid scores hold at most"):
        CM.calinski_harabasz_score(np.zeros((200, 2)), np.arange(200) % (M.MAX_K + 1))
    with pytest.raises(ValueError, match="centroid scores hold at most"):
        CM.davies_bouldin_score(np.zeros((20, M.MAX_D + 1)), np.arange(20) % 2)
    with pytest.raises(ValueError, match="sample_size"):
        CM.silhouette_score(X, labels, sample_size=0)
    with pytest.raises(ValueError, match="criteria"):
        CM.select_n_components(X, [2, 3], criteria=("bic", "banana"))
    with pytest.raises(ValueError):
        CM.select_n_components(X, [2, M.MAX_K + 1])
    with pytest.raises(NotImplementedError):
        CM.select_n_components(X, [2], covariance_type="tied")


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X, labels = SC.case("n63_k3")
    for fn in (CM.silhouette_samples, CM.silhouette_score, CM.calinski_harabasz_score, CM.davies_bouldin_score,
               CM.cluster_sums):
        with pytest.raises(_lib.AvaHipError):
            fn(X, labels)
    with pytest.raises(_lib.AvaHipError):
        CM.select_n_components(X, [2, 3])


def test_sample_size_draw_equals_sklearns():
    from sklearn.utils import check_random_state
    for n, size, seed in ((100, 30, 0), (2119, 500, 42), (64, 64, 7), (10, 20, 3)):
        want = check_random_state(seed).permutation(n)[:size]
        np.testing.assert_array_equal(CM._subsample_indices(n, size, seed), want)
    rs, rs2 = np.random.RandomState(5), np.random.RandomState(5)
    np.testing.assert_array_equal(CM._subsample_indices(50, 10, rs), check_random_state(rs2).permutation(50)[:10])
    np.random.seed(11)
    got = CM._subsample_indices(50, 10, None)
    np.random.seed(11)
    np.testing.assert_array_equal(got, check_random_state(None).permutation(50)[:10])


def test_tables():
    enc, k = CM._encode(np.array(["b", "a", "c", "a", "b", "a"]), 6)
    np.testing.assert_array_equal(enc, [1, 0, 2, 0, 1, 0])
    order, off = CM._tables(enc, k)
    np.testing.assert_array_equal(order, [1, 3, 5, 0, 4, 2])              # stable
    np.testing.assert_array_equal(off, [0, 3, 5, 6])
    assert order.dtype == off.dtype == enc.dtype == np.int64
    for name in SC.CASES:
        labels = SC.case(name)[1]
        np.testing.assert_array_equal(CM._encode(labels, len(labels))[0], SC.encode(labels)[0])


def test_host_formulas_from_exact_sums():
    """the two formulas evaluated on the host, fed the restatement's sums, give the restatement's scores"""
    for name in SC.GOLDEN_CASES:
        X, labels = SC.case(name)
        sizes, means, sum_dist, sum_sq = (np.asarray(a, dtype=np.float64) for a in SC.centroid_stats(X, labels))
        np.testing.assert_allclose(CM._ch_from_stats(sizes, means, sum_sq), SC.calinski_harabasz(X, labels),
                                   rtol=SC.centroid_bound(X, labels))
        np.testing.assert_allclose(CM._db_from_stats(sizes, means, sum_dist), SC.davies_bouldin(X, labels),
                                   rtol=SC.centroid_bound(X, labels))
    assert CM._ch_from_stats(np.array([2.0, 2.0]), np.array([[0.0], [1.0]]), np.zeros(2)) == 1.0
    assert CM._db_from_stats(np.array([2.0, 2.0]), np.array([[0.0], [1.0]]), np.zeros(2)) == 0.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def up256(x):
    return (x + 255) // 256 * 256


def test_library_argument_checks():
    """ava_sil_* return sizes / AVA_EINVAL / AVA_EWORKSPACE before any HIP call"""
    lib = _lib.load()
    assert (lib.ava_sil_max_k(), lib.ava_sil_chunk_cols()) == (CM.MAX_K, CM.CHUNK_COLS) == (1024, SC.CHUNK)
    for n, d, k in ((10, 0, 2), (10, 4, 1), (10, 4, 10), (2000, 4, 1025), (3, 4, 3), (-1, 4, 2), ((1 << 30) + 1, 1, 2)):
        assert lib.ava_sil_workspace_bytes(n, d, k) == 0
    for n, d, k in ((3, 1, 2), (5000, 33, 7), (2048, 16, 2), (2049, 300, 1024)):
        chunks = -(-n // 2048)
        assert lib.ava_sil_workspace_bytes(n, d, k) == up256(n * d * 8) + up256(chunks * 8) + up256(chunks * k * 16) + 256
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    big = 1 << 30
    s_ok = [p, 1, 8, 2, 2, p, p, p, p, big]
    for i, bad in ((0, None), (1, 2), (1, -1), (2, 2), (3, 0), (4, 1), (4, 8), (4, 1025), (5, None), (6, None),
                   (7, None), (8, None)):
        a = list(s_ok)
        a[i] = bad
        assert lib.ava_sil_cluster_sums(*a, None) == -1, (i, bad)
    assert lib.ava_sil_cluster_sums(*(s_ok[:9] + [8]), None) == -3
    p_ok = [p, 1, 8, 2, p, p, p]
    for i, bad in ((0, None), (1, 3), (2, 2), (3, 1), (3, 8), (4, None), (5, None), (6, None)):
        a = list(p_ok)
        a[i] = bad
        assert lib.ava_sil_cluster_sums_pre(*a, None) == -1, (i, bad)
    f_ok = [p, 8, 2, p, p, p, p, p, p, p, big]
    for i, bad in ((0, None), (1, 2), (2, 1), (2, 8), (3, None), (4, None), (5, None), (6, None), (7, None), (8, None),
                   (9, None)):
        a = list(f_ok)
        a[i] = bad
        assert lib.ava_sil_finish(*a, None) == -1, (i, bad)
    assert lib.ava_sil_finish(*(f_ok[:10] + [8]), None) == -3
    c_ok = [p, 1, 200, 2, 2, p, p, p, p, p, big]
    for i, bad in ((0, None), (1, 2), (2, 2), (3, 0), (3, M.MAX_D + 1), (4, 1), (4, M.MAX_K + 1), (5, None), (6, None),
                   (7, None), (8, None), (9, None)):
        a = list(c_ok)
        a[i] = bad
        assert lib.ava_sil_centroid_stats(*a, None) == -1, (i, bad)
    assert lib.ava_sil_centroid_stats(*(c_ok[:10] + [8]), None) == -3
