"""The kernels of csrc/silhouette.hip and ava_amd.cluster_metrics on the MI355X: the cluster sums, a, b, s and the scores
against the longdouble restatement of tests/silhouette_cases.py at row-tile, column-tile, stage and chunk edges, the
runs that must not change a bit (float32 / float64 copies, relabelled clusters, other clusters resized), the special
rows, the precomputed metric, scikit-learn's own values (tests/golden/cluster_metrics.npz), the two centroid scores,
select_n_components and the error paths.  tests/test_cpu_cluster_metrics.py shows that the restatement is sklearn's
arithmetic and that the golden cases are well conditioned.

Bounds (derived in silhouette_cases.py; U = 2^-53): a sum S[i, k] is held, element by element, within
``C_SUMS (d + 2 + n_max) U`` relative of the restatement with ``C_SUMS = 2``; a and b one division further (+ U); s
within 3 (that + U) + 2 U absolute; the score n U more; the centroid scores within ``C_CENTROID (d + 2 + n_max) U``
relative with ``C_CENTROID = 4``.  Against sklearn every quantity is held within max(that bound, 4 x the stored
reference-side floor)."""
import numpy as np
import pytest
import torch

import silhouette_cases as SC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import cluster_metrics as CM
from ava_amd import mixture as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("cluster_metrics.npz")


def within_rel(got, want, bound, what):
    """element by element: |got - want| <= bound |want|, NaN where NaN is wanted"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.dtype == np.float64, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    worst = float((err / np.maximum(np.abs(want[ok]), np.finfo(float).tiny)).max()) if err.max() > 0 else 0.0
    print("%s: max rel err %.2e, bound %.2e" % (what, worst, bound))
    assert np.all(err <= bound * np.abs(want[ok])), what


def within_abs(got, want, bound, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.abs(got - want).max())
    print("%s: max abs err %.2e, bound %.2e" % (what, err, bound))
    assert np.isfinite(got).all() and err <= bound, what


def s_bound(eps):
    return 3.0 * (eps + SC.U) + 2.0 * SC.U


# ---- sums, a, b, s, score against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_silhouette_against_restatement(name):
    X, labels = SC.case(name)
    want = SC.silhouette(name)
    eps = SC.sums_bound(X.shape[1], labels)
    S = CM.cluster_sums(X, labels)
    within_rel(S, want["S"], eps, "S")
    s, a, b = CM.silhouette_samples(X, labels, return_parts=True)
    within_rel(a, want["a"], eps + SC.U, "a")
    within_rel(b, want["b"], eps + SC.U, "b")
    within_abs(s, want["s"], s_bound(eps), "s")
    score = CM.silhouette_score(X, labels)
    within_abs(score, want["score"], s_bound(eps) + len(X) * SC.U, "score")
    # float32 rows and their float64 copies, host arrays and device tensors: identical bits
    assert X.dtype == np.float32
    np.testing.assert_array_equal(CM.cluster_sums(X.astype(np.float64), labels), S)
    np.testing.assert_array_equal(CM.silhouette_samples(X.astype(np.float64), labels), s)
    np.testing.assert_array_equal(CM.silhouette_samples(torch.from_numpy(X).cuda(), labels), s)
    assert CM.silhouette_score(X.astype(np.float64), labels) == score
    np.testing.assert_array_equal(CM.silhouette_samples(X, labels), s)
    # a cluster of one row scores exactly 0
    enc = SC.encode(labels)[0]
    alone = np.bincount(enc)[enc] == 1
    assert np.all(s[alone] == 0.0) and np.all(np.isnan(a[alone]))
    assert alone.any() == (name == "sizes_1_2_65")


def test_special_rows():
    """duplicate rows in different clusters: a = b = 0 gives s = 0 exactly; a whole cluster of identical rows: a = 0
    and s = 1 exactly"""
    X, labels = SC.case("duplicates")
    s, a, b = CM.silhouette_samples(X, labels, return_parts=True)
    assert np.all(a[:10] == 0.0) and np.all(b[:10] == 0.0) and np.all(s[:10] == 0.0)
    assert np.all(s[10:] > 0.0)
    X, labels = SC.case("identical")
    s, a, b = CM.silhouette_samples(X, labels, return_parts=True)
    assert np.all(a[:7] == 0.0) and np.all(s[:7] == 1.0)


# ---- runs that change no bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n129_k3", "k64_n200", "chunk2049"])
def test_relabelled_clusters_give_identical_bits(name):
    """other label values, in another order (the clusters swap places in the sorted order): the same s, a, b per row"""
    X, labels = SC.case(name)
    base = CM.silhouette_samples(X, labels, return_parts=True)
    enc, k = SC.encode(labels)
    reverse = (1000 - 7 * enc).astype(np.int64)                          # descending: the sorted order is reversed
    rotate = np.asarray(["c%04d" % ((j + k // 2) % k) for j in range(k)])[enc]
    for other in (reverse, rotate):
        got = CM.silhouette_samples(X, other, return_parts=True)
        for g, w in zip(got, base):
            np.testing.assert_array_equal(g, w)
    S, R = CM.cluster_sums(X, labels), CM.cluster_sums(X, reverse)
    np.testing.assert_array_equal(R[:, ::-1], S)


@pytest.mark.parametrize("name", ["chunk2049", "n129_k3"])
def test_sums_of_an_untouched_cluster_do_not_depend_on_the_others(name):
    """the order contract: rows of the other clusters removed (so that the kept cluster moves in the sorted order, its
    rows fall into other tiles and N changes): S[:, k] of the kept cluster keeps its bits on every remaining row"""
    X, labels = SC.case(name)
    enc, k = SC.encode(labels)
    kept = int(np.argmax(np.bincount(enc)))
    first = (enc - kept - 1) % k + 1                                     # the kept cluster sorts last
    S = CM.cluster_sums(X, first)
    assert np.all(first[enc == kept] == k)
    for drop in (5, 37):
        others = np.flatnonzero(enc != kept)
        keep = np.setdiff1d(np.arange(len(X)), others[1:1 + drop])
        got = CM.cluster_sums(X[keep], first[keep])
        np.testing.assert_array_equal(got[:, -1], S[keep, -1])


# ---- the precomputed metric --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n65_k3", "sizes_1_2_65", "chunk2049"])
def test_precomputed(name):
    X, labels = SC.case(name)
    want = SC.silhouette(name)
    d = X.shape[1]
    eps = SC.sums_bound(d, labels)
    D = np.array(want["D"])
    S = CM.cluster_sums(D, labels, metric="precomputed")
    within_rel(S, want["S"], eps, "S from float64 distances")
    s, a, b = CM.silhouette_samples(D, labels, metric="precomputed", return_parts=True)
    within_rel(a, want["a"], eps + SC.U, "a")
    within_rel(b, want["b"], eps + SC.U, "b")
    within_abs(s, want["s"], s_bound(eps), "s")
    within_abs(CM.silhouette_score(D, labels, metric="precomputed"), want["score"], s_bound(eps) + len(X) * SC.U, "score")
    np.testing.assert_array_equal(CM.silhouette_samples(torch.from_numpy(D).cuda(), labels, metric="precomputed"), s)
    # a float32 matrix: the sums of its own (rounded) entries
    D32 = D.astype(np.float32)
    want32 = np.asarray(SC.sums_from_distances(D32, labels), dtype=np.float64)
    within_rel(CM.cluster_sums(D32, labels, metric="precomputed"), want32, eps, "S from float32 distances")
    s32 = CM.silhouette_samples(D32, labels, metric="precomputed")
    within_abs(s32, SC.finish(want32, labels)[0], s_bound(eps), "s from float32 distances")
    # a non-zero diagonal raises, on the host and on the device
    D[3, 3] = 1e-9
    for bad in (D, torch.from_numpy(D).cuda()):
        with pytest.raises(ValueError, match="non-zero elements on the diagonal"):
            CM.silhouette_samples(bad, labels, metric="precomputed")


def test_sample_size_subsamples_as_sklearn():
    from sklearn.utils import check_random_state
    X, labels = SC.case("n129_k3")
    idx = check_random_state(4).permutation(129)[:80]
    want = CM.silhouette_score(X[idx], labels[idx])
    assert CM.silhouette_score(X, labels, sample_size=80, random_state=4) == want
    assert CM.silhouette_score(torch.from_numpy(X).cuda(), labels, sample_size=80, random_state=4) == want
    D = np.array(SC.silhouette("n129_k3")["D"])
    want = CM.silhouette_score(D[idx][:, idx], labels[idx], metric="precomputed")
    assert CM.silhouette_score(D, labels, metric="precomputed", sample_size=80, random_state=4) == want
    sub = SC.finish(SC.sums_from_distances(D[idx][:, idx], labels[idx]), labels[idx])[0]
    within_abs(want, float(sub.mean()), s_bound(SC.sums_bound(5, labels[idx])) + 80 * SC.U, "subsampled score")


# ---- sklearn's own values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.GOLDEN_CASES)
def test_against_sklearn(golden, name):
    X, labels = SC.case(name)
    eps = SC.sums_bound(X.shape[1], labels)

    def floor(q):
        return 4.0 * float(golden["%s_floor_%s" % (name, q)])

    s = CM.silhouette_samples(X, labels)
    scale = np.abs(golden[name + "_s"]).max()
    within_abs(s, golden[name + "_s"], max(s_bound(eps), floor("s") * scale), "s")
    want = float(golden[name + "_score"])
    within_abs(CM.silhouette_score(X, labels), want, max(s_bound(eps) + len(X) * SC.U, floor("score") * abs(want)),
               "score")
    cb = SC.centroid_bound(X, labels)
    within_rel(CM.calinski_harabasz_score(X, labels), golden[name + "_ch"], max(cb, floor("ch")), "ch")
    within_rel(CM.davies_bouldin_score(X, labels), golden[name + "_db"], max(cb, floor("db")), "db")


# ---- the centroid scores -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.CENTROID_CASES)
def test_centroid_scores_against_restatement(name):
    X, labels = SC.case(name)
    cb = SC.centroid_bound(X, labels)
    ch, db = CM.calinski_harabasz_score(X, labels), CM.davies_bouldin_score(X, labels)
    assert isinstance(ch, float) and isinstance(db, float)
    within_rel(ch, SC.calinski_harabasz(X, labels), cb, "calinski_harabasz")
    within_rel(db, SC.davies_bouldin(X, labels), cb, "davies_bouldin")
    assert CM.calinski_harabasz_score(X.astype(np.float64), labels) == ch
    assert CM.davies_bouldin_score(torch.from_numpy(X).cuda(), labels) == db
    # the sums behind them
    sizes, means, sum_dist, sum_sq = CM._centroid_stats(X, labels)
    wsizes, wmeans, wdist, wsq = (np.asarray(a, dtype=np.float64) for a in SC.centroid_stats(X, labels))
    np.testing.assert_array_equal(sizes, wsizes)
    # every cluster's sums relative to themselves, plus the room the rounding of that cluster's mean gives them
    # (silhouette_cases.centroid_sum_terms: what keeps the sum of a cluster of one row, wanted 0, at a few ulp of |x|)
    term_dist, term_sq = SC.centroid_sum_terms(X, labels)
    for j in range(len(sizes)):
        within_abs(sum_dist[j], wdist[j], cb * wdist[j] + term_dist[j], "sum of distances, cluster %d" % j)
        within_abs(sum_sq[j], wsq[j], cb * wsq[j] + term_sq[j], "sum of squared distances, cluster %d" % j)
    # the cluster means are mixture.m_step's for one-hot responsibilities, bit for bit
    enc, k = SC.encode(labels)
    resp = np.zeros((len(X), k))
    resp[np.arange(len(X)), enc] = 1.0
    np.testing.assert_array_equal(means, M.m_step(X, resp, 1e-6, "diag")[1].cpu().numpy())


def test_centroid_scores_special_values():
    """identical rows within every cluster: Davies-Bouldin is 0.0 as sklearn defines it and every silhouette is 1.
    Calinski-Harabasz is sklearn's 1.0 only where the within-cluster sum is exactly 0.  Here it is not: mixture's means
    divide by n_k + 10 eps (5 + 2 ulp for these clusters of 5), so a coordinate 1 has the mean 1 - 3 ulp, the
    within-cluster sum is about 1e-30 and the score finite and huge (a documented deviation)"""
    X = np.repeat(np.array([[0.0, 1.0], [4.0, 1.0], [0.0, 9.0]], dtype=np.float32), 5, axis=0)
    labels = np.repeat([3, 1, 2], 5)
    ch = CM.calinski_harabasz_score(X, labels)
    assert np.isfinite(ch) and ch > 1e25
    sum_sq = CM._centroid_stats(X, labels)[3]
    assert np.all(sum_sq > 0.0) and np.all(sum_sq < 1e-27)
    assert CM.davies_bouldin_score(X, labels) == 0.0
    np.testing.assert_array_equal(CM.silhouette_samples(X, labels), 1.0)


# ---- select_n_components -----------------------------------------------------------------------------------------------
def test_select_n_components():
    X = SC.three_blobs()
    counts = [1, 2, 3, 4, 5]
    out = CM.select_n_components(X, counts, random_state=42)          # a start that finds the blobs (checked on the CPU)
    assert sorted(out) == sorted(["n_components", "labels", "bic", "aic", "silhouette", "calinski_harabasz",
                                  "davies_bouldin"])
    np.testing.assert_array_equal(out["n_components"], counts)
    assert out["labels"].shape == (5, 600) and out["labels"].dtype == np.int64
    assert counts[int(np.nanargmax(out["silhouette"]))] == 3
    # one component: a single cluster, the geometric scores are NaN, the likelihood criteria are not
    assert all(np.isnan(out[c][0]) for c in ("silhouette", "calinski_harabasz", "davies_bouldin"))
    assert np.isfinite(out["bic"]).all() and np.isfinite(out["aic"]).all()
    assert np.isfinite(out["silhouette"][1:]).all()
    # every row equals a separate fit and separate metric calls, bit for bit
    for i, c in enumerate(counts):
        g = M.GaussianMixture(c, random_state=42).fit(X)
        labels = g.predict(X)
        np.testing.assert_array_equal(out["labels"][i], labels)
        assert out["bic"][i] == g.bic(X) and out["aic"][i] == g.aic(X)
        if c > 1:
            assert out["silhouette"][i] == CM.silhouette_score(X, labels)
            assert out["calinski_harabasz"][i] == CM.calinski_harabasz_score(X, labels)
            assert out["davies_bouldin"][i] == CM.davies_bouldin_score(X, labels)
    # the three blobs are found: every blob is one cluster
    assert sorted(len(set(out["labels"][2][j::3])) for j in range(3)) == [1, 1, 1]
    some = CM.select_n_components(torch.from_numpy(X).cuda(), [3], covariance_type="diag", criteria=("silhouette",))
    assert sorted(some) == ["labels", "n_components", "silhouette"]
    assert some["silhouette"][0] == CM.silhouette_score(X, some["labels"][0])


# ---- error paths -------------------------------------------------------------------------------------------------------
def test_library_refusal_raises_and_the_device_stays_usable():
    lib = _lib.load()
    dev = torch.device("cuda")
    with pytest.raises(ValueError, match="unsupported shape"):
        CM._workspace(5000, 4, CM.MAX_K + 1, dev)                      # more labels than the library holds
    with pytest.raises(ValueError, match="at most %d" % CM.MAX_K):
        CM.silhouette_samples(np.zeros((CM.MAX_K + 2, 1)), np.arange(CM.MAX_K + 2) % (CM.MAX_K + 1))
    X = torch.zeros((8, 2), dtype=torch.float64, device=dev)
    idx = torch.zeros(16, dtype=torch.int64, device=dev)
    out = torch.full((64,), 7.0, dtype=torch.float64, device=dev)
    p, i, o, st = X.data_ptr(), idx.data_ptr(), out.data_ptr(), _lib.stream()
    assert lib.ava_sil_cluster_sums(p, 1, 8, 2, 8, i, i, o, o, 1 << 20, st) == -1                   # K > N - 1
    assert lib.ava_sil_cluster_sums(p, 1, 8, 2, 2, i, i, o, o, 8, st) == -3
    assert lib.ava_sil_cluster_sums_pre(p, 2, 8, 2, i, i, o, st) == -1
    assert lib.ava_sil_finish(o, 8, 1, i, i, o, o, o, o, o, 1 << 20, st) == -1
    assert lib.ava_sil_centroid_stats(p, 1, 8, 2, M.MAX_K + 1, i, o, o, o, o, 1 << 20, st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    X, labels = SC.case("n65_k3")                                       # the next call runs
    within_abs(CM.silhouette_samples(X, labels), SC.silhouette("n65_k3")["s"],
               s_bound(SC.sums_bound(5, labels)), "s after the refusals")
