"""ava_amd.kmeans without a GPU: the restatement of tests/kmeans_cases.py against scikit-learn's own KMeans and
kmeans_plusplus, the margin of every golden case to the model's discontinuous rules, the content of
tests/golden/kmeans.npz, the argument checks that need no device and the C ABI's refusals.

Label and index comparisons are exact on every row; floats are held to max(1e-11, 4 x floor) with the floors of
make_golden_kmeans.py (the reference's own noise)."""
import warnings

import numpy as np
import pytest
import torch

import kmeans_cases as KC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import kmeans as KM

MARGIN = 1e-9


@pytest.fixture(scope="module")
def golden():
    return load_golden("kmeans.npz")


_RUNS = {}


def restated(name):
    """the restatement's fit of a golden case and its trace, computed once"""
    if name not in _RUNS:
        X, kw = KC.fit_case(name)
        kw = dict(kw)
        trace = {}
        _RUNS[name] = (KC.fit(X, kw.pop('n_clusters'), trace=trace, **kw), trace)
    return _RUNS[name]


def close(got, want, floor):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() <= max(1e-11, 4.0 * float(floor)) * np.abs(want).max()


# ---- the restatement, the margins, the golden file -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KC.FIT_CASES))
def test_restatement_is_sklearns(golden, name):
    """labels equal on every row, n_iter equal, centres and inertia within max(1e-11, 4 floors) of the golden file, which
    holds what sklearn gives now"""
    from sklearn.cluster import KMeans
    X, kw = KC.fit_case(name)
    mine, _ = restated(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = KMeans(algorithm='lloyd', **kw).fit(X)
    assert np.array_equal(sk.labels_, golden[name + "/labels"]) and sk.n_iter_ == golden[name + "/n_iter"]
    # sklearn's own floats move in the last bits from run to run (its sums are split over threads)
    assert close(sk.cluster_centers_, golden[name + "/centres"], golden[name + "/floor_centres"])
    assert close(sk.inertia_, golden[name + "/inertia"], golden[name + "/floor_inertia"])
    assert mine["labels"].dtype == np.int32 and np.array_equal(mine["labels"], golden[name + "/labels"])
    assert mine["n_iter"] == golden[name + "/n_iter"]
    assert close(mine["centres"], golden[name + "/centres"], golden[name + "/floor_centres"])
    assert close(mine["inertia"], golden[name + "/inertia"], golden[name + "/floor_inertia"])


@pytest.mark.parametrize("name", sorted(KC.FIT_CASES))
def test_plusplus_indices_are_sklearns(golden, name):
    from sklearn.cluster import kmeans_plusplus
    X, kw = KC.fit_case(name)
    seed = kw.get('random_state', 0)
    trace = {}
    mine = KC.plusplus(X, kw['n_clusters'], np.random.RandomState(seed), trace)
    assert np.array_equal(mine, golden[name + "/pp"])
    assert np.array_equal(kmeans_plusplus(X, kw['n_clusters'], random_state=seed)[1], golden[name + "/pp"])
    assert trace.get('search', np.inf) > MARGIN and trace.get('potential', np.inf) > MARGIN, trace


@pytest.mark.parametrize("name", sorted(KC.FIT_CASES))
def test_cases_are_away_from_the_discontinuous_rules(name):
    """the best and second-best centre of every row at every iteration, every searchsorted threshold and its neighbouring
    scan entries, the candidates' potentials, and shift against the tolerance: each more than 1e-9 relative apart"""
    _, trace = restated(name)
    X, kw = KC.fit_case(name)
    if kw['n_clusters'] > 1:
        assert 'assign' in trace
    if isinstance(kw.get('init', 'k-means++'), str) and kw.get('init', 'k-means++') == 'k-means++':
        assert 'search' in trace
    for key, value in trace.items():
        assert value > MARGIN, (key, value)


def test_empty_three_case_has_three_empty_clusters_and_ties():
    X, init = KC.empty_three_case()
    labels, d2 = KC.assign(X, init)
    counts = np.bincount(labels, minlength=len(init))
    assert list(np.flatnonzero(counts == 0)) == [2, 3, 4]
    top = np.sort(d2)[::-1]
    assert top[0] == top[1] == top[2] == top[3]                    # the farthest distance is shared by four rows
    sums, cnt = KC.cluster_sums(X, labels, len(init))
    KC.relocate(X, sums, cnt, labels, d2)
    far = np.flatnonzero(d2 == top[0])[:3]                         # the lowest rows of the tie, in ascending order
    assert np.array_equal(sums[2:], X[far]) and list(cnt[2:]) == [1, 1, 1]


def test_chunk_orders():
    v = np.random.RandomState(0).standard_normal(5000) ** 2
    scan = KC.chunk_scan(v)
    assert scan[2047] == np.cumsum(v[:2048])[-1] and scan[2048] == scan[2047] + v[2048]
    assert scan[-1] == KC.chunk_sum(v) and np.all(np.diff(scan) >= 0)
    assert abs(scan[-1] - v.sum()) <= 1e-12 * v.sum()


# ---- argument checks that need no device -----------------------------------------------------------------------------
def test_checks_run_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(KM, "_device", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    X = KC.blobs(50, 4, 3, 3.0, 0)
    holes = np.arange(X.size).reshape(X.shape) == 7
    for k in (0, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="'n_clusters' parameter of KMeans must be an int in the range"):
            KM.KMeans(k).fit(X)
        with pytest.raises(ValueError, match="'n_clusters' parameter"):
            KM.kmeans_sweep(X, [2, k])
        with pytest.raises(ValueError, match="'n_clusters' parameter"):
            KM.kmeans_plusplus(X, k)
    with pytest.raises(ValueError, match="at most 256 clusters"):
        KM.KMeans(257).fit(np.zeros((300, 2)))
    with pytest.raises(ValueError, match="d = 129 features, at most 128"):
        KM.KMeans(2).fit(np.zeros((10, 129)))
    with pytest.raises(ValueError, match=r"n_samples=50 should be >= n_clusters=51\."):
        KM.KMeans(51).fit(X)
    with pytest.raises(ValueError, match=r"n_samples=50 should be >= n_clusters=51\."):
        KM.kmeans_plusplus(X, 51)
    for bad, message in [(dict(n_init=0), "'n_init' parameter"), (dict(n_init="many"), "'n_init' parameter"),
                         (dict(max_iter=0), "'max_iter' parameter"), (dict(max_iter=2.5), "'max_iter' parameter"),
                         (dict(tol=-1e-3), "'tol' parameter"), (dict(tol="small"), "'tol' parameter"),
                         (dict(tol=float("nan")), "'tol' parameter"), (dict(iter_block=0), "'iter_block' parameter"),
                         (dict(init="kmeans"), "'init' parameter"), (dict(algorithm="full"), "'algorithm' parameter"),
                         (dict(random_state="seed"), "cannot be used to seed"),
                         (dict(init=np.zeros((2, 4))), "does not match the number of clusters 3"),
                         (dict(init=np.zeros((3, 5))), "does not match the number of features of the data 4"),
                         (dict(init=np.full((3, 4), np.nan)), "Input init contains NaN or infinity")]:
        with pytest.raises(ValueError, match=message):
            KM.KMeans(3, **bad).fit(X)
    with pytest.raises(NotImplementedError, match="elkan"):
        KM.KMeans(3, algorithm='elkan').fit(X)
    with pytest.raises(NotImplementedError, match="sample_weight"):
        KM.KMeans(3).fit(X, sample_weight=np.ones(50))
    with pytest.raises(NotImplementedError, match="callable"):
        KM.KMeans(3, init=lambda X, k, rs: X[:k]).fit(X)

    class Sparse:
        shape = (50, 4)

        def tocsr(self):
            return self
    with pytest.raises(NotImplementedError, match="sparse"):
        KM.KMeans(3).fit(Sparse())
    rows = [(X[:, 0], "Expected 2D array"), (np.where(holes, np.nan, X), "Input X contains NaN."),
            (np.where(holes, np.inf, X), "Input X contains infinity"),
            (torch.from_numpy(np.where(holes, np.nan, X)), "Input X contains NaN."),
            (np.zeros((0, 3)), "minimum of 1 is required")]
    for bad, message in rows:
        with pytest.raises(ValueError, match=message):
            KM.KMeans(3).fit(bad)
        with pytest.raises(ValueError, match=message):
            KM.assign(bad, np.zeros((3, 4)))
        with pytest.raises(ValueError, match=message):
            KM.kmeans_sweep(bad, [2, 3])
    with pytest.raises(ValueError, match="centres has 5 features, the rows have 4"):
        KM.assign(X, np.zeros((3, 5)))
    with pytest.raises(ValueError, match=r"labels must be \[N\] integers"):
        KM.update(X, np.zeros(49, dtype=np.int64), 3)
    with pytest.raises(ValueError, match=r"labels must be \[N\] integers"):
        KM.update(X, np.zeros(50), 3)
    with pytest.raises(ValueError, match="non-empty sequence"):
        KM.kmeans_sweep(X, [])
    for call in (lambda m: m.predict(X), lambda m: m.transform(X), lambda m: m.score(X)):
        with pytest.raises(ValueError, match="not fitted yet"):
            call(KM.KMeans(3))
    with pytest.warns(RuntimeWarning, match="performing only one init"):
        with pytest.raises(AssertionError, match="the device was touched"):
            KM.KMeans(3, init=X[:3], n_init=4).fit(X)
    with pytest.raises(AssertionError, match="the device was touched"):        # everything checked: the device is next
        KM.KMeans(3).fit(X)


def test_types_and_defaults():
    m = KM.KMeans()
    assert (m.n_clusters, m.init, m.n_init, m.max_iter, m.tol, m.algorithm, m.iter_block) == (
        8, 'k-means++', 'auto', 300, 1e-4, 'lloyd', 16)
    assert KM.KMeans(3)._check_params()[3] == 1 and KM.KMeans(3, init='random')._check_params()[3] == 10
    assert KM.KMeans(3, init=np.zeros((3, 2)))._check_params()[3] == 1
    assert issubclass(KM.KMeansConvergenceWarning, UserWarning)
    assert (KM.MAX_D, KM.MAX_K, KM.CHUNK_ROWS) == (128, 256, KC.CHUNK)
    assert KM._n_trials(2) == 2 and KM._n_trials(256) == 7 and KC.n_trials(256) == 7
    a = np.array([0, 0, 1, 2]); b = np.array([2, 2, 0, 1]); c = np.array([0, 1, 1, 2])
    assert KM._is_same_clustering(a, b, 3) and not KM._is_same_clustering(a, c, 3)
    assert KC.same_clustering(a, b, 3) and not KC.same_clustering(a, c, 3)


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.AvaHipError, match="k-means kernels only run on an MI355X"):
        KM.KMeans(2).fit(KC.blobs(20, 2, 2, 3.0, 0))


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_limits_and_refusals_without_a_launch():
    """the constants, the workspace sizes, and AVA_EINVAL / AVA_EWORKSPACE for bad arguments: every refusal comes before
    any HIP call, so it needs no device (the pointers are never dereferenced)"""
    lib = _lib.load()
    assert (lib.ava_km_max_d(), lib.ava_km_max_k(), lib.ava_km_chunk_rows()) == (KM.MAX_D, KM.MAX_K, KM.CHUNK_ROWS)
    for n, d, k in [(0, 4, 2), (10, 0, 2), (10, 129, 2), (10, 4, 0), (300, 4, 257), (-1, 4, 2), (2 ** 31 - 63, 4, 2)]:
        assert lib.ava_km_workspace_bytes(n, d, k) == 0, (n, d, k)
    small, big = lib.ava_km_workspace_bytes(100, 4, 3), lib.ava_km_workspace_bytes(5000, 128, 256)
    assert 0 < small < big and lib.ava_km_workspace_bytes(2 ** 31 - 64, 1, 1) > 0
    assert big >= 3 * 256 * 128 * 8                                   # three chunks of per-cluster sums
    p, EINVAL, EWS = 4096, -1, -3                                     # a non-null pointer that is never used
    assert lib.ava_km_assign(None, 1, 10, 4, 2, p, p, p, None, p, big, None) == EINVAL
    assert lib.ava_km_assign(p, 2, 10, 4, 2, p, p, p, None, p, big, None) == EINVAL
    assert lib.ava_km_assign(p, 1, 10, 129, 2, p, p, p, None, p, big, None) == EINVAL
    assert lib.ava_km_assign(p, 1, 10, 4, 257, p, p, p, None, p, big, None) == EINVAL
    assert lib.ava_km_assign(p, 1, 10, 4, 2, None, p, p, None, p, big, None) == EINVAL
    assert lib.ava_km_assign(p, 1, 10, 4, 2, p, None, p, None, p, big, None) == EINVAL
    assert lib.ava_km_assign(p, 1, 10, 4, 2, p, p, None, None, p, big, None) == EINVAL
    assert lib.ava_km_assign(p, 1, 10, 4, 2, p, p, p, None, None, big, None) == EINVAL
    assert lib.ava_km_assign(p, 1, 10, 4, 2, p, p, p, None, p, 16, None) == EWS
    assert lib.ava_km_update(p, 1, 10, 4, 2, None, p, p, p, big, None) == EINVAL
    assert lib.ava_km_update(p, 0, 10, 4, 2, p, p, p, p, 16, None) == EWS
    assert lib.ava_km_update(p, 0, 10, 4, 0, p, p, p, p, big, None) == EINVAL
    fit = lambda **kw: lib.ava_km_fit(*[kw.get(a, v) for a, v in [
        ("x", p), ("dtype", 1), ("n", 10), ("d", 4), ("k", 2), ("centres", p), ("labels", p), ("d2", p), ("tol", 1e-4),
        ("mean_var", p), ("it0", 0), ("n_iters", 1), ("ctl", p), ("shift", None), ("ws", p), ("ws_bytes", big),
        ("s", None)]])
    for bad in (dict(x=None), dict(dtype=-1), dict(n=0), dict(d=0), dict(k=11), dict(k=0), dict(centres=None),
                dict(labels=None), dict(d2=None), dict(tol=-1.0), dict(tol=float("nan")), dict(mean_var=None),
                dict(it0=-1), dict(n_iters=0), dict(ctl=None), dict(ws=None)):
        assert fit(**bad) == EINVAL, bad
    assert fit(ws_bytes=16) == EWS
    assert lib.ava_km_pp_start(p, 1, 10, 4, 10, p, None) == EINVAL and lib.ava_km_pp_start(p, 1, 10, 4, -1, p, None) == EINVAL
    assert lib.ava_km_pp_start(p, 1, 10, 4, 0, None, None) == EINVAL
    assert lib.ava_km_pp_step(p, 1, 10, 4, 0, p, p, p, p, p, big, None) == EINVAL
    assert lib.ava_km_pp_step(p, 1, 10, 4, 9, p, p, p, p, p, big, None) == EINVAL
    assert lib.ava_km_pp_step(p, 1, 10, 4, 2, None, p, p, p, p, big, None) == EINVAL
    assert lib.ava_km_pp_step(p, 1, 10, 4, 2, p, p, p, p, p, 16, None) == EWS
    assert lib.ava_km_variance(p, 1, 10, 4, None, p, big, None) == EINVAL
    assert lib.ava_km_variance(p, 3, 10, 4, p, p, big, None) == EINVAL
    assert lib.ava_km_variance(p, 1, 10, 4, p, p, 16, None) == EWS
    assert lib.ava_km_transform(p, 1, 10, 4, 2, p, None, None) == EINVAL
    assert lib.ava_km_transform(p, 1, 10, 200, 2, p, p, None) == EINVAL
    assert lib.ava_km_transform(None, 1, 10, 4, 2, p, p, None) == EINVAL
