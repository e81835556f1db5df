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


# ---- the edge cases of test_gpu_kmeans_edges.py: each decides what it claims ------------------------------------------
def _wanted_centres(X, labels, k):
    sums, counts = KC.cluster_sums(X, labels, k)
    return np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], 0.0), counts


@pytest.mark.parametrize("n,d,k", KC.EDGE_DISPATCH)
def test_edge_dispatch_cases_fill_every_cluster_in_every_chunk(n, d, k):
    """every cluster has rows; the clusters at the ends of the accumulator slots (15, 16, K - 16, K - 1) have rows in both
    chunks of the two-chunk cases; every row decides its centre by more than 1e-9"""
    X32, C = KC.dispatch_case(n, d, k)
    trace = {}
    labels, _ = KC.assign(X32.astype(np.float64), C, trace)
    assert trace['assign'] > MARGIN
    assert np.bincount(labels, minlength=k).min() > 0
    assert sorted({(k + 15) // 16 for _, _, k in KC.EDGE_DISPATCH}) == [1, 2, 3, 4]       # every case of the switch
    assert {k for _, _, k in KC.EDGE_DISPATCH} == {16, 17, 32, 33, 48, 49}
    if n > KC.CHUNK:
        for c in {15, 16, k - 16, k - 1}:
            assert (labels[:KC.CHUNK] == c).any() and (labels[KC.CHUNK:] == c).any(), c
    assert any(n > KC.CHUNK for n, _, _ in KC.EDGE_DISPATCH)


@pytest.mark.parametrize("k,k2", KC.EDGE_BOUNDARIES)
def test_edge_boundary_cases_use_every_label_below_k(k, k2):
    X32, labels = KC.boundary_case(k)
    assert k2 == k + 1 and (k + 15) // 16 != (k2 + 15) // 16                            # the pair straddles a dispatch boundary
    assert labels.min() == 0 and labels.max() == k - 1 and np.bincount(labels).min() > 0
    centres, counts = _wanted_centres(X32.astype(np.float64), labels, k2)
    assert counts[k] == 0 and not centres[k].any() and np.abs(centres[:k]).min() > 0


@pytest.mark.parametrize("k", KC.EDGE_FOREIGN_K)
@pytest.mark.parametrize("rot", [0, 3])
def test_edge_foreign_labels_would_show_if_counted(k, rot):
    """the six foreign values sit at the stage and chunk edges, their rows have no zero entry, and clusters 0 and 15 have
    rows: counting a foreign row into either (-1 & 15 == 15, -1 / 16 == 0; -16 & 15 == 0) changes its centre"""
    X32, labels, rows = KC.foreign_case(k, rot)
    X = X32.astype(np.float64)
    assert set(labels[rows].tolist()) == {-1, k, k + 15, -16, KC.INT32_MAX, KC.INT32_MIN}
    assert {63, 64, 2047, 2048} <= set(rows.tolist()) and (rows < KC.CHUNK).any() and (rows >= KC.CHUNK).any()
    assert np.all(X[rows] != 0.0)
    inside = (labels >= 0) & (labels < k)
    assert np.array_equal(np.flatnonzero(~inside), np.sort(rows))
    centres, counts = _wanted_centres(X, labels, k)
    assert counts.sum() == len(X) - len(rows) and counts[0] > 0 and counts[15] > 0
    assert np.array_equal(np.bincount(labels[inside], minlength=k), counts)              # the rows removed: the same counts
    for leak in (0, 15):                                                                 # every foreign row counted into it
        wrong = labels.copy()
        wrong[rows] = leak
        assert np.all(_wanted_centres(X, wrong, k)[0][leak] != centres[leak])
        for row in rows:                                                                 # and any single one
            wrong = labels.copy()
            wrong[row] = leak
            assert np.all(_wanted_centres(X, wrong, k)[0][leak] != centres[leak])


@pytest.mark.parametrize("m", KC.EDGE_RELOCATION_M)
@pytest.mark.parametrize("reverse", [False, True])
def test_edge_relocation_case_decides_every_path_of_the_pick(m, reverse):
    X, init = KC.relocation_case(m, reverse)
    n, k = len(X), len(init)
    assert n == 2314 and k == 4 + m and (k > 64) == (m == 66)
    assert np.array_equal(X, np.round(X)) and np.array_equal(X.astype(np.float32).astype(np.float64), X)
    trace = {}
    labels, d2 = KC.assign(X, init, trace)
    assert trace['assign'] > MARGIN                                                    # the one iteration that is asserted
    assert np.array_equal(d2, np.round(d2))
    counts = np.bincount(labels, minlength=k)
    assert counts[:4].tolist() == [1156, 1156, 1, 1] and not counts[4:].any()
    picks = KC.relocation_picks(d2, m)
    assert np.array_equal(picks, np.lexsort((np.arange(n), -d2))[:m])
    if not reverse:
        assert picks[:12].tolist() == [2312, 2313, 0, 16, 272, 288, 289, 305, 561, 577, 578, 594][:m]
        assert picks[0] >= KC.CHUNK and picks[1] >= KC.CHUNK                           # the first picks lie in chunk 1
        assert labels[2312] == 2 and labels[2313] == 3
        assert 16 % 256 == 272 % 256 and 305 % 256 == 561 % 256                        # ties inside one thread's rows
    else:
        assert picks[:2].tolist() == [0, 1] and (picks[2:] > 1).all()
        mirror = n - 1 - KC.relocation_picks(KC.assign(X[::-1], init)[1], m)
        assert not np.array_equal(picks, mirror)                                       # its own lowest rows, not the mirror's
        assert (picks >= KC.CHUNK).any() == (m == 66)
    assert (np.diff(d2[picks]) <= 0).all() and (picks % 256 != picks).any()           # rows of a second pass of r += 256
    tie = np.flatnonzero(np.diff(d2[picks]) == 0)
    assert len(tie) and (np.diff(picks)[tie] > 0).all()                                # ascending rows inside every tie
    same_thread = [(a, b) for a in picks for b in picks if a < b and a % 256 == b % 256 and d2[a] == d2[b]]
    assert same_thread
    assert len(np.unique(d2[picks])) == (3 if m == 66 else 2)
    assert m > 3
    new, shift = KC.update(X, labels, d2, init)
    donors = labels[picks[:2]]
    assert sorted(donors.tolist()) == [2, 3] and not new[donors].any()                 # count 0: the residual sum (0, 0) stays
    assert np.array_equal(new[4:], X[picks]) and shift > 0
    # a whole fit is not asserted on these rows: from the second iteration lattice rows lie exactly between two centres
    whole = {}
    KC.fit(X, k, init=init, trace=whole)
    assert whole['assign'] <= MARGIN


def test_edge_many_tiles_case_changes_labels_only_past_tile_255():
    """258 assign tiles; an iteration that is neither the first nor the last changes labels in tiles >= 256 alone, so a
    changed-label count over the first 256 tiles stops there, strictly and too early"""
    X32, init = KC.many_tiles_case()
    X = X32.astype(np.float64)
    assert X32.shape == (16449, 2) and -(-len(X) // 64) == 258
    trace = {}
    steps = KC.lloyd_steps(X, init, 0.0, 300, trace)
    assert trace['assign'] > 3e-5 and 'shift' not in trace
    assert len(steps) == 5 and steps[-1]['strict']
    assert [len(s['changed']) for s in steps] == [16449, 27, 32, 6, 0]
    middle = [s for s in steps[1:-1] if len(s['changed']) and (s['changed'] // 64).min() >= 256]
    assert len(middle) == 3
    assert all((s['changed'] // 64 == 256).all() for s in steps[2:4])
    run = KC.fit(X, 2, init=init, tol=0.0)
    assert run['n_iter'] == 5 and np.array_equal(run['labels'], steps[-1]['labels'])


@pytest.mark.parametrize("n,d,k", KC.EDGE_TRANSFORM)
def test_edge_transform_cases_decide_their_argmin(n, d, k):
    X32, C = KC.transform_case(n, d, k)
    trace = {}
    KC.assign(X32.astype(np.float64), C, trace)
    assert trace['assign'] > MARGIN
    assert any(k > 64 and n % 64 for n, _, k in KC.EDGE_TRANSFORM)                      # grid.y > 1 with a row tail


@pytest.mark.parametrize("n,d", KC.EDGE_VARIANCE)
def test_edge_variance_cases(n, d):
    """the restated column variances against numpy's, the constant column and the single row"""
    X = KC.variance_case(n, d).astype(np.float64)
    mean, var = KC.column_variances(X)
    assert np.allclose(mean, X.mean(axis=0), rtol=1e-12, atol=0) and np.allclose(var, X.var(axis=0), rtol=1e-10, atol=1e-300)
    assert KC.mean_variance(X) == float(np.cumsum(var)[-1] / d)
    if d >= 2:
        assert (X[:, d // 2] == 3.0).all() and mean[d // 2] == 3.0 and var[d // 2] == 0.0
    if n == 1:
        assert not var.any()
    else:
        assert (np.delete(var, d // 2) > 0.0).all() if d >= 2 else var[0] > 0.0
    assert {(n - 1) // KC.CHUNK for n, _ in KC.EDGE_VARIANCE} == {0, 1, 2}


def test_edge_scan_case_is_exact():
    """closest, the scan and every threshold are exact, the thresholds sit on a chunk's last scan entry and just past it,
    the last chunk has one row, and the best potential is tied between different rows"""
    X = KC.scan_case()
    n = len(X)
    assert n == 2 * KC.CHUNK + 1
    closest = KC.sqd(X, X[0:1])[:, 0]
    assert closest[0] == 0.0 and (closest[1:] == 1.0).all()
    scan = KC.chunk_scan(closest)
    assert np.array_equal(scan, np.arange(n, dtype=np.float64)) and scan[-1] == 4096.0
    rand = np.array(KC.EDGE_SCAN_RAND)
    v = rand * scan[-1]
    assert v.tolist() == [0.0, 2047.0, 2047.5, 2048.0, 4095.0, 4095.5, 4096.0, 6144.0]
    assert v[1] == scan[KC.CHUNK - 1] and v[4] == scan[2 * KC.CHUNK - 1] and v[6] == scan[-1]
    assert np.minimum(np.searchsorted(scan, v), n - 1).tolist() == KC.EDGE_SCAN_ROWS
    for r, row in zip(rand, KC.EDGE_SCAN_ROWS):
        cand, pots, b, _ = KC.plusplus_trial(X, closest, [r])
        assert cand.tolist() == [row] and b == 0 and pots[0] == (4096.0 if row == 0 else 2048.0)
    cand, pots, b, new = KC.plusplus_trial(X, closest, rand)
    assert cand.tolist() == KC.EDGE_SCAN_ROWS and b == 1 and cand[1] != cand[2]
    assert pots.tolist() == [4096.0] + [2048.0] * 7                                      # the tie: rows 2047 and 2048 first
    assert np.array_equal(new[1::2], np.zeros(2048)) and new[0] == 0.0 and (new[2::2] == 1.0).all()
    assert np.array_equal(KC.plusplus_steps(X, 2, 0, rand[None, :]), [0, 2047])


def test_edge_scan_plateaus_cross_both_chunk_boundaries():
    X = KC.scan_case()
    closest = KC.sqd(X, X[2047:2048])[:, 0]
    assert closest[0] == 1.0 and not closest[1::2].any() and (closest[2::2] == 4.0).all()
    scan = KC.chunk_scan(closest)
    assert scan[-1] == 8193.0 and np.array_equal(scan[2::2], 1.0 + 4.0 * np.arange(1, 2049))
    for last in (KC.CHUNK - 1, 2 * KC.CHUNK - 1):                                        # a plateau ends each full chunk
        assert scan[last] == scan[last - 1] and scan[last + 1] == scan[last] + 4.0
    rand, v = KC.plateau_thresholds()
    assert np.array_equal(rand * scan[-1], v)
    dyadic = rand[:8]
    assert np.array_equal(dyadic * 2048, np.round(dyadic * 2048))
    assert np.array_equal(v[:8] * 2048, np.round(v[:8] * 2048))                          # exact products
    assert v[8:].tolist() == [1.0, 2.0, 5.0, 6.0, 4093.0, 4094.0, 4097.0, 4098.0, 8189.0, 8190.0]
    on = np.isin(v, scan)
    assert on.sum() == 6 and (~on).sum() == 12                                           # on plateau values and between them
    rows = np.minimum(np.searchsorted(scan, v), len(X) - 1)
    assert rows[8:].tolist() == [0, 2, 2, 4, 2046, 2048, 2048, 2050, 4094, 4096]
    assert rows[:8].tolist() == [0, 2, 1024, 2046, 2048, 2050, 4094, 4096]
    for r, row in zip(rand, rows):
        assert KC.plusplus_steps(X, 2, 2047, np.array([[r]])).tolist() == [2047, row]


@pytest.mark.parametrize("name,tol", KC.EDGE_CONTROL)
def test_edge_control_cases_stop_as_they_claim(name, tol):
    """several iterations, every assign and shift margin above 1e-9, a strict stop for the cases' own tolerances and a
    stop by the tolerance for 1e-3; the steps are the iterations of ``lloyd``"""
    strict = tol is None                                                                 # the cases' own tolerances
    X, start, tol, tol_abs = KC.control_case(name, tol)
    trace = {}
    steps = KC.lloyd_steps(X, start, tol_abs, 300, trace)
    assert all(value > MARGIN for value in trace.values()), trace
    assert len(steps) >= 2 and steps[-1]['stopped'] and not any(s['stopped'] for s in steps[:-1])
    assert steps[-1]['strict'] == strict
    if steps[-1]['strict']:
        assert steps[-1]['shift'] == 0.0 and np.array_equal(steps[-1]['centres'], steps[-2]['centres'])
    else:
        assert 0.0 < steps[-1]['shift'] <= tol_abs and len(steps[-1]['changed']) > 0
    labels, inertia, C, n_iter = KC.lloyd(X, start, tol_abs, 300)
    assert n_iter == len(steps) and np.array_equal(C, steps[-1]['centres'])
    assert {tol for _, tol in KC.EDGE_CONTROL} == {None, 1e-3}


def test_edge_permuted_lattice_stops_after_one_iteration():
    X, init, perm = KC.permuted_lattice_case()
    assert len(np.unique(X, axis=0)) == 256 and not np.array_equal(perm, np.arange(256))
    run = KC.fit(X, 256, init=init)
    inverse = np.empty(256, dtype=np.int64)
    inverse[perm] = np.arange(256)
    assert run['n_iter'] == 1 and np.array_equal(run['labels'], inverse) and run['inertia'] == 0.0
    step, = KC.lloyd_steps(X, init, KC.mean_variance(X) * 1e-4, 300)
    assert not step['strict'] and step['stopped'] and step['shift'] == 0.0               # stopped by the tolerance
