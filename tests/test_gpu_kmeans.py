"""ava_amd.kmeans on the MI355X against the numpy restatement of tests/kmeans_cases.py and scikit-learn's golden results
(tests/golden/kmeans.npz).  Shapes sit at the kernels' edges: the 64-row assign tile, the 64-centre tile, the 16-feature
slab and 32-feature stage, the 2048-row chunk.

Bounds: labels, indices and n_iter are exact.  A step (assign, update, inertia) is within 1e-12 of the largest wanted entry,
the project's step bound for fp64 sums of this length (test_gpu_gmm.py); whole fits are within 1e-11 of the restatement and
max(1e-11, 4 x floor) of sklearn, the floors being the reference's own noise (make_golden_kmeans.py).  The golden cases are
verified on the CPU to stay 1e-9 away from every discontinuous rule (test_cpu_kmeans.py), so equal labels are a condition,
not a hope."""
import warnings

import numpy as np
import pytest
import torch

import kmeans_cases as KC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import cluster_metrics as CM
from ava_amd import kmeans as KM

pytestmark = pytest.mark.gpu
STEP = 1e-12
FIT = 1e-11


@pytest.fixture(scope="module")
def golden():
    return load_golden("kmeans.npz")


_RUNS = {}


def restated(name):
    if name not in _RUNS:
        X, kw = KC.fit_case(name)
        kw = dict(kw)
        _RUNS[name] = KC.fit(X, kw.pop('n_clusters'), **kw)
    return _RUNS[name]


def within(got, want, bound):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() <= bound * max(np.abs(want).max(), np.finfo(float).tiny)


def rows32(n, d, seed):
    """(float32 rows, their float64 copy)"""
    X32 = np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)
    return X32, X32.astype(np.float64)


def pair_sqdist(X, C, labels):
    """ava_pair_sqdist of every (row, its centre) pair, float64 [N] on the device"""
    L = torch.cat([torch.from_numpy(X), torch.from_numpy(C)]).cuda().contiguous()
    a = torch.arange(len(X), dtype=torch.int64, device="cuda")
    b = labels.to(torch.int64) + len(X)
    out = torch.empty(len(X), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().ava_pair_sqdist(L.data_ptr(), X.shape[1], a.data_ptr(), b.data_ptr(), len(X), out.data_ptr(),
                                           _lib.stream()), "ava_pair_sqdist")
    return out


# ---- assign and update -----------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (63, 31, 2), (64, 32, 63), (65, 33, 64), (65, 1, 65), (2047, 31, 65), (2048, 32, 129),
          (2049, 128, 256), (4097, 33, 2), (4097, 1, 129)]


@pytest.mark.parametrize("n,d,k", SHAPES)
def test_assign_and_update_against_the_restatement(n, d, k):
    X32, X = rows32(n, d, 100 + n + d + k)
    rng = np.random.RandomState(k)
    C = X[rng.choice(n, size=k, replace=k > n)] + 0.25 * rng.standard_normal((k, d))
    want_labels, want_d2 = KC.assign(X, C)
    labels, d2 = KM.assign(X, C)
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want_labels)
    assert torch.equal(d2, pair_sqdist(X, C, labels))                       # the bits of the pair
    assert within(d2, want_d2, STEP)
    labels32, d232 = KM.assign(X32, C)
    assert torch.equal(labels32, labels) and torch.equal(d232, d2)          # float32 rows: the same bits
    total = KM._assign_device(torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda(), inertia=True)[2]
    assert within(total, KC.chunk_sum(want_d2), STEP)
    sums, counts = KC.cluster_sums(X, want_labels, k)
    want_centres = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], 0.0)
    centres, cnt = KM.update(X, labels, k)
    assert cnt.dtype == torch.int64 and np.array_equal(cnt.cpu().numpy(), counts)
    assert within(centres, want_centres, STEP)
    centres32, cnt32 = KM.update(X32, labels.cpu().numpy().astype(np.int64), k)
    assert torch.equal(centres32, centres) and torch.equal(cnt32, cnt)


def test_ties_go_to_the_lowest_index():
    _, X = rows32(200, 7, 3)
    C = np.array(X[:130])
    C[70] = C[5]
    C[129] = C[5]                                                           # duplicates in the second and third centre tile
    C[64] = C[63]
    labels = KM.assign(X, C)[0].cpu().numpy()
    assert np.array_equal(labels, KC.assign(X, C)[0])
    assert labels[5] == 5 and not np.isin(labels, [64, 70, 129]).any()
    # a row equidistant from two centres (exactly: the differences are the same numbers with other signs)
    Y = np.array([[0.0, 0.0], [3.0, 0.5]])
    D = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0], [3.0, 1.5], [3.0, -0.5]])
    labels, d2 = KM.assign(Y, D)
    assert labels.cpu().tolist() == [0, 4] and d2.cpu().tolist() == [1.0, 1.0]


# ---- k-means++ -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(300, 5, 2), (3000, 7, 9), (4500, 3, 256)])
def test_plusplus_against_the_restatement(n, d, k):
    """one, two and three scan chunks; L = 2 (K = 2) and L = 7 (K = 256)"""
    assert KC.n_trials(2) == 2 and KC.n_trials(256) == 7
    X32, X = rows32(n, d, n + k)
    want = KC.plusplus(X, k, np.random.RandomState(5))
    centres, idx = KM.kmeans_plusplus(X, k, random_state=5)
    assert idx.dtype == np.int64 and np.array_equal(idx, want) and np.array_equal(centres, X[want])
    centres32, idx32 = KM.kmeans_plusplus(torch.from_numpy(X32).cuda(), k, random_state=np.random.RandomState(5))
    assert idx32.is_cuda and np.array_equal(idx32.cpu().numpy(), want) and centres32.dtype == torch.float32
    assert np.array_equal(centres32.cpu().numpy(), X32[want])


def test_plusplus_thresholds_at_zero_and_at_the_potential():
    """a threshold of 0 finds row 0; one at the potential finds the last row that adds to the scan; one past it is
    clipped to N - 1"""
    _, X = rows32(4500, 3, 11)
    rand = np.array([[0.0, 0.5, 1.0], [1.5, 0.0, 0.3], [1.0, 1.0, 1.0]])
    want = KC.plusplus_steps(X, 4, 7, rand)
    got = KM._plusplus_device(torch.from_numpy(X).cuda(), 4, None, rand=rand, first=7)
    assert np.array_equal(got.cpu().numpy(), want)
    only_zero = KM._plusplus_device(torch.from_numpy(X).cuda(), 2, None, rand=np.zeros((1, 2)), first=7)
    assert only_zero.cpu().tolist() == [7, 0]
    past = KM._plusplus_device(torch.from_numpy(X).cuda(), 2, None, rand=np.full((1, 2), 1.5), first=7)
    assert past.cpu().tolist() == [7, 4499]


@pytest.mark.parametrize("name", sorted(KC.FIT_CASES))
def test_plusplus_indices_are_sklearns(golden, name):
    X, kw = KC.fit_case(name)
    idx = KM.kmeans_plusplus(X, kw['n_clusters'], random_state=kw.get('random_state', 0))[1]
    assert np.array_equal(idx, golden[name + "/pp"])


# ---- whole fits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KC.FIT_CASES))
def test_fit_is_the_restatements_and_sklearns(golden, name):
    """labels on every row and n_iter equal to both; floats within 1e-11 of the restatement and max(1e-11, 4 floors) of
    sklearn.  The cases cover init as an array (one_empty: one empty cluster in the first iteration), 'random' with
    n_init = 3, max_iter = 1 (a non-strict stop with the extra assignment) and tol = 0."""
    X, kw = KC.fit_case(name)
    mine = restated(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", KM.KMeansConvergenceWarning)
        m = KM.KMeans(**kw).fit(X)
    assert m.labels_.dtype == np.int32 and m.cluster_centers_.dtype == np.float64 and m.n_features_in_ == X.shape[1]
    print(name, "n_iter", m.n_iter_, "inertia rel", abs(m.inertia_ - mine["inertia"]) / mine["inertia"],
          "centres", np.abs(m.cluster_centers_ - mine["centres"]).max() / np.abs(mine["centres"]).max())
    assert np.array_equal(m.labels_, mine["labels"]) and np.array_equal(m.labels_, golden[name + "/labels"])
    assert m.n_iter_ == mine["n_iter"] == golden[name + "/n_iter"]
    assert within(m.cluster_centers_, mine["centres"], FIT) and within(m.inertia_, mine["inertia"], FIT)
    assert within(m.cluster_centers_, golden[name + "/centres"], max(FIT, 4 * float(golden[name + "/floor_centres"])))
    assert within(m.inertia_, golden[name + "/inertia"], max(FIT, 4 * float(golden[name + "/floor_inertia"])))
    if name == "max_iter1":
        assert m.n_iter_ == 1 and np.array_equal(m.labels_, KC.assign(X, m.cluster_centers_)[0])


def test_fit_bits_do_not_depend_on_the_run_the_block_or_the_container():
    X64, kw = KC.fit_case("n2049_d33_k8")
    X32 = X64.astype(np.float32)
    X = X32.astype(np.float64)

    def fit(rows, **more):
        m = KM.KMeans(**dict(kw, **more)).fit(rows)
        if torch.is_tensor(rows):
            assert m.labels_.is_cuda and m.cluster_centers_.is_cuda and m.labels_.dtype == torch.int32
            return m.labels_.cpu().numpy(), m.cluster_centers_.cpu().numpy(), m.inertia_, m.n_iter_
        return m.labels_, m.cluster_centers_, m.inertia_, m.n_iter_

    first = fit(X)
    assert first[3] > 3                                                     # several blocks at iter_block = 1 and 3
    others = [fit(X, iter_block=b) for b in (1, 3, 16, 300)] + [fit(X), fit(torch.from_numpy(X).cuda()), fit(X32),
                                                                  fit(torch.from_numpy(X32).cuda())]
    for other in others:
        assert np.array_equal(other[0], first[0]) and np.array_equal(other[1], first[1])
        assert other[2] == first[2] and other[3] == first[3]


# ---- empty clusters --------------------------------------------------------------------------------------------------
def test_three_empty_clusters_and_ties_in_the_farthest_distance():
    """Three clusters are empty at once and the farthest distance is shared by eight rows: the empty clusters 2, 3, 4 take
    the rows 0, 8, 72 (the lowest rows of the tie, ascending).  Checked against the restatement only: sklearn's
    argpartition leaves the order among rows at equal distance, and among several picks, unspecified."""
    X, init = KC.empty_three_case()
    one = KM.KMeans(5, init=init, max_iter=1).fit(X)
    labels, d2 = KC.assign(X, init)
    want, _ = KC.update(X, labels, d2, init)
    assert np.array_equal(want[2:], X[[0, 8, 72]])
    assert np.array_equal(one.cluster_centers_[2:], X[[0, 8, 72]]) and within(one.cluster_centers_, want, STEP)
    mine = KC.fit(X, 5, init=init)
    m = KM.KMeans(5, init=init).fit(X)
    assert np.array_equal(m.labels_, mine["labels"]) and m.n_iter_ == mine["n_iter"]
    assert within(m.cluster_centers_, mine["centres"], FIT) and within(m.inertia_, mine["inertia"], FIT)


def test_fewer_distinct_clusters_than_asked_for_warns():
    X = np.repeat(np.array([[0.0, 0.0], [5.0, 5.0]]), 10, axis=0)
    with pytest.warns(KM.KMeansConvergenceWarning, match=r"distinct clusters \(2\) found smaller than n_clusters \(3\)"):
        m = KM.KMeans(3, init=np.array([[0.0, 0.0], [5.0, 5.0], [0.0, 0.0]])).fit(X)
    mine = KC.fit(X, 3, init=np.array([[0.0, 0.0], [5.0, 5.0], [0.0, 0.0]]))
    assert np.array_equal(m.labels_, mine["labels"]) and m.n_iter_ == mine["n_iter"] and m.inertia_ == 0.0


# ---- the other entry points ------------------------------------------------------------------------------------------
def test_predict_transform_and_score_on_unseen_rows():
    X, kw = KC.fit_case("n300_d5_k4_sep1")
    m = KM.KMeans(**kw).fit(X)
    for Y in (KC.blobs(77, 5, 4, 1.0, 50), KC.blobs(3, 5, 4, 1.0, 51)):     # also fewer rows than centres
        labels, d2 = KC.assign(Y, m.cluster_centers_)
        assert m.predict(Y).dtype == np.int32 and np.array_equal(m.predict(Y), labels)
        dist = m.transform(Y)
        assert dist.shape == (len(Y), 4) and within(dist, np.sqrt(KC.sqd(Y, m.cluster_centers_)), STEP)
        assert np.array_equal(np.argmin(dist, axis=1), labels)
        assert within(m.score(Y), -KC.chunk_sum(d2), STEP)
        assert torch.equal(m.predict(torch.from_numpy(Y).cuda()).cpu(), torch.from_numpy(m.predict(Y)))
    assert np.array_equal(KM.KMeans(**kw).fit_predict(X), m.labels_)
    assert np.array_equal(KM.KMeans(**kw).fit_transform(X), m.transform(X))
    with pytest.raises(ValueError, match="X has 4 features, but KMeans is expecting 5 features"):
        m.predict(np.zeros((3, 4)))


def test_sweep_equals_separate_fits_and_separate_scores():
    X, _ = KC.fit_case("n300_d5_k4_sep6")
    ks = [2, 4, 7]
    sweep = KM.kmeans_sweep(X, ks, scores=True, random_state=0)
    assert sweep['k'].tolist() == ks and sweep['labels'].shape == (3, 300) and sweep['labels'].dtype == np.int32
    for a, k in enumerate(ks):
        m = KM.KMeans(k, random_state=0).fit(X)
        assert np.array_equal(sweep['labels'][a], m.labels_)
        assert sweep['inertia'][a] == m.inertia_ and sweep['n_iter'][a] == m.n_iter_
        assert sweep['silhouette'][a] == CM.silhouette_score(X, m.labels_)
        assert sweep['calinski_harabasz'][a] == CM.calinski_harabasz_score(X, m.labels_)
        assert sweep['davies_bouldin'][a] == CM.davies_bouldin_score(X, m.labels_)
    assert set(KM.kmeans_sweep(X, [3], random_state=0)) == {'k', 'inertia', 'n_iter', 'labels'}


def test_refusals_leave_the_outputs_untouched():
    """AVA_EINVAL / AVA_EWORKSPACE come before any launch: the outputs keep their fill"""
    lib = _lib.load()
    X = torch.zeros((100, 4), dtype=torch.float64, device="cuda")
    C = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
    labels = torch.full((100,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((100,), -7.0, dtype=torch.float64, device="cuda")
    nbytes = int(lib.ava_km_workspace_bytes(100, 4, 3))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = _lib.stream()
    args = [X.data_ptr(), 1, 100, 4, 3, C.data_ptr(), labels.data_ptr(), d2.data_ptr(), None, ws.data_ptr(), nbytes, st]
    for pos, bad, rc in [(1, 5, -1), (2, 0, -1), (3, 129, -1), (4, 257, -1), (5, None, -1), (9, None, -1), (10, 8, -3)]:
        call = list(args)
        call[pos] = bad
        assert lib.ava_km_assign(*call) == rc, pos
    ctl = torch.zeros(8, dtype=torch.int32, device="cuda")
    mv = torch.ones(1, dtype=torch.float64, device="cuda")
    fit = [X.data_ptr(), 1, 100, 4, 3, C.data_ptr(), labels.data_ptr(), d2.data_ptr(), 1e-4, mv.data_ptr(), 0, 2,
           ctl.data_ptr(), None, ws.data_ptr(), nbytes, st]
    for pos, bad, rc in [(4, 101, -1), (8, -1.0, -1), (9, None, -1), (11, 0, -1), (12, None, -1), (15, 8, -3)]:
        call = list(fit)
        call[pos] = bad
        assert lib.ava_km_fit(*call) == rc, pos
    torch.cuda.synchronize()
    assert bool((labels == -7).all()) and bool((d2 == -7.0).all()) and bool((ctl == 0).all())


def test_limits_are_refused():
    with pytest.raises(ValueError, match="at most 256 clusters"):
        KM.KMeans(257).fit(np.zeros((300, 2)))
    with pytest.raises(ValueError, match="d = 129 features, at most 128"):
        KM.KMeans(2).fit(np.zeros((10, 129)))
    with pytest.raises(ValueError, match="n_samples=3 should be >= n_clusters=4"):
        KM.KMeans(4).fit(np.zeros((3, 2)))
