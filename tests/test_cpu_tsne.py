"""ava_amd.tsne without a GPU: the numpy restatement of tests/tsne_cases.py against scikit-learn's own functions
(tests/golden/tsne.npz), the host schedule against sklearn's ``_gradient_descent``, the argument checks that need no
device, and ``mmd.install(tsne=True)``."""
import types

import numpy as np
import pytest

import tsne_cases as TC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import mmd
from ava_amd import tsne as T


@pytest.fixture(scope="module")
def golden():
    return load_golden("tsne.npz")


# ---- the restatement against sklearn ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.GOLDEN_P_CASES)
def test_restatement_probabilities(golden, name):
    P = TC.p_case(name)[4]                                           # asserts the search margin
    want = golden["P_" + name]
    np.testing.assert_allclose(P, want, rtol=0, atol=1e-12 * want.max())
    np.testing.assert_array_equal(P, P.T)
    # the eps clamp adds at most eps per entry to a sum of 1
    assert np.all(np.diag(P) == 0.0) and abs(P.sum() - 1.0) <= P.size * TC.MACHINE_EPSILON + 1e-12


@pytest.mark.parametrize("name", TC.GOLDEN_P_CASES)
def test_restatement_kl_gradient(golden, name):
    kl, grad = TC.kl_gradient(golden["Y_" + name], golden["P_" + name])
    np.testing.assert_allclose(kl, golden["kl_" + name], rtol=1e-11)
    want = golden["grad_" + name]
    np.testing.assert_allclose(grad, want, rtol=0, atol=1e-11 * np.abs(want).max())


def test_special_cases_take_their_branches():
    """the outlier row starts from sum_Pi == 0 and ends at P's eps clamp; duplicates have zero distances; the clamp
    layout reaches Q's eps clamp"""
    X, _, _, D2, P = TC.p_case("outlier")
    assert np.exp(-D2[11] * 1.0)[np.arange(len(X)) != 11].sum() == 0.0
    assert np.sum(np.delete(P[11], 11) == TC.MACHINE_EPSILON) > 10
    D2 = TC.p_case("duplicates")[3]
    assert D2[5, 7] == 0.0 and D2[40, 45] == 0.0
    Y = TC.clamp_y(130)
    w = 1.0 / (1.0 + ((Y[2] - Y[0]) ** 2).sum())
    Z = sum(1.0 / (1.0 + ((Y[i] - Y[j]) ** 2).sum()) for i in range(130) for j in range(130) if i != j)
    assert w / Z < TC.MACHINE_EPSILON and np.all(Y[3] == Y[4])


def test_fma_restatement_is_one_rounding():
    """the emulated fma against exact rational arithmetic"""
    from fractions import Fraction
    a = TC.syn.gauss(200, 9790)
    c = np.abs(TC.syn.gauss(200, 9791)) * 10.0
    got = TC.fma(a, a, c)
    for x, z, g in zip(a, c, got):
        assert g == float(Fraction(float(x)) * Fraction(float(x)) + Fraction(float(z)))


def test_descent_references_are_away_from_the_gain_threshold():
    for name in TC.DESCENT_CASES:
        for state in TC.DESCENT_STATES:
            for momentum, exaggeration in ((0.5, 12.0), (0.8, 1.0)):
                TC.descent_reference(name, state, momentum, exaggeration, 5)         # asserts the margin


# ---- the schedule against sklearn's _gradient_descent ----------------------------------------------------------------
def _sklearn_schedule(errors, max_iter, n_iter_without_progress, min_grad_norm):
    """TSNE._tsne's two calls of sklearn's _gradient_descent on a scripted objective: iteration i costs errors[i] and
    has a constant gradient"""
    from sklearn.manifold._t_sne import _gradient_descent
    calls = []

    def objective(p, compute_error=True):
        calls.append(1)
        return errors[len(calls) - 1], np.ones_like(p)

    args = dict(n_iter_check=50, min_grad_norm=min_grad_norm, learning_rate=1.0, verbose=0, kwargs={}, args=[])
    _, error, it = _gradient_descent(objective, np.zeros(4), it=0, max_iter=250, n_iter_without_progress=250,
                                     momentum=0.5, **args)
    if it < 250 or max_iter - 250 > 0:
        _, error, it = _gradient_descent(objective, np.zeros(4), it=it + 1, max_iter=max_iter,
                                         n_iter_without_progress=n_iter_without_progress, momentum=0.8, **args)
    return error, it, len(calls)


def _scripted_run(errors, log):
    done = [0]

    def run(n_iters, exaggeration, momentum):
        log.append((done[0], n_iters, exaggeration, momentum))
        done[0] += n_iters
        return errors[done[0] - 1], 1.0

    return run, done


SCHEDULES = {
    "no_stop": (lambda i: 10.0 / (1 + i), 1000, 300, 1e-7),
    "no_stop_ragged": (lambda i: 10.0 / (1 + i), 1013, 300, 1e-7),
    "grad_norm": (lambda i: 10.0 / (1 + i), 1000, 300, np.inf),
    "no_progress": (lambda i: 10.0 / (1 + i) if i < 400 else 1.0 + 1e-3 * i, 1000, 100, 1e-7),
    "no_progress_phase1": (lambda i: 10.0 + i, 1000, 300, 1e-7),
    "shortest": (lambda i: 10.0 / (1 + i), 250, 300, 1e-7),
}


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_schedule_matches_sklearn(name):
    fn, max_iter, nwp, min_grad_norm = SCHEDULES[name]
    errors = [fn(i) for i in range(max_iter + 1)]
    want_error, want_it, want_calls = _sklearn_schedule(errors, max_iter, nwp, min_grad_norm)
    log = []
    run, done = _scripted_run(errors, log)
    kl, it = T.schedule(run, max_iter, nwp, min_grad_norm, 12.0)
    assert (kl, it, done[0]) == (want_error, want_it, want_calls)
    for start, n_iters, _, _ in log:                               # blocks end at a check or at the last iteration
        assert 1 <= n_iters <= 50 and ((start + n_iters) % 50 == 0 or start + n_iters == max_iter)
    if name == "grad_norm":
        assert it == 99 and log == [(0, 50, 12.0, 0.5), (50, 50, 1.0, 0.8)]
    if name == "no_stop":
        assert it == 999 and len(log) == 20 and log[4] == (200, 50, 12.0, 0.5) and log[5] == (250, 50, 1.0, 0.8)
    if name == "no_progress":
        assert it < 999


def test_schedule_matches_the_restatement_schedule():
    """tsne_cases.run (one iteration at a time) and ava_amd.tsne.schedule (blocks of 50) stop at the same iteration"""
    P = TC.run_case("precomputed40")[5]
    Y0 = TC.random_init(40)
    for min_grad_norm, want in ((np.inf, 99), (1e-7, 299)):
        Y, kl, it = TC.run(P, Y0, max_iter=300, min_grad_norm=min_grad_norm)
        state = [Y0.copy(), np.zeros((40, 2)), np.ones((40, 2))]

        def run(n_iters, exaggeration, momentum):
            state[0], state[1], state[2], k, g = TC.descend(*state, P, n_iters, momentum, 50.0, exaggeration)
            return k, g

        kl2, it2 = T.schedule(run, 300, 300, min_grad_norm, 12.0)
        assert it == it2 == want and kl == kl2
        np.testing.assert_array_equal(Y, state[0])


# ---- argument checks that need no device -----------------------------------------------------------------------------
def test_constructor_rejects_what_is_not_on_the_device():
    for kw in (dict(n_components=3), dict(method="barnes_hut"), dict(metric="cosine"), dict(init="pca")):
        with pytest.raises(NotImplementedError):
            T.TSNE(**kw)
    with pytest.raises(ValueError):
        T.TSNE(max_iter=249)
    t = T.TSNE(n_components=2, random_state=42, metric='precomputed', method='exact', perplexity=30.0, verbose=1,
               n_jobs=2)                                            # the reference's call, and ignored keywords
    assert (t.metric, t.perplexity, t.random_state, t.init, t.learning_rate) == ('precomputed', 30.0, 42, 'random', 'auto')
    assert T.MAX_N == 32768


def test_fit_checks_run_before_the_device_is_touched():
    D = np.abs(TC.syn.gauss(40 * 40, 9795)).reshape(40, 40)
    cases = [
        (dict(metric='precomputed', perplexity=40.0), D),                       # perplexity >= N
        (dict(metric='precomputed', perplexity=30.0), D[:20, :20]),             # the reference's default, 20 conditions
        (dict(metric='precomputed', perplexity=5.0), -D),                       # negative distances
        (dict(metric='precomputed', perplexity=5.0), np.where(np.eye(40) > 0, np.nan, D)),
        (dict(metric='precomputed', perplexity=5.0), np.where(np.eye(40) > 0, np.inf, D)),
        (dict(metric='precomputed', perplexity=5.0), D[:, :30]),                # not square
        (dict(perplexity=5.0), np.full((40, 3), np.inf)),
        (dict(perplexity=5.0), np.zeros(40)),                                   # not 2-D
        (dict(perplexity=5.0, init=np.zeros((39, 2))), D),                      # init of another shape
    ]
    for kw, X in cases:
        with pytest.raises(ValueError):
            T.TSNE(**kw).fit(X)

    t = T.TSNE()
    with pytest.raises(ValueError, match="MAX_N"):
        t._check(np.broadcast_to(np.float32(0.0), (T.MAX_N + 1, 2)))


def test_library_argument_checks():
    """ava_ts_* return AVA_EINVAL / sizes before any HIP call"""
    lib = _lib.load()
    assert lib.ava_ts_max_n() == T.MAX_N
    assert lib.ava_ts_col_chunks(1) == 0 and lib.ava_ts_col_chunks(T.MAX_N + 1) == 0
    assert [lib.ava_ts_col_chunks(n) for n in (2, 300, 1024, 10000, 32768)] == [1, 1, 2, 3, 1]
    assert lib.ava_ts_workspace_bytes(1, 0) == 0 and lib.ava_ts_workspace_bytes(100, 65) == 0
    # the larger of (64-row tiles)^2 + 2 and 2 (32-row tiles) chunks + 2 n chunks doubles, rounded up to 256, plus 256
    assert lib.ava_ts_workspace_bytes(130, 3) == ((2 * 5 * 3 + 3 * 130 * 2) * 8 + 255) // 256 * 256 + 256
    assert lib.ava_ts_workspace_bytes(10000, 0) == ((2 * 313 * 3 + 3 * 10000 * 2) * 8 + 255) // 256 * 256 + 256
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    assert p % 16 == 0
    assert lib.ava_ts_sqdist(None, 0, 4, 3, 1, p, 4, None) == -1
    assert lib.ava_ts_sqdist(p, 2, 4, 3, 1, p, 4, None) == -1                     # dtype
    assert lib.ava_ts_sqdist(p, 0, 5, 3, 1, p, 5, None) == -1                     # odd row stride
    assert lib.ava_ts_sqdist(p, 0, 4, 3, 1, p + 8, 4, None) == -1                 # misaligned
    assert lib.ava_ts_square(p, 1, p, 2, None) == -1
    assert lib.ava_ts_joint(p, 4, 4, 4.0, p, 1 << 20, None) == -1                 # perplexity >= n
    assert lib.ava_ts_joint(p, 4, 4, 2.0, p, 8, None) == -3
    assert lib.ava_ts_kl_gradient(p, p, 4, 4, 1.0, 65, p, p, p, 1 << 20, None) == -1
    assert lib.ava_ts_kl_gradient(p, p, 4, 4, 1.0, 1, p, p, p, 8, None) == -3
    assert lib.ava_ts_descend(p, p, p, p, 4, 4, 0, 0.5, 1.0, 1.0, 1, p, p, 1 << 20, None) == -1
    assert lib.ava_ts_descend(p, None, p, p, 4, 4, 1, 0.5, 1.0, 1.0, 1, p, p, 1 << 20, None) == -1


# ---- mmd.install ------------------------------------------------------------------------------------------------------
def test_install_tsne():
    stub = types.SimpleNamespace(TSNE="sklearn's", other=1)
    before = dict(vars(stub))
    mmd.install(module=stub)
    assert stub.TSNE == "sklearn's"
    plain = dict(vars(stub))
    mmd.install(module=stub, tsne=True)
    assert stub.TSNE is T.TSNE
    after = dict(vars(stub))
    after.pop("TSNE"), plain.pop("TSNE")
    assert after == plain and before["other"] == stub.other
    bare = types.SimpleNamespace()
    mmd.install(module=bare)
    assert not hasattr(bare, "TSNE")
