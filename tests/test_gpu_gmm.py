"""The kernels of csrc/mixture.hip and ava_amd.mixture.GaussianMixture on the MI355X: the E-step and the M-step against
the numpy restatement of tests/gmm_cases.py at chunk, stage and block edges, whole fits against the restatement and
against scikit-learn's own values (tests/golden/gmm.npz), both again at the library's limits of 64 components and 128
features, the run shapes that must not change a bit, the k-means start, the statistics and the error paths.
tests/test_cpu_gmm.py shows that the restatement is sklearn's arithmetic and that
the cases are away from the discontinuous rules.

Bounds: a step is held within 1e-12 of the largest wanted entry of each quantity (the project's bound for fp64 sums of
this length).  A whole fit is held, per quantity and relative to its largest entry, within 1e-11 of the restatement
and within max(1e-11, 4 x the stored reference-side floor) of sklearn."""
import numpy as np
import pytest
import torch

import gmm_cases as GC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import mixture as M

pytestmark = pytest.mark.gpu
STEP_TOL = 1e-12
FIT_TOL = 1e-11


@pytest.fixture(scope="module")
def golden():
    return load_golden("gmm.npz")


def _np(t):
    return t.cpu().numpy()


def close(got, want, tol, what, where=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if where is not None:
        got, want = got[where], want[where]
    bound = tol * np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: max err %.2e, bound %.2e" % (what, err, bound))
    assert np.isfinite(got).all() and err <= bound, what


def check_e_step(case, cov_type):
    X, weights, means, _, pchol, lpn, log_resp, resp = case
    got = [_np(t) for t in M.e_step(X, weights, means, pchol, cov_type)]
    close(got[0], lpn, STEP_TOL, "log_prob_norm")
    close(got[1], log_resp, STEP_TOL, "log_resp", resp >= 1e-300)
    close(got[2], resp, STEP_TOL, "resp")
    assert not np.isnan(got[1]).any()
    from_tensor = M.e_step(torch.from_numpy(X).cuda(), *(torch.from_numpy(a).cuda() for a in (weights, means, pchol)),
                           cov_type)
    for a, b in zip(got, from_tensor):
        np.testing.assert_array_equal(a, _np(b))
    return got


def check_m_step(case, cov_type, reg_covar=1e-6):
    X, resp = case[0], case[7]
    want = GC.m_step(X, resp, reg_covar, cov_type)
    got = [_np(t) for t in M.m_step(X, resp, reg_covar, cov_type)]
    for q, g, w in zip(("weights", "means", "covariances", "precisions_cholesky"), got, want):
        close(g, w, STEP_TOL, q)
    close(got[4], GC.log_det(want[3], cov_type), STEP_TOL, "log_det")
    if cov_type == "full":
        np.testing.assert_array_equal(got[2], np.swapaxes(got[2], 1, 2))            # exactly symmetric
        np.testing.assert_array_equal(np.tril(got[3], -1), 0.0)                     # exactly triangular
    return got


# ---- steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", sorted(GC.STEP_CASES))
def test_e_step(name, cov_type):
    check_e_step(GC.step_case(name, cov_type), cov_type)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", sorted(GC.STEP_CASES))
def test_m_step(name, cov_type):
    check_m_step(GC.step_case(name, cov_type), cov_type)


@pytest.mark.parametrize("n", GC.THRESHOLD_ROWS)
def test_m_step_across_the_chunk_count_threshold(n):
    """both forms of the chunk-sum kernel (1 and 4 outputs per thread), means and centred second moments"""
    X, resp = GC.threshold_case(n)
    want = GC.m_step(X, resp, 1e-6, "diag")
    got = [_np(t) for t in M.m_step(X, resp, 1e-6, "diag")]
    for q, g, w in zip(("weights", "means", "covariances", "precisions_cholesky"), got, want):
        close(g, w, STEP_TOL, q)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", ["duplicates", "offset"])
def test_steps_special_rows(name, cov_type):
    case = GC.special_case(name, cov_type)
    check_e_step(case, cov_type)
    check_m_step(case, cov_type)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
def test_steps_small_weight(cov_type):
    case = GC.small_weight_case(cov_type)
    check_e_step(case, cov_type)
    check_m_step(case, cov_type)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
def test_steps_empty_component(cov_type):
    """a component that owns no sample: resp exactly 0, nk = 10 eps, mean 0, covariance reg_covar I, no NaN"""
    case = GC.empty_case(cov_type)
    assert np.all(check_e_step(case, cov_type)[2][:, 2] == 0.0)
    weights, means, cov, pchol, log_det = check_m_step(case, cov_type)
    want = GC.m_step(case[0], case[7], 1e-6, cov_type)
    np.testing.assert_allclose(weights[2], want[0][2], rtol=1e-14)
    assert np.all(means[2] == 0.0)
    np.testing.assert_array_equal(cov[2], 1e-6 * np.eye(5) if cov_type == "full" else np.full(5, 1e-6))
    assert all(np.isfinite(a).all() for a in (weights, means, cov, pchol, log_det))


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", ["n33_d5_k3", "n2049_d33_k2", "offset", "small_weight"])
def test_steps_against_sklearn(golden, name, cov_type):
    """the device against sklearn's own values: the step bound plus 4 x the reference-side floor"""
    if name in GC.STEP_CASES:
        case = GC.step_case(name, cov_type)
    else:
        case = GC.small_weight_case(cov_type) if name == "small_weight" else GC.special_case(name, cov_type)
    X, resp = case[0], case[7]
    key = "%s_%s_" % (name, cov_type)
    got = [_np(t) for t in M.e_step(X, golden[key + "weights"], golden[key + "means"], golden[key + "pchol"], cov_type)]
    close(got[0], golden[key + "lpn"], STEP_TOL + 4 * golden[key + "floor_lpn"], "log_prob_norm")
    seen = resp >= 1e-300
    close(got[1], golden[key + "log_resp"], STEP_TOL + 4 * golden[key + "floor_log_resp"], "log_resp", seen)
    got = [_np(t) for t in M.m_step(X, resp, 1e-6, cov_type)]
    for q, g in zip(("m_weights", "m_means", "m_cov", "m_pchol"), got):
        close(g, golden[key + q], STEP_TOL + 4 * golden[key + "floor_" + q], q)


# ---- steps at the library's limits: up to 64 components in 128 dimensions ----------------------------------------------
# STEP_TOL holds unchanged: no sum of these cases is longer than one of the cases above (a chunk is 2048 rows, d = 128
# and 63 chunks are among them); only the number of sums grows.
@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", sorted(GC.LIMIT_CASES))
def test_e_step_at_limits(name, cov_type):
    check_e_step(GC.limit_case(name, cov_type), cov_type)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", sorted(GC.LIMIT_CASES))
def test_m_step_at_limits(name, cov_type):
    check_m_step(GC.limit_m_case(name, cov_type), cov_type)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", GC.LIMIT_GOLDEN)
def test_steps_at_limits_against_sklearn(golden, name, cov_type):
    """the device against sklearn's own values through the reduced quantities of ``GC.limit_reduced``: the step bound
    plus 4 x the reference-side floor"""
    X, weights, means, _, pchol, _, _, _ = GC.limit_case(name, cov_type)
    key = GC.limit_key(name, cov_type)
    got = _np(M.e_step(X, weights, means, pchol, cov_type)[0])
    close(got, golden[key + "lpn"], STEP_TOL + 4 * golden[key + "floor_lpn"], "log_prob_norm")
    got = [_np(t) for t in M.m_step(X, GC.limit_resp(name), 1e-6, cov_type)]
    close(got[4], GC.log_det(got[3], cov_type), STEP_TOL, "log_det of the returned factors")
    for q, g in zip(GC.LIMIT_QUANTITIES, GC.limit_reduced(*got[:4], cov_type)):
        close(g, golden[key + q], STEP_TOL + 4 * golden[key + "floor_" + q], q)


# ---- whole fits ------------------------------------------------------------------------------------------------------
def device_fit(case, **kw):
    name, cov_type, init, run = case
    tol, max_iter = {r[0]: r[1:] for r in GC.FIT_RUNS}[run]
    X, k = GC.FIT_ROWS[name]()
    args = dict(covariance_type=cov_type, tol=tol, max_iter=max_iter)
    if init == "explicit":
        w, mu, prec = GC.explicit_init(X, k, cov_type)
        args.update(weights_init=w, means_init=mu, precisions_init=prec)
    else:
        args.update(init_params=init)
    args.update(kw)
    dtype = args.pop("dtype", None)
    return M.GaussianMixture(k, **args).fit(X if dtype is None else X.astype(dtype)), X


def fitted_arrays(g):
    return dict(weights=g.weights_, means=g.means_, covariances=g.covariances_,
                precisions_cholesky=g.precisions_cholesky_, lower_bound=np.float64(g.lower_bound_))


@pytest.mark.parametrize("case", GC.FIT_CASES, ids=GC.fit_id)
def test_fit(golden, case):
    want = GC.fit_case(*case)
    g, X = device_fit(case)
    key = GC.fit_id(case) + "_"
    print("n_iter %d (restatement %d, sklearn %d)" % (g.n_iter_, want["n_iter"], golden[key + "n_iter"]))
    assert g.n_iter_ == want["n_iter"] == int(golden[key + "n_iter"])
    assert g.converged_ == want["converged"] == bool(golden[key + "converged"])
    got = fitted_arrays(g)
    for q in GC.FIT_QUANTITIES:
        assert got[q].dtype == np.float64
        close(got[q], want[q], FIT_TOL, q + " vs restatement")
        close(got[q], golden[key + q], max(FIT_TOL, 4 * float(golden[key + "floor_" + q])), q + " vs sklearn")
    close(g.lower_bounds_, want["lower_bounds"], FIT_TOL, "lower_bounds_")
    assert len(g.lower_bounds_) == g.n_iter_ and g.lower_bounds_[-1] == g.lower_bound_
    if case[1] == "full":
        np.testing.assert_array_equal(g.covariances_, np.swapaxes(g.covariances_, 1, 2))
        np.testing.assert_array_equal(np.tril(g.precisions_cholesky_, -1), 0.0)
        want_prec = np.array([p @ p.T for p in g.precisions_cholesky_])
    else:
        want_prec = g.precisions_cholesky_ ** 2
    np.testing.assert_array_equal(g.precisions_, want_prec)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
def test_predict_and_statistics(cov_type):
    case = ("blobs300", cov_type, "kmeans", "tol1e-3")
    want = GC.fit_case(*case)
    g, X = device_fit(case)
    labels = GC.predict(X, want, cov_type)                           # asserts the posterior margin
    got = g.predict(X)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, labels)
    np.testing.assert_array_equal(M.GaussianMixture(3, covariance_type=cov_type).fit_predict(X), labels)
    np.testing.assert_array_equal(g.predict(torch.from_numpy(X).cuda()), labels)
    # sklearn's formulas on the fitted parameters
    lpn, _, resp = GC.e_step(X, g.weights_, g.means_, g.precisions_cholesky_, cov_type)
    n, d = X.shape
    close(g.score_samples(X), lpn, STEP_TOL, "score_samples")
    close(g.predict_proba(X), resp, STEP_TOL, "predict_proba")
    np.testing.assert_allclose(g.score(X), lpn.mean(), rtol=1e-12)
    n_par = GC.n_parameters(3, d, cov_type)
    np.testing.assert_allclose(g.bic(X), -2.0 * lpn.mean() * n + n_par * np.log(n), rtol=1e-12)
    np.testing.assert_allclose(g.aic(X), -2.0 * lpn.mean() * n + 2.0 * n_par, rtol=1e-12)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
def test_predict_and_statistics_at_k64(cov_type):
    """the fitted 64-component model: labels wherever the restatement's posterior margin decides them (the CPU test
    holds that it does in 99 % of the rows), sklearn's formulas on the fitted parameters"""
    case = ("k64_d5", cov_type, "kmeans", "tol1e-3")
    want = GC.fit_case(*case)
    g, X = device_fit(case)
    labels, clear = GC.predict(X, want, cov_type, near_ties=0.01)
    got = g.predict(X)
    assert got.dtype == np.int64 and got.shape == labels.shape
    np.testing.assert_array_equal(got[clear], labels[clear])
    assert len(set(got)) == 64
    lpn, _, resp = GC.e_step(X, g.weights_, g.means_, g.precisions_cholesky_, cov_type)
    n, d = X.shape
    close(g.score_samples(X), lpn, FIT_TOL, "score_samples")
    proba = g.predict_proba(X)
    close(proba, resp, FIT_TOL, "predict_proba")
    assert np.abs(proba.sum(axis=1) - 1.0).max() <= 1e-12
    np.testing.assert_allclose(g.score(X), lpn.mean(), rtol=FIT_TOL)
    n_par = GC.n_parameters(64, d, cov_type)
    assert g._n_parameters(d) == n_par
    np.testing.assert_allclose(g.bic(X), -2.0 * lpn.mean() * n + n_par * np.log(n), rtol=FIT_TOL)
    np.testing.assert_allclose(g.aic(X), -2.0 * lpn.mean() * n + 2.0 * n_par, rtol=FIT_TOL)


# ---- run shapes that change no bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
def test_run_shapes_give_identical_bits(cov_type):
    case = ("chunks2100", cov_type, "kmeans", "tol1e-3")
    base, _ = device_fit(case)
    assert base.converged_ and 1 < base.n_iter_ < 100
    runs = [device_fit(case, iter_block=1)[0], device_fit(case, iter_block=3)[0], device_fit(case, iter_block=10)[0],
            device_fit(case)[0], device_fit(case, dtype=np.float64)[0], device_fit(case, dtype=np.float32)[0]]
    for g in runs:
        assert (g.n_iter_, g.converged_) == (base.n_iter_, base.converged_)
        assert g.lower_bounds_ == base.lower_bounds_
        for q, a in fitted_arrays(g).items():
            np.testing.assert_array_equal(a, fitted_arrays(base)[q], err_msg=q)
    # tol = 0 never stops early, whatever the block
    for block in (1, 7):
        g, _ = device_fit(("chunks2100", cov_type, "explicit", "tol0_20"), iter_block=block)
        assert (g.n_iter_, g.converged_) == (20, False)


# ---- the k-means start and n_init ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GC.FIT_ROWS))
def test_kmeans_labels(name):
    X, k = GC.FIT_ROWS[name]()
    rows = GC.seeds(len(X), k)
    want, rounds = GC.kmeans(X, rows)                                # asserts the margin
    got, got_rounds = M.kmeans_labels(X, rows)
    assert got.dtype == np.int64 and got_rounds == rounds
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(M.kmeans_labels(X.astype(np.float64), rows)[0], want)


def test_kmeans_empty_cluster_keeps_its_centre():
    X, rows = GC.empty_cluster_rows()                                # two seeds on the same duplicated row
    want, rounds = GC.kmeans(X, rows, check_margin=False)
    got, got_rounds = M.kmeans_labels(X, rows)
    np.testing.assert_array_equal(got, want)
    assert got_rounds == rounds and np.all(got[:12] == 0) and np.all(got[12:] == 2)


def test_n_init_picks_the_restatements_start():
    X = GC.blobs(400, 3, 5, 9940, spread=2.0)
    rs = np.random.RandomState(7)
    fits = []
    for _ in range(3):
        params = GC.start(X, 4, "full", init_params="random_from_data", random_state=rs)[0]
        fits.append(GC.fit(X, params, "full"))
    bounds = sorted(f["lower_bound"] for f in fits)
    assert bounds[2] - bounds[1] > 1e-6                              # the best start is best by a margin
    best = max(fits, key=lambda f: f["lower_bound"])
    g = M.GaussianMixture(4, init_params="random_from_data", n_init=3, random_state=7).fit(X)
    assert (g.n_iter_, g.converged_) == (best["n_iter"], best["converged"])
    close(g.lower_bound_, best["lower_bound"], FIT_TOL, "lower_bound")
    close(g.means_, best["means"], FIT_TOL, "means")
    single = M.GaussianMixture(4, init_params="random_from_data", n_init=1, random_state=7).fit(X)
    close(single.lower_bound_, fits[0]["lower_bound"], FIT_TOL, "first start")


# ---- error paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
def test_ill_defined_covariance_raises_and_the_device_stays_usable(cov_type):
    """reg_covar = 0 and a component of identical rows (at the origin, so that its mean and its covariance are exactly
    0 in any order of the sums)"""
    X = np.concatenate([np.zeros((20, 3), dtype=np.float32), GC.blobs(60, 3, 1, 9950) + 50.0])
    means = np.array([[0.0, 0.0, 0.0], [50.0, 50.0, 50.0]])
    prec = np.ones((2, 3, 3)) * np.eye(3) if cov_type == "full" else np.ones((2, 3))
    kw = dict(covariance_type=cov_type, weights_init=[0.25, 0.75], means_init=means, precisions_init=prec)
    with pytest.raises(ValueError, match=GC.ILL_DEFINED):
        GC.fit(X, (np.array([0.25, 0.75]), means, prec, prec), cov_type, reg_covar=0.0, check_margin=False)
    with pytest.raises(ValueError, match=GC.ILL_DEFINED):
        M.GaussianMixture(2, reg_covar=0.0, **kw).fit(X)
    with pytest.raises(ValueError, match=GC.ILL_DEFINED):
        M.m_step(X, GC.onehot((np.arange(80) >= 20).astype(int), 2), 0.0, cov_type)
    g = M.GaussianMixture(2, reg_covar=1e-6, **kw).fit(X)                       # the next fit runs
    assert g.converged_ and np.isfinite(g.lower_bound_)
    np.testing.assert_allclose(g.weights_, [0.25, 0.75], rtol=1e-12)


def test_library_refuses_before_any_launch():
    lib = _lib.load()
    X = torch.zeros((8, 2), dtype=torch.float64, device="cuda")
    out = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    ctl = torch.full((16,), 7, dtype=torch.int32, device="cuda")
    p, o, c, st = X.data_ptr(), out.data_ptr(), ctl.data_ptr(), _lib.stream()
    assert lib.ava_gm_e_step(p, 1, 8, 129, 2, 0, o, o, o, o, o, o, o, st) == -1
    assert lib.ava_gm_e_step(p, 1, 8, 2, 9, 0, o, o, o, o, o, o, o, st) == -1                       # K > N
    assert lib.ava_gm_means(p, 1, 8, 2, 2, o, o, o, o, o, 8, st) == -3
    assert lib.ava_gm_m_step(p, 1, 8, 2, 2, 0, o, -1.0, o, o, o, o, o, c, o, 1 << 20, st) == -1
    assert lib.ava_gm_fit(p, 1, 8, 2, 2, 0, o, o, o, o, o, -1.0, 0.0, 0, 1, o, c, o, o, o, o, 1 << 20, st) == -1
    assert lib.ava_gm_fit(p, 1, 8, 2, 2, 1, o, o, o, o, o, 0.0, 0.0, 0, 1, o, c, o, o, o, o, 8, st) == -3
    assert lib.ava_gm_onehot(p, p, 8, 65, o, c, st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ctl == 7).all())
