"""ava_amd.mixture without a GPU: the numpy restatement of tests/gmm_cases.py against scikit-learn's own values
(tests/golden/gmm.npz), its k-means start and stopping rule, the argument checks that need no device and the C ABI's
mirror and refusals.

Bounds: the golden file stores, per case and quantity, the reference-side noise ``floor`` (the larger of |sklearn -
restatement| where the file was written and |sklearn - sklearn on rows perturbed by 1e-15 relative|, relative to
max |sklearn|).  The restatement is held within 4 x that floor, the project's usual margin over reference-side noise;
a floor below 1e-15 (4.5 ulp, the resolution of a stored fp64 result of a few operations) counts as 1e-15, because
another BLAS build may round a sum that happened to agree bit for bit here differently."""

import numpy as np
import pytest

import gmm_cases as GC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import mixture as M

MIN_FLOOR = 1e-15
STEP_GOLDEN = ["n33_d5_k3", "n17_d16_k17", "n2049_d33_k2", "duplicates", "offset", "small_weight", "empty"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("gmm.npz")


def close(got, want, floor, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = 4.0 * max(float(floor), MIN_FLOOR) * np.abs(want[np.isfinite(want)]).max()
    err = np.abs(got - want)[np.isfinite(want)].max()
    print("%s: max err %.2e, bound %.2e" % (what, err, bound))
    assert err <= bound, what


def step_inputs(name, cov_type):
    if name in GC.STEP_CASES:
        return GC.step_case(name, cov_type)
    if name == "empty":
        return GC.empty_case(cov_type)
    if name == "small_weight":
        return GC.small_weight_case(cov_type)
    return GC.special_case(name, cov_type)


# ---- the restatement against sklearn ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", STEP_GOLDEN)
def test_restatement_steps(golden, name, cov_type):
    X = step_inputs(name, cov_type)[0]
    key = "%s_%s_" % (name, cov_type)
    weights, means, pchol = golden[key + "weights"], golden[key + "means"], golden[key + "pchol"]
    lpn, log_resp, resp = GC.e_step(X, weights, means, pchol, cov_type)
    close(lpn, golden[key + "lpn"], golden[key + "floor_lpn"], "log_prob_norm")
    seen = resp >= 1e-300
    close(np.where(seen, log_resp, 0.0), golden[key + "log_resp"], golden[key + "floor_log_resp"], "log_resp")
    np.testing.assert_allclose(resp.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    got = GC.m_step(X, resp, 1e-6, cov_type)
    for q, g in zip(("m_weights", "m_means", "m_cov", "m_pchol"), got):
        close(g, golden[key + q], golden[key + "floor_" + q], q)
    if cov_type == "full":
        np.testing.assert_array_equal(got[2], np.swapaxes(got[2], 1, 2))
        np.testing.assert_array_equal(np.tril(got[3], -1), 0.0)


@pytest.mark.parametrize("case", GC.FIT_CASES, ids=GC.fit_id)
def test_restatement_fits_and_stopping_rule(golden, case):
    fitted = GC.fit_case(*case)                                      # asserts the margin at the stopping threshold
    key = GC.fit_id(case) + "_"
    assert fitted["n_iter"] == int(golden[key + "n_iter"])
    assert fitted["converged"] == bool(golden[key + "converged"])
    for q in GC.FIT_QUANTITIES:
        close(fitted[q], golden[key + q], golden[key + "floor_" + q], q)
    assert len(fitted["lower_bounds"]) == fitted["n_iter"] and fitted["lower_bounds"][-1] == fitted["lower_bound"]


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
def test_fits_at_64_components_are_well_conditioned_and_decided(cov_type):
    """the fitted covariances of the 64-component fits keep cond < 1e3 like the step cases, and the model the statistics
    test predicts with leaves at most 1 % of the rows within the 1e-6 posterior margin"""
    for case in GC.FIT_CASES:
        if case[0] == "k64_d5" and case[1] == cov_type:
            cond = worst_cond(GC.fit_case(*case)["covariances"], cov_type)
            print("%s: cond %.1f" % (GC.fit_id(case), cond))
            assert cond < 1e3, case
    X = GC.fit_start("k64_d5", cov_type, "kmeans")[0]
    labels, clear = GC.predict(X, GC.fit_case("k64_d5", cov_type, "kmeans", "tol1e-3"), cov_type, near_ties=0.01)
    print("rows within the margin: %d of %d" % ((~clear).sum(), len(clear)))
    assert len(set(labels)) == 64


def test_empty_component():
    """a component that owns no sample: nk = 10 eps, mean 0, covariance reg_covar I, nothing is NaN"""
    for cov_type in GC.COV_TYPES:
        X, _, _, _, _, _, _, resp = GC.empty_case(cov_type)
        weights, means, cov, pchol = GC.m_step(X, resp, 1e-6, cov_type)
        assert weights[2] == GC.EPS10 / 300 / ((resp.sum(axis=0) + GC.EPS10) / 300).sum()
        assert np.all(means[2] == 0.0)
        want = 1e-6 * np.eye(5) if cov_type == "full" else np.full(5, 1e-6)
        np.testing.assert_array_equal(cov[2], want)
        assert all(np.isfinite(a).all() for a in (weights, means, cov, pchol))


def worst_cond(cov, cov_type):
    return max(np.linalg.cond(c) for c in cov) if cov_type == "full" else (cov.max(axis=1) / cov.min(axis=1)).max()


def test_step_cases_are_well_conditioned():
    """the GPU tests hold precisions_cholesky within 1e-12 of its largest entry; two factorisations of the same matrix
    differ by a small multiple of cond(C) eps, so the cases keep cond(C) below 1e3 (1e3 eps = 2.2e-13).  At the limits
    that covers the explicit covariances of the E-step and the ones the M-step returns, 'diag' as max / min."""
    for name in GC.STEP_CASES:
        cov = GC.step_case(name, "full")[3]
        assert max(np.linalg.cond(c) for c in cov) < 1e3, name
    for name in GC.LIMIT_CASES:
        for cov_type in GC.COV_TYPES:
            X, _, _, cov, _, _, _, _ = GC.limit_case(name, cov_type)
            given = worst_cond(cov, cov_type)
            returned = worst_cond(GC.m_step(X, GC.limit_resp(name), 1e-6, cov_type)[2], cov_type)
            print("%s %s: cond %.1f (E-step), %.1f (M-step)" % (name, cov_type, given, returned))
            assert given < 1e3 and returned < 1e3, (name, cov_type)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", sorted(GC.LIMIT_CASES))
def test_limit_cases_are_soft(name, cov_type):
    """fitted parameters at 64 components in 128 dimensions leave a one-hot E-step; the explicit ones of the limit
    cases must not: in at least half the rows the second-largest responsibility is above 1e-3, and the M-step's input
    gives every component a share of every row"""
    resp = GC.limit_case(name, cov_type)[7]
    share = float((np.partition(resp, -2, axis=1)[:, -2] > 1e-3).mean())
    print("%s %s: second-largest responsibility above 1e-3 in %.3f of the rows" % (name, cov_type, share))
    assert share >= 0.5
    given = GC.limit_resp(name)
    assert given.shape == resp.shape and given.min() > 0.0
    np.testing.assert_allclose(given.sum(axis=1), 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize("cov_type", GC.COV_TYPES)
@pytest.mark.parametrize("name", sorted(GC.LIMIT_CASES))
def test_restatement_steps_at_limits(golden, name, cov_type):
    """the restatement against sklearn at up to 64 components in 128 dimensions, through the reduced quantities of
    ``GC.limit_reduced`` (the covariances themselves are 8 MB at the corner)"""
    X, _, _, _, _, lpn, _, resp = GC.limit_case(name, cov_type)
    key = GC.limit_key(name, cov_type)
    close(lpn, golden[key + "lpn"], golden[key + "floor_lpn"], "log_prob_norm")
    # log_prob_norm is near -d: its rounding, eps |lpn| / 2 and as much again for the logarithm, scales the row's sum
    np.testing.assert_allclose(resp.sum(axis=1), 1.0, rtol=0, atol=np.finfo(np.float64).eps * max(1.0, np.abs(lpn).max()))
    got = GC.m_step(X, GC.limit_resp(name), 1e-6, cov_type)
    for q, g in zip(GC.LIMIT_QUANTITIES, GC.limit_reduced(*got, cov_type)):
        close(g, golden[key + q], golden[key + "floor_" + q], q)
    if cov_type == "full":
        np.testing.assert_array_equal(got[2], np.swapaxes(got[2], 1, 2))
        np.testing.assert_array_equal(np.tril(got[3], -1), 0.0)


def test_limit_reduced_sees_one_wrong_entry():
    """the reduced quantities move when a single mean or variance does"""
    X = GC.limit_case("k25_d3", "diag")[0]
    weights, means, cov, pchol = GC.m_step(X, GC.limit_resp("k25_d3"), 1e-6, "diag")
    want = GC.limit_reduced(weights, means, cov, pchol, "diag")
    for which, slots in ((1, (1, 2)), (2, (3, 4))):
        arrays = [weights, means.copy(), cov.copy(), pchol]
        arrays[which][7, 2] *= 1.0 + 1e-9
        got = GC.limit_reduced(*arrays, "diag")
        for i, (g, w) in enumerate(zip(got, want)):
            assert (np.abs(g - w).max() > 1e-11 * np.abs(w).max()) == (i in slots), (which, i)


def test_kmeans_restatement():
    X, k = GC.FIT_ROWS["blobs300"]()
    labels, rounds = GC.kmeans(X, GC.seeds(len(X), k))               # asserts the margin between the two nearest centres
    assert 2 <= rounds < GC.KMEANS_MAX_ITER
    # the blobs are well separated: every cluster is one blob
    assert sorted(len(set(labels[np.arange(len(X)) % k == j])) for j in range(k)) == [1] * k
    assert len(set(labels)) == k
    X, k = GC.FIT_ROWS["chunks2100"]()
    labels, rounds = GC.kmeans(X, GC.seeds(len(X), k))
    assert rounds < GC.KMEANS_MAX_ITER and len(set(labels)) == k
    # 64 centres: some blobs hold several seeds and some none, so clusters split and merge, but none runs empty or small
    X, k = GC.FIT_ROWS["k64_d5"]()
    labels, rounds = GC.kmeans(X, GC.seeds(len(X), k))
    assert k == 64 and 2 <= rounds < GC.KMEANS_MAX_ITER and np.bincount(labels, minlength=k).min() >= 15
    # an empty cluster keeps its centre: two seeds on the same duplicated row
    X, rows = GC.empty_cluster_rows()
    labels, rounds = GC.kmeans(X, rows, check_margin=False)
    assert rounds == 2 and np.all(labels[:12] == 0) and np.all(labels[12:] == 2)


# ---- argument checks that need no device -----------------------------------------------------------------------------
def test_not_implemented_branches():
    for kw in (dict(covariance_type="tied"), dict(covariance_type="spherical"), dict(init_params="k-means++"),
               dict(init_params="random"), dict(warm_start=True)):
        with pytest.raises(NotImplementedError):
            M.GaussianMixture(2, **kw)
    with pytest.raises(NotImplementedError):
        M.e_step(np.zeros((4, 2)), np.ones(1), np.zeros((1, 2)), np.ones((1, 2)), covariance_type="tied")


def test_constructor_errors():
    for kw in (dict(tol=-1e-3), dict(reg_covar=-1.0), dict(max_iter=0), dict(n_init=0), dict(iter_block=0),
               dict(covariance_type="banana"), dict(init_params="banana"), dict(n_components=0),
               dict(n_components=M.MAX_K + 1), dict(tol=float("nan"))):
        with pytest.raises(ValueError):
            M.GaussianMixture(**kw)
    g = M.GaussianMixture()
    assert (g.n_components, g.covariance_type, g.tol, g.reg_covar, g.max_iter, g.n_init, g.init_params,
            g.random_state, g.iter_block) == (1, "full", 1e-3, 1e-6, 100, 1, "kmeans", 42, 10)
    assert (M.MAX_D, M.MAX_K, M.CHUNK_ROWS, M.KMEANS_MAX_ITER) == (128, 64, GC.CHUNK, GC.KMEANS_MAX_ITER)


def test_fit_checks_run_before_the_device_is_touched():
    X = GC.blobs(40, 3, 2, 9990)
    cases = [
        (dict(n_components=41), X),                                             # N < K
        (dict(n_components=2), np.where(np.arange(120).reshape(40, 3) == 7, np.nan, X)),
        (dict(n_components=2), np.where(np.arange(120).reshape(40, 3) == 7, np.inf, X)),
        (dict(n_components=2), X[:, 0]),                                        # not 2-D
        (dict(n_components=2), np.zeros((40, M.MAX_D + 1))),
        (dict(n_components=2, weights_init=[0.5, 0.6]), X),
        (dict(n_components=2, weights_init=[1.0]), X),
        (dict(n_components=2, means_init=np.zeros((2, 4))), X),
        (dict(n_components=2, precisions_init=np.zeros((2, 3, 3))), X),
        (dict(n_components=2, precisions_init=np.ones((2, 3))), X),             # 'full' wants [K, d, d]
        (dict(n_components=2, covariance_type="diag", precisions_init=-np.ones((2, 3))), X),
    ]
    for kw, rows in cases:
        with pytest.raises(ValueError):
            M.GaussianMixture(**kw).fit(rows)
    with pytest.raises(ValueError):
        M.GaussianMixture(2).predict(X)                                         # not fitted
    with pytest.raises(ValueError):
        M.m_step(X, np.ones((40, 2)) / 2, reg_covar=-1.0)


def test_n_parameters_matches_sklearn():
    from sklearn.mixture import GaussianMixture as SK
    for cov_type in GC.COV_TYPES:
        sk = SK(3, covariance_type=cov_type)
        sk.means_ = np.zeros((3, 5))
        assert M.GaussianMixture(3, covariance_type=cov_type)._n_parameters(5) == sk._n_parameters() \
            == GC.n_parameters(3, 5, cov_type)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def up256(x):
    return (x + 255) // 256 * 256


def test_library_argument_checks():
    """ava_gm_* return sizes / AVA_EINVAL / AVA_EWORKSPACE before any HIP call"""
    lib = _lib.load()
    assert (lib.ava_gm_max_d(), lib.ava_gm_max_k(), lib.ava_gm_chunk_rows()) == (M.MAX_D, M.MAX_K, M.CHUNK_ROWS)
    for n, d, k, c in ((10, 0, 2, 0), (10, 129, 2, 0), (10, 4, 0, 0), (100, 4, 65, 0), (3, 4, 4, 0), (10, 4, 2, 2),
                       (10, 4, 2, -1)):
        assert lib.ava_gm_workspace_bytes(n, d, k, c) == 0
    for n, d, k in ((5000, 33, 7), (2048, 16, 1), (2049, 128, 64)):
        chunks, dp = -(-n // 2048), 16 * (1 if d <= 16 else 2 if d <= 32 else 4 if d <= 64 else 8)
        common = up256(chunks * k * 8) + up256(chunks * k * d * 8) + up256(chunks * 8) + up256(k * 8) + 256
        assert lib.ava_gm_workspace_bytes(n, d, k, 1) == common
        assert lib.ava_gm_workspace_bytes(n, d, k, 0) == common + up256(chunks * k * dp * dp * 8)
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    big = 1 << 30
    e_ok = [p, 1, 8, 2, 2, 0, p, p, p, p, p, p, p]
    for i, bad in ((0, None), (1, 2), (2, 1), (3, 0), (3, 129), (4, 0), (4, 65), (5, 2), (6, None), (9, None),
                   (12, None)):
        a = list(e_ok)
        a[i] = bad
        assert lib.ava_gm_e_step(*a, None) == -1, (i, bad)
    assert lib.ava_gm_means(p, 1, 8, 2, 2, None, p, p, p, p, big, None) == -1
    assert lib.ava_gm_means(p, 1, 8, 2, 2, p, p, p, p, p, 8, None) == -3
    m_ok = [p, 1, 8, 2, 2, 0, p, 1e-6, p, p, p, p, p, p, p, big]
    for i, bad in ((0, None), (1, -1), (5, 3), (6, None), (7, -1e-6), (7, float("nan")), (13, None), (14, None)):
        a = list(m_ok)
        a[i] = bad
        assert lib.ava_gm_m_step(*a, None) == -1, (i, bad)
    assert lib.ava_gm_m_step(*(m_ok[:15] + [8]), None) == -3
    f_ok = [p, 1, 8, 2, 2, 0, p, p, p, p, p, 1e-3, 1e-6, 0, 10, p, p, p, p, p, p, big]
    for i, bad in ((0, None), (2, 1), (11, -1.0), (12, -1.0), (13, -1), (14, 0), (15, None), (16, None), (19, None),
                   (20, None)):
        a = list(f_ok)
        a[i] = bad
        assert lib.ava_gm_fit(*a, None) == -1, (i, bad)
    assert lib.ava_gm_fit(*(f_ok[:21] + [8]), None) == -3
    assert lib.ava_gm_onehot(None, p, 8, 2, p, p, None) == -1
    assert lib.ava_gm_onehot(p, p, 8, 65, p, p, None) == -1
    assert lib.ava_gm_onehot(p, p, 0, 2, p, p, None) == -1
