"""ava_amd.projection without a GPU: the numpy restatement (tests/projection_cases.py) against scikit-learn's recorded
outputs (tests/golden/projection.npz), properties of the fuzzy graph and the bandwidth search, (a, b), install() and
argument validation."""
import types

import numpy as np
import pytest
import scipy.sparse

import projection_cases as PC
from conftest import load_golden
from ava_amd import projection as P


@pytest.mark.parametrize("name", sorted(PC.GOLDEN_CASES))
def test_restated_knn_matches_sklearn(name):
    golden = load_golden("projection.npz")
    X, k = PC.golden_input(name)
    idx, dist = PC.knn(X, k)
    np.testing.assert_array_equal(idx, golden[name + "_knn_idx"])
    assert np.all(dist[:, 0] == 0) and np.all(np.diff(dist, axis=1) >= 0)


@pytest.mark.parametrize("name", sorted(PC.PCA_CASES))
def test_restated_pca_matches_sklearn(name):
    """both of sklearn's regimes: covariance_eigh (n >= 10 d) and the full SVD (n < 10 d)"""
    want = load_golden("projection.npz")[name + "_pca"]
    got = PC.pca(PC.pca_input(name))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max())


def test_restated_trustworthiness_matches_sklearn():
    golden = load_golden("projection.npz")
    got = PC.trustworthiness(golden["trust_X"], golden["trust_Y"], n_neighbors=10)
    assert abs(got - float(golden["trust_10"])) < 1e-12


def test_knn_ties_resolve_to_lowest_index():
    X = PC.duplicates()
    idx, dist = PC.knn(X, 20)
    np.testing.assert_array_equal(idx[:, 0], np.arange(len(X)))
    np.testing.assert_array_equal(idx[5, 1:4], [7, 150, 299])
    np.testing.assert_array_equal(idx[40, 1:20], np.arange(41, 60))
    np.testing.assert_array_equal(idx[59, 1:20], np.arange(40, 59))


def test_bandwidth_search_hits_log2_k():
    X, _ = PC.blobs(n=300, d=16, c=3, salt=9130)
    idx, dist = PC.knn(X, 15)
    sigma, rho, w = PC.smooth_knn(idx, dist)
    assert np.all(sigma > 0) and np.all(rho > 0)
    np.testing.assert_allclose(rho, dist[:, 1])                 # local_connectivity 1: the nearest other row
    np.testing.assert_allclose(PC.psum(dist, rho, sigma), np.log2(15), atol=1e-5)
    assert np.all(w[:, 0] == 0) and np.all(w[:, 1] == 1)


def test_fuzzy_union_is_symmetric_and_matches_dense():
    X = PC.duplicates()
    n = len(X)
    idx, dist = PC.knn(X, 20)
    _, rho, w = PC.smooth_knn(idx, dist)
    assert np.any(rho == 0)                                   # the block of equal rows
    for mix in (1.0, 0.7):
        G = P.fuzzy_union(idx, w, n, mix)
        assert scipy.sparse.isspmatrix_csr(G) and G.has_sorted_indices
        assert np.all(G.data != 0)
        D = G.toarray()
        np.testing.assert_array_equal(D, D.T)
        np.testing.assert_allclose(D, PC.fuzzy_union_dense(idx, w, n, mix), rtol=0, atol=1e-15)


def test_ab_params():
    a, b = P.find_ab_params(1.0, 0.1)
    assert abs(a - 1.577) < 1e-3 and abs(b - 0.895) < 1e-3
    assert (a, b) == PC.find_ab_params(1.0, 0.1)


def test_epochs_per_sample():
    w = np.array([1.0, 0.5, 0.25, 0.0])
    np.testing.assert_array_equal(P.epochs_per_sample(w, 200), [1.0, 2.0, 4.0, -1.0])


def test_restated_layout_is_finite_and_spreads_blobs():
    X, labels = PC.blobs(n=300, d=16, c=3, salt=9140)
    idx, dist = PC.knn(X, 15)
    _, _, w = PC.smooth_knn(idx, dist)
    G = PC.prune(P.fuzzy_union(idx, w, len(X)), 200)
    rs = np.random.RandomState(42)
    Y0 = P.init_embedding(G, 'random', rs)
    assert Y0.min() == 0.0 and Y0.max() == 10.0
    a, b = PC.find_ab_params()
    Y = PC.layout(G, Y0, 200, a, b, rs.randint(2 ** 31 - 1))
    assert np.all(np.isfinite(Y))
    assert PC.knn_label_accuracy(Y, labels) == 1.0


def test_init_spectral_and_fallback():
    X, _ = PC.spiral(n=400, d=16, salt=9220)
    idx, dist = PC.knn(X, 15)
    _, _, w = PC.smooth_knn(idx, dist)
    G = P.fuzzy_union(idx, w, len(X))
    Y = P.init_embedding(G, 'spectral', np.random.RandomState(42))
    assert Y.shape == (400, 2) and np.allclose(Y.min(0), 0) and np.allclose(Y.max(0), 10)
    # a disconnected graph falls back to the random init, with a warning
    G2 = scipy.sparse.block_diag([G, G]).tocsr()
    with pytest.warns(UserWarning, match="connected components"):
        Y2 = P.init_embedding(G2, 'spectral', np.random.RandomState(42))
    rs = np.random.RandomState(42)
    want = rs.uniform(-10, 10, (800, 2))
    want = 10 * (want - want.min(0)) / (want.max(0) - want.min(0))
    np.testing.assert_array_equal(Y2, want)


class _DataContainerStub:
    def _make_latent_mean_umap_projection(self):
        return "reference"

    def _make_latent_mean_pca_projection(self):
        return "reference"


def test_install_on_stub_module():
    module = types.SimpleNamespace(DataContainer=_DataContainerStub)
    assert P.install(module) is module
    assert _DataContainerStub._make_latent_mean_umap_projection is P._make_latent_mean_umap_projection
    assert _DataContainerStub._make_latent_mean_pca_projection is P._make_latent_mean_pca_projection


@pytest.mark.parametrize("kwargs, exc", [
    (dict(n_components=3), NotImplementedError),
    (dict(metric='cosine'), NotImplementedError),
    (dict(n_neighbors=1), ValueError),
    (dict(n_neighbors=65), ValueError),
    (dict(init='pca'), ValueError),
    (dict(n_epochs=0), ValueError),
    (dict(negative_sample_rate=8), ValueError),
    (dict(set_op_mix_ratio=1.5), ValueError),
    (dict(min_dist=2.0), ValueError),
])
def test_umap_argument_validation(kwargs, exc):
    with pytest.raises(exc):
        P.UMAP(**kwargs).fit(np.zeros((10, 3), dtype=np.float32))


def test_transform_is_not_supported():
    with pytest.raises(NotImplementedError):
        P.UMAP().transform(np.zeros((10, 3)))
