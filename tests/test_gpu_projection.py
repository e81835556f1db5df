"""ava_amd.projection on the MI355X: the device kNN, bandwidths, graph and layout against the numpy restatement
(tests/projection_cases.py), reproducibility, the quality of the embeddings, PCA against sklearn's recorded outputs
(tests/golden/projection.npz), and the installed DataContainer methods."""
import warnings

import numpy as np
import pytest
import torch

import projection_cases as PC
from conftest import load_golden
from ava_amd import projection as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(PC.GOLDEN_CASES))
def test_knn_matches_sklearn_and_restatement(name):
    X, k = PC.golden_input(name)
    idx, dist = P.knn(X, k)
    want_idx, want_dist = PC.knn(X, k)
    np.testing.assert_array_equal(idx, load_golden("projection.npz")[name + "_knn_idx"])
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)


@pytest.mark.parametrize("chunk_rows", [None, 1, 7, 197])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_knn_ties_and_chunking(chunk_rows, dtype):
    X = PC.duplicates().astype(dtype)
    idx, dist = P.knn(X, 20, chunk_rows=chunk_rows)
    want_idx, want_dist = PC.knn(X, 20)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)
    ref_idx, ref_dist = P.knn(torch.from_numpy(X).cuda(), 20)          # device input, one launch: same bits
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(dist, ref_dist)


def test_knn_full_k_and_multiple_tiles():
    X = PC.gaussian(2000, 40, 9600)
    idx, dist = P.knn(X, 64, chunk_rows=300)
    want_idx, want_dist = PC.knn(X, 64)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", ["blobs", "duplicates"])
def test_bandwidths_and_graph(case):
    X = PC.blobs(n=2000, d=32, salt=9150)[0] if case == "blobs" else PC.duplicates()
    k = 20
    idx, dist = P.knn(X, k)
    sigma, rho, w = P.smooth_knn(idx, dist)
    want_sigma, want_rho, want_w = PC.smooth_knn(idx, dist)
    np.testing.assert_allclose(rho, want_rho, rtol=1e-12, atol=0)
    np.testing.assert_allclose(sigma, want_sigma, rtol=1e-12, atol=0)
    np.testing.assert_allclose(w, want_w, rtol=0, atol=1e-12)
    model = P.UMAP(n_epochs=1).fit(X)
    np.testing.assert_array_equal(model.sigmas_, sigma)
    np.testing.assert_array_equal(model.rhos_, rho)
    G = model.graph_
    assert G.has_sorted_indices and np.all(G.data != 0)
    D = G.toarray()
    np.testing.assert_array_equal(D, D.T)
    np.testing.assert_allclose(D, PC.fuzzy_union_dense(idx, want_w, len(X)), rtol=0, atol=1e-12)
    G2 = P.UMAP(n_epochs=1).fit(X).graph_
    for a in ("indptr", "indices", "data"):
        np.testing.assert_array_equal(getattr(G2, a), getattr(G, a))


def _layout_case():
    X, _ = PC.blobs(n=2000, d=32, c=5, salt=9160)
    idx, dist = PC.knn(X, 20)
    _, _, w = PC.smooth_knn(idx, dist)
    G = PC.prune(P.fuzzy_union(idx, w, len(X)), 500)
    rs = np.random.RandomState(7)
    Y0 = P.init_embedding(G, 'random', rs)
    return G, Y0, rs.randint(2 ** 31 - 1)


def test_layout_epochs_match_restatement():
    """1 and 3 epochs to 1e-9.  The early epochs are chaotic: a relative change of 1e-15 in the start moves the
    positions by about 1e-6 after 10 epochs (measured on the restatement alone), and the device's pow differs from
    numpy's in the last bit now and then, so 10 epochs are held to 1e-5."""
    G, Y0, salt = _layout_case()
    a, b = P.find_ab_params(1.0, 0.1)
    for epochs, atol in ((1, 1e-9), (3, 1e-9), (10, 1e-5)):
        got = P.Layout(G, Y0, 500, a, b, salt=salt).run(0, epochs).positions()
        want = PC.layout(G, Y0, 500, a, b, salt, epochs=epochs)
        # epoch 0 samples no edge (every edge's first sample is due at its period, >= 1), as in umap-learn
        assert np.array_equal(want, Y0) == (epochs == 1)
        np.testing.assert_allclose(got, want, rtol=0, atol=atol)
    # the same epochs enqueued in pieces give the same bits
    whole = P.Layout(G, Y0, 500, a, b, salt=salt).run(0, 10).positions()
    lay = P.Layout(G, Y0, 500, a, b, salt=salt)
    for e0, e1 in ((0, 1), (1, 4), (4, 10)):
        lay.run(e0, e1)
    np.testing.assert_array_equal(lay.positions(), whole)


def test_fit_transform_is_reproducible():
    X, _ = PC.blobs(n=1500, d=32, salt=9170)
    Y1 = P.UMAP().fit_transform(X)
    Y2 = P.UMAP().fit_transform(X)
    assert Y1.dtype == np.float32 and Y1.shape == (1500, 2) and np.all(np.isfinite(Y1))
    np.testing.assert_array_equal(Y1, Y2)


def test_blobs_quality():
    X, labels = PC.blobs(n=1500, d=32, c=6, salt=9100)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # six separate blobs: the random init
        Y = P.UMAP().fit_transform(X)
    tw = PC.trustworthiness(X, Y, 10)
    print("blobs trustworthiness@10 %.4f" % tw)
    assert tw >= 0.92
    assert PC.knn_label_accuracy(Y, labels, 5) == 1.0


def test_spiral_quality():
    X, _ = PC.spiral(n=1500, d=32, salt=9200)
    Y = P.UMAP().fit_transform(X)
    tw = PC.trustworthiness(X, Y, 10)
    tw_pca = PC.trustworthiness(X, P.pca_projection(X), 10)
    print("spiral trustworthiness@10 umap %.4f pca %.4f" % (tw, tw_pca))
    assert tw >= 0.99 and tw > tw_pca


def test_fit_transform_latent_scale():
    X = PC.gaussian(20000, 32, 9700)
    Y = P.UMAP().fit_transform(X)
    assert Y.shape == (20000, 2) and Y.dtype == np.float32 and np.all(np.isfinite(Y))


def test_small_inputs():
    with pytest.warns(UserWarning, match="n_neighbors"):
        Y = P.UMAP(init='random').fit_transform(PC.gaussian(12, 4, 9710))
    assert Y.shape == (12, 2) and np.all(np.isfinite(Y))
    np.testing.assert_array_equal(P.UMAP().fit_transform(np.ones((1, 5))), np.zeros((1, 2), dtype=np.float32))


@pytest.mark.parametrize("name", sorted(PC.PCA_CASES))
def test_pca_matches_sklearn(name):
    want = load_golden("projection.npz")[name + "_pca"]
    X = PC.pca_input(name)
    got = P.pca_projection(X)
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max())
    np.testing.assert_array_equal(P.pca_projection(torch.from_numpy(X).cuda()), got)


class _DC:
    """stand-in for ava.data.data_container.DataContainer: request(), verbose and _write_projection()"""

    def __init__(self, latent_means):
        self.latent_means = latent_means
        self.verbose = True
        self.requested = []
        self.written = {}

    def request(self, field):
        self.requested.append(field)
        return self.latent_means

    def _write_projection(self, key, data):
        self.written[key] = data


def test_installed_data_container_methods(capsys):
    module = type("data_container", (), {})()
    module.DataContainer = type("DataContainer", (), {})
    P.install(module)
    X = PC.pca_input("latent_f64")
    dc = _DC(X)
    emb = module.DataContainer._make_latent_mean_pca_projection(dc)
    assert dc.requested == ['latent_means'] and dc.written["latent_mean_pca"] is emb
    np.testing.assert_array_equal(emb, P.pca_projection(X))
    emb = module.DataContainer._make_latent_mean_umap_projection(dc)
    assert dc.requested == ['latent_means'] * 2 and dc.written["latent_mean_umap"] is emb
    assert emb.shape == (len(X), 2) and emb.dtype == np.float32
    np.testing.assert_array_equal(emb, P.UMAP().fit_transform(X))
    out = capsys.readouterr().out
    assert "Running PCA..." in out and "Running UMAP... (n=2000)" in out


def test_not_implemented_paths():
    X = PC.gaussian(50, 4, 9720)
    with pytest.raises(NotImplementedError):
        P.UMAP(n_components=3).fit_transform(X)
    with pytest.raises(NotImplementedError):
        P.UMAP(metric='correlation').fit_transform(X)
    with pytest.raises(NotImplementedError):
        P.UMAP().fit(X).transform(X)
