"""GPU tests of the spectral row (f27): the kernels of csrc/spectral.hip against the numpy restatement of
tests/spectral_cases.py at their edges (components, degrees, the operator, Lanczos steps, the rotation), the solver against
dense spectra and scikit-learn's golden embeddings and labels, the two classes and the opt-in UMAP init."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.sparse
import torch

import projection_cases as PC
import spectral_cases as SC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import projection as P
from ava_amd import spectral as SP

pytestmark = pytest.mark.gpu
TOL = 1e-10
U = SC.U


@pytest.fixture(scope="module")
def golden():
    return load_golden("spectral.npz")


@pytest.fixture(scope="module")
def dense():
    """name -> (lambda, X, dd, c) of every golden graph, made once"""
    out = {}
    for name, _ in SC.EMBED_CASES:
        A = SC.case_graph(name)
        out[name] = SC.dense_spectrum(A) + (SC.components(A)[0],)
    return out


def graph_of(A):
    A = scipy.sparse.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return SP._Graph(A)


# ---- components ------------------------------------------------------------------------------------------------------------
def check_components(A):
    c, labels = graph_of(A).components()
    want_c, want = SC.components(A)
    assert c == want_c
    np.testing.assert_array_equal(labels.cpu().numpy(), want)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 2049])
def test_components_of_a_path(n):
    """one component whose diameter is n - 1: the pointer jumping"""
    check_components(SC.path_graph(n))


@pytest.mark.parametrize("n", [63, 64, 65, 257, 2049])
def test_components_two_halves_linked_by_the_last_row(n):
    A = SC.two_halves_last_edge(n)
    check_components(A)
    cut = A.copy()                                    # a stored zero is no edge: two components
    for i, j in ((n - 1, 1), (1, n - 1)):
        at = cut.indptr[i] + int(np.searchsorted(cut.indices[cut.indptr[i]:cut.indptr[i + 1]], j))
        assert cut.indices[at] == j
        cut.data[at] = 0.0
    assert cut.nnz == A.nnz
    c, labels = graph_of(cut).components()
    assert c == 2 and int(labels[0]) == 0 and int(labels[1]) == 1 and int(labels[n - 1]) == 0


@pytest.mark.parametrize("a, b, iso", [(5, 4, 3), (40, 30, 7), (300, 3, 1025)])
def test_components_cliques_and_isolated_rows(a, b, iso):
    check_components(SC.cliques_and_isolated(a, b, iso))


def test_components_ignore_the_diagonal_and_number_by_smallest_row():
    A = scipy.sparse.lil_matrix((6, 6))
    for i in range(6):
        A[i, i] = 2.0
    A[5, 0] = A[0, 5] = 1.0
    A[4, 2] = A[2, 4] = 1.0
    c, labels = SP.connected_components(scipy.sparse.csr_matrix(A))
    assert c == 4 and list(labels) == [0, 1, 2, 3, 2, 0] and labels.dtype == np.int32


def test_bad_graphs_are_refused_before_they_are_followed():
    lib = _lib.load()
    g = graph_of(SC.path_graph(70))
    ws, nb = g.workspace(1)
    labels = torch.empty(g.n, dtype=torch.int32, device=g.dev)
    count = ctypes.c_int(-7)

    def run(indptr, col, nnz):
        return lib.ava_sp_components(indptr.data_ptr(), col.data_ptr(), g.val.data_ptr(), g.n, nnz, labels.data_ptr(),
                                     ctypes.byref(count), ws.data_ptr(), nb, _lib.stream())

    assert run(g.indptr, g.col, g.nnz) == 0 and count.value == 1
    for bad in (-1, 70, 2 ** 31 - 1):
        col = g.col.clone()
        col[g.nnz - 1] = bad
        assert run(g.indptr, col, g.nnz) == -1
    for at, bad in ((0, 1), (35, 0), (35, g.nnz + 1), (70, g.nnz - 1)):
        indptr = g.indptr.clone()
        indptr[at] = bad
        assert run(indptr, g.col, g.nnz) == -1
    x = torch.zeros(g.n, dtype=torch.float64, device=g.dev)
    col = g.col.clone()
    col[3] = 70
    assert lib.ava_sp_apply(g.indptr.data_ptr(), col.data_ptr(), g.val.data_ptr(), g.dd.data_ptr(), g.n, g.nnz,
                            x.data_ptr(), torch.empty_like(x).data_ptr(), ws.data_ptr(), nb, _lib.stream()) == -1
    assert lib.ava_sp_apply(g.indptr.data_ptr(), g.col.data_ptr(), g.val.data_ptr(), g.dd.data_ptr(), g.n, g.nnz,
                            x.data_ptr(), x.data_ptr(), ws.data_ptr(), nb, _lib.stream()) == -1      # x is y
    assert lib.ava_sp_components(g.indptr.data_ptr(), g.col.data_ptr(), g.val.data_ptr(), g.n, g.nnz, labels.data_ptr(),
                                 ctypes.byref(count), ws.data_ptr(), nb - 1, _lib.stream()) == -3
    b = SP._Basis(g, 8, 1)
    for j0, j1 in ((0, 7), (-1, 2), (3, 2)):                      # 1 + 7 + 1 vectors do not fit in 8
        assert lib.ava_sp_lanczos(g.indptr.data_ptr(), g.col.data_ptr(), g.val.data_ptr(), g.dd.data_ptr(), g.n, g.nnz,
                                  b.V.data_ptr(), 8, 1, j0, j1, 1e-12, b.alpha.data_ptr(), b.beta.data_ptr(),
                                  b.ws.data_ptr(), b.nb, _lib.stream()) == -1
    assert lib.ava_sp_rotate(b.V.data_ptr(), g.n, 8, 9, 2, b.V.data_ptr(), b.ws.data_ptr(), b.nb, _lib.stream()) == -1
    assert lib.ava_sp_rotate(b.V.data_ptr(), g.n, 8, 4, 5, b.V.data_ptr(), b.ws.data_ptr(), b.nb, _lib.stream()) == -1


# ---- degrees and the operator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", [-1, 0, 1])
def test_degrees_and_operator_at_row_lengths_and_chunk_edges(dn):
    n = _lib.load().ava_sp_chunk_rows() + dn
    A = SC.mixed_rows(n, dn + 1)
    off = SC.off_diagonal(A)
    assert list(np.diff(off.indptr)[:6]) == [0, 1, 63, 64, 65, 300] and A.diagonal()[:40].min() > 0.0
    g = graph_of(A)
    deg, dd, bound = SC.degrees(A)
    got_deg, got_dd = g.deg.cpu().numpy(), g.dd.cpu().numpy()
    err = np.abs(got_deg - deg)
    print("degrees: worst error / bound %.3f" % np.max(err / np.maximum(bound, 1e-300)))
    assert (err <= bound).all()
    assert got_deg[0] == 0.0 and got_dd[0] == 1.0
    assert (np.abs(got_dd - np.where(got_deg == 0.0, 1.0, np.sqrt(got_deg))) <= U * got_dd).all()
    x = SC.start_vector(n, 11) * 4.0
    y = g.apply(torch.from_numpy(x).to(g.dev)).cpu().numpy()
    want, ybound = SC.apply_exact(A, got_dd, x)
    err = np.abs(y - want)
    print("operator: worst error / bound %.3f" % np.max(err / np.maximum(ybound, 1e-300)))
    assert (err <= ybound).all() and y[0] == 0.0


# ---- Lanczos steps -------------------------------------------------------------------------------------------------------
def run_steps(g, nlock, labels, j, splits, seed=5):
    """a basis of nlock + j + 1 vectors after the steps [0, j) made in the calls ``splits``"""
    b = SP._Basis(g, nlock + j + 1, nlock)
    if nlock:
        b.null_vectors(labels, nlock)
    b.start(seed)
    for j0, j1 in splits:
        b.lanczos(j0, j1)
    alpha, beta = b.tridiagonal(j)
    return b.V.cpu().numpy(), alpha.copy(), beta.copy()


@pytest.mark.parametrize("name, j", [("wring", 24), ("blobs1", 24), ("ring1023", 20), ("ring1025", 20),
                                     ("ring2049", 36)])
def test_lanczos_steps(name, j):
    A = SC.weighted_ring(int(name[4:]), 2) if name.startswith("ring") else SC.case_graph(name)
    g = graph_of(A)
    c, labels = g.components()
    V, alpha, beta = run_steps(g, c, labels, j, [(0, j)])
    bound = 64 * U * j
    G = V @ V.T
    err = np.abs(G - np.eye(len(G))).max()
    print("%s: orthonormality %.3e, bound %.3e" % (name, err, bound))
    assert err <= bound                                   # the locked vectors are among the rows of V
    M, _ = SC.operator(A)
    Va = V[c:c + j]
    T = Va @ (M @ Va.T)
    want = np.diag(alpha) + np.diag(beta[:j - 1], 1) + np.diag(beta[:j - 1], -1)
    err = np.abs(T - want).max()
    print("%s: V^T M V - T %.3e, bound %.3e" % (name, err, bound))
    assert err <= bound
    assert np.abs(V[:c] @ (M @ Va.T)).max() <= bound      # M leaves the complement of the null space invariant
    V2, alpha2, beta2 = run_steps(g, c, labels, j, [(0, j // 2), (j // 2, j)])
    assert np.array_equal(V, V2) and np.array_equal(alpha, alpha2) and np.array_equal(beta, beta2)


def test_start_vector_is_the_hash_orthogonalised():
    A = SC.case_graph("blobs1")
    g = graph_of(A)
    c, labels = g.components()
    b = SP._Basis(g, c + 1, c)
    b.null_vectors(labels, c)
    norm = b.start(9)
    V = b.V.cpu().numpy()
    N = SC.null_vectors(labels.cpu().numpy(), g.dd.cpu().numpy(), c)
    assert np.abs(V[:c] - N).max() <= g.n * U             # entries below 1, a norm over n terms
    _, beta, v = SC._orth_normalise(N, SC.start_vector(g.n, 9))
    assert abs(norm - beta) <= 64 * U * g.n ** 0.5 and np.abs(V[c] - v).max() <= 64 * U
    b0 = SP._Basis(g, 1, 0)
    b0.start(9)
    w = SC.start_vector(g.n, 9)
    assert np.abs(b0.V.cpu().numpy()[0] - w / np.linalg.norm(w)).max() <= 8 * U


# ---- the rotation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncv", [7, 8, 9, 17])
def test_rotation_at_tile_edges(ncv):
    assert _lib.load().ava_sp_rotate_tile() == 8
    g = graph_of(SC.path_graph(1025))
    rs = np.random.RandomState(ncv)
    for keep in (1, ncv - 1, ncv):
        b = SP._Basis(g, ncv + 2, 1)
        V = rs.normal(size=(ncv + 2, g.n))
        b.V.copy_(torch.from_numpy(V))
        S = rs.normal(size=(ncv, keep))
        b.rotate(ncv, S)
        got = b.V.cpu().numpy()
        want = S.T @ V[1:1 + ncv]
        bound = ncv * U * (np.abs(S).T @ np.abs(V[1:1 + ncv]))
        assert (np.abs(got[1:1 + keep] - want) <= bound).all()
        assert np.array_equal(got[0], V[0]) and np.array_equal(got[1 + keep:], V[1 + keep:])


# ---- the solver ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SC.EMBED_CASES)))
def test_solver_against_dense_and_sklearn(golden, dense, case):
    name, k = SC.EMBED_CASES[case]
    A = SC.case_graph(name)
    lam_dense, _, dd, c = dense[name]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        lam, u = SP.laplacian_eigenmaps(A, k + 1, tol=TOL, drop_first=False)
        lam2, u2 = SP.laplacian_eigenmaps(A, k + 1, tol=TOL, drop_first=False)
        lam3, u3 = SP.laplacian_eigenmaps(A, k, tol=TOL)
    assert (c > 1) == any("Graph is not fully connected" in str(w.message) for w in caught)
    assert np.array_equal(lam, lam2) and np.array_equal(u, u2)            # two runs, bit for bit
    assert np.array_equal(lam3, lam[1:]) and np.array_equal(u3, u[:, 1:])  # drop_first drops the first
    assert u.shape == (A.shape[0], k + 1) and (np.diff(lam) >= 0.0).all()
    SC.check_eigenvalues(lam, lam_dense, A.shape[0], TOL)
    SC.check_embedding(name, k, lam_dense, c, u, golden["e%d_Y" % case], TOL)
    res = SC.residuals(A, lam, u)
    print("%s residuals %s" % (name, res))
    assert (res <= TOL).all()


def test_solver_restarts_and_other_ncv():
    """a small ncv forces thick restarts: the same pairs"""
    A = SC.case_graph("gauss")
    lam_dense = SC.dense_spectrum(A)[0]
    g = SP._Graph(SP._check_graph(A))
    sol = SP._solve(g, 4, TOL, ncv=12, seed=3)
    assert sol.n_restarts > 0 and sol.n_ops > 12
    assert np.abs((1.0 - sol.mu) - lam_dense[:4]).max() <= TOL + 64 * g.n * U
    x = sol.x.cpu().numpy()
    assert np.abs(x @ x.T - np.eye(4)).max() <= 64 * U * sol.n_ops
    with pytest.raises(SP.SpectralConvergenceError):
        SP._solve(g, 4, 1e-13, ncv=8, seed=3, maxiter=20)
    with pytest.raises(ValueError, match="ncv"):
        SP._solve(g, 4, TOL, ncv=4)


@pytest.mark.parametrize("what", ["all_pairs", "room_is_ncv", "isolated_only", "fewer_than_components", "one_row"])
def test_solver_breakdown_cases(what):
    ncv = None
    if what == "all_pairs":                       # n - c = the pairs Lanczos is asked for
        A, k = SC.weighted_ring(6, 1), 6
    elif what == "room_is_ncv":                   # n - c = ncv
        A, k, ncv = SC.weighted_ring(33, 1), 3, 32
    elif what == "isolated_only":
        A, k = scipy.sparse.csr_matrix((7, 7)), 3
    elif what == "fewer_than_components":         # no Lanczos at all
        A, k = SC.cliques_and_isolated(5, 4, 3), 4
    else:
        A, k = scipy.sparse.csr_matrix((1, 1)), 1
    n = A.shape[0]
    lam_dense, _, dd = SC.dense_spectrum(A)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lam, u = SP.laplacian_eigenmaps(A, k, tol=TOL, ncv=ncv, drop_first=False)
    assert np.abs(lam - lam_dense[:k]).max() <= 64 * n * U
    assert (SC.residuals(A, lam, u) <= 64 * n * U).all()
    x = SC.unit(u * dd[:, None])
    assert np.abs(x.T @ x - np.eye(k)).max() <= 64 * n * U
    if what == "isolated_only":
        assert np.array_equal(u, np.eye(7)[:, :3])
    if what == "fewer_than_components":
        c, labels = SC.components(A)
        want = SC.sign_flip((SC.null_vectors(labels, dd, k) / dd[None, :]).T)
        assert np.abs(u - want).max() <= 4 * U


# ---- the classes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SC.CLUSTER_CASES)))
def test_spectral_clustering_equals_sklearn(golden, case):
    name = SC.CLUSTER_CASES[case]
    X, truth, k = SC.cluster_rows(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = SP.SpectralClustering(n_clusters=k, n_neighbors=SC.BLOB_K, random_state=0)
        labels = est.fit_predict(X)
    assert abs(est.affinity_matrix_ - SC.case_graph(name)).nnz == 0
    assert labels.shape == (len(X),) and SC.is_permutation(golden["l%d" % case], labels)
    if name == "blobs0":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            X32 = X.astype(np.float32)
            l32 = SP.SpectralClustering(n_clusters=k, n_neighbors=SC.BLOB_K, random_state=0).fit_predict(X32)
            l64 = SP.SpectralClustering(n_clusters=k, n_neighbors=SC.BLOB_K,
                                        random_state=0).fit_predict(X32.astype(np.float64))
            pre = SP.SpectralClustering(n_clusters=k, affinity='precomputed',
                                        random_state=0).fit_predict(SC.case_graph(name))
        assert np.array_equal(l32, l64) and SC.is_permutation(l32, truth) and SC.is_permutation(pre, truth)


@pytest.mark.parametrize("case", [0, 3, 4])
def test_spectral_embedding_equals_sklearn(golden, dense, case):
    name, k = SC.EMBED_CASES[case]
    A = SC.case_graph(name)
    lam_dense, _, dd, c = dense[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = SP.SpectralEmbedding(n_components=k, affinity='precomputed')
        Y = est.fit_transform(A)
    assert Y.shape == (A.shape[0], k) and est.embedding_ is Y and abs(est.affinity_matrix_ - A).nnz == 0
    bound = (TOL + 1e-12) / SC.gaps(lam_dense, c, k + 1)
    for col in range(c - 1):                                    # in the null space: constant on every component
        _, labels = SC.components(A)
        assert max(np.ptp(Y[labels == comp, col]) for comp in range(c)) <= bound
    for col in range(c - 1, k):
        a, b = SC.unit(SC.sign_flip(Y[:, col:col + 1])), SC.unit(SC.sign_flip(golden["e%d_Y" % case][:, col:col + 1]))
        assert np.linalg.norm(a - b) <= bound
    if name == "blobs0":
        X, _ = SC.case_rows(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Yn = SP.SpectralEmbedding(n_components=k, n_neighbors=SC.BLOB_K).fit_transform(X)
        assert np.array_equal(Yn, Y)


def test_spectral_embedding_of_a_umap_graph():
    X, _ = PC.spiral(n=600, d=16, salt=9300)
    um = P.UMAP(n_epochs=20).fit(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Y = SP.SpectralEmbedding(n_components=2, affinity='precomputed', tol=1e-6).fit_transform(um.graph_)
    assert Y.shape == (600, 2) and np.isfinite(Y).all()


# ---- the UMAP init -----------------------------------------------------------------------------------------------------------
def test_device_init_spans_the_dense_eigenvectors(dense):
    A = SC.case_graph("gauss")
    lam, X, dd, c = dense["gauss"]
    assert c == 1
    n_comp, Y = SP.umap_eigenvectors(A, tol=1e-4)
    gap = min(lam[1] - lam[0], lam[3] - lam[2])
    sine = SC.subspace_sine(X[:, 1:3], Y)
    print("init subspace sine %.3e, bound %.3e" % (sine, 1e-4 / gap))
    assert n_comp == 1 and sine <= 1e-4 / gap
    Y0 = P.init_embedding(A, 'spectral', np.random.RandomState(4), eigen_solver='device')
    assert Y0.shape == (A.shape[0], 2) and Y0.min() == 0.0 and Y0.max() == 10.0
    rs = np.random.RandomState(4)
    Z = Y * (10.0 / np.abs(Y).max()) + rs.normal(scale=0.0001, size=Y.shape)
    assert np.array_equal(Y0, 10.0 * (Z - Z.min(0)) / (Z.max(0) - Z.min(0)))


def test_device_init_of_a_disconnected_graph_is_the_random_init():
    A = SC.case_graph("blobs1")
    with pytest.warns(UserWarning, match="4 connected components: using the random init"):
        dev = P.init_embedding(A, 'spectral', np.random.RandomState(5), eigen_solver='device')
    with pytest.warns(UserWarning, match="4 connected components: using the random init"):
        host = P.init_embedding(A, 'spectral', np.random.RandomState(5))
    assert np.array_equal(dev, host)


def test_umap_with_the_device_init_and_the_unchanged_default():
    X, _ = PC.spiral(n=1500, d=32, salt=9200)
    Y = P.UMAP(eigen_solver='device').fit_transform(X)
    assert Y.shape == (1500, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
    assert np.array_equal(Y, P.UMAP(eigen_solver='device').fit_transform(X))
    tw = PC.trustworthiness(X, Y, 10)
    print("spiral trustworthiness@10 with the device init %.4f" % tw)
    default = P.UMAP().fit_transform(X)
    assert np.array_equal(default, P.UMAP(eigen_solver='scipy').fit_transform(X))
    Yt = P.TransformableUMAP(eigen_solver='device', n_epochs=30).fit(X[:400]).transform(X[400:500])
    assert Yt.shape == (100, 2) and np.isfinite(Yt).all()
