"""CPU-side tests of the spectral row (f27, no GPU needed): the numpy restatement of the solver reproduces the dense
spectra and scikit-learn's embeddings and labels of tests/golden/spectral.npz, the golden cases meet the gap condition,
the argument checks come before any device call, and include/ava_spectral.h and _lib.SP_SIGNATURES mirror each other."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse

import spectral_cases as SC
from conftest import ROOT, load_golden
from ava_amd import _lib
from ava_amd import projection as P
from ava_amd import spectral as SP

TOL = 1e-10


@pytest.fixture(scope="module")
def golden():
    return load_golden("spectral.npz")


@pytest.fixture(scope="module")
def dense():
    """name -> (lambda, X, dd, c) of every golden graph, made once"""
    out = {}
    for name in [c[0] for c in SC.EMBED_CASES] + ["rings"]:
        A = SC.case_graph(name)
        out[name] = SC.dense_spectrum(A) + (SC.components(A)[0],)
    return out


@pytest.fixture(scope="module")
def solved():
    """name -> the restatement's solve of every embedding case with one pair more than sklearn returns"""
    return {name: SC.Solve(SC.case_graph(name), k + 1, tol=TOL) for name, k in SC.EMBED_CASES}


@pytest.mark.parametrize("case", range(len(SC.EMBED_CASES)))
def test_restatement_eigenvalues_equal_dense(dense, solved, case):
    name, k = SC.EMBED_CASES[case]
    lam, _, _, c = dense[name]
    assert solved[name].n_comp == c
    SC.check_eigenvalues(solved[name].lam, lam, len(lam), TOL)


@pytest.mark.parametrize("case", range(len(SC.EMBED_CASES)))
def test_gap_condition(dense, case):
    name, k = SC.EMBED_CASES[case]
    lam, _, _, c = dense[name]
    assert SC.gaps(lam, c, k + 1) >= SC.MIN_GAP
    assert np.abs(lam[:c]).max() <= 64 * len(lam) * SC.U and lam[c] > SC.MIN_GAP


@pytest.mark.parametrize("case", range(len(SC.EMBED_CASES)))
def test_restatement_embedding_equals_sklearn(golden, dense, solved, case):
    name, k = SC.EMBED_CASES[case]
    lam, _, _, c = dense[name]
    got_lam, u = solved[name].embedding(drop_first=False)
    SC.check_embedding(name, k, lam, c, u, golden["e%d_Y" % case], TOL)


def test_restatement_without_locking_would_miss_the_null_space(dense):
    """why the null space is locked: the residual test alone accepts pairs of a disconnected graph that are not the
    smallest ones; the restatement with the locking returns the dense values"""
    lam, _, _, c = dense["blobs1"]
    assert c == 4
    s = SC.Solve(SC.case_graph("blobs1"), 6)
    assert np.abs(s.lam[:4]).max() == 0.0 and np.abs(s.lam - lam[:6]).max() <= TOL + 64 * 300 * SC.U


@pytest.mark.parametrize("n, ncomp", [(5, 5), (7, 3), (40, 39)])
def test_restatement_breakdown_is_exact(n, ncomp):
    """n - c <= ncv: the Krylov space is the whole complement"""
    A = SC.weighted_ring(n, 3)
    lam = SC.dense_spectrum(A)[0]
    s = SC.Solve(A, ncomp)
    assert s.n_restarts == 0 and np.abs(s.lam - lam[:ncomp]).max() <= 64 * n * SC.U


@pytest.mark.parametrize("case", range(len(SC.CLUSTER_CASES)))
def test_restatement_labels_equal_sklearn(golden, case):
    name = SC.CLUSTER_CASES[case]
    X, truth, k = SC.cluster_rows(name)
    assert SC.is_permutation(golden["l%d" % case], truth)          # sklearn recovers the truth: ARI 1.0
    _, u = SC.Solve(SC.case_graph(name), k).embedding(drop_first=False)
    assert SC.is_permutation(golden["l%d" % case], SC.lloyd(u, k))


def test_components_restatement_numbers_by_smallest_row():
    A = SC.cliques_and_isolated(5, 4, 3)
    c, lab = SC.components(A)
    assert c == 5 and list(lab) == [0] * 5 + [1, 2, 3] + [4] * 4
    A = SC.two_halves_last_edge(65)
    assert SC.components(A)[0] == 1
    B = scipy.sparse.lil_matrix(A)
    B[64, 1] = B[1, 64] = 0.0
    c, lab = SC.components(scipy.sparse.csr_matrix(B))
    assert c == 2 and lab[0] == 0 and lab[1] == 1 and lab[64] == 0


def test_start_vector_is_counter_based():
    a, b = SC.start_vector(100, 7), SC.start_vector(300, 7)
    assert np.array_equal(a, b[:100]) and not np.array_equal(a, SC.start_vector(100, 8))
    assert np.abs(a).max() <= 0.5 and abs(a.mean()) < 0.1


def test_projected_matrix_mirror():
    """the package's host helpers against the restatement's"""
    rs = np.random.RandomState(0)
    theta, s, alpha, beta = rs.normal(size=3), rs.normal(size=3), rs.normal(size=9), rs.normal(size=9)
    for k, m in ((0, 9), (3, 9), (3, 4)):
        assert np.array_equal(SP.projected_matrix(theta, s, alpha, beta, k, m),
                              SC.projected_matrix(theta, s, alpha, beta, k, m))
    assert SP.restart_size(64, 2) == 33 and SP.BREAKDOWN == SC.BREAKDOWN and SP.default_ncv(2) == 64
    assert SP.default_ncv(40) == 81


def test_golden_file_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "spectral.npz")) < 300 * 1024


# ---- argument checks: all of them before any device call (this machine has no GPU, a device call would raise
# AvaHipError) -------------------------------------------------------------------------------------------------------------
def test_argument_checks_come_first():
    A = SC.path_graph(6)
    with pytest.raises(ValueError, match="n_components"):
        SP.laplacian_eigenmaps(A, 0)
    with pytest.raises(ValueError, match="n_components"):
        SP.laplacian_eigenmaps(A, 7, drop_first=False)
    with pytest.raises(ValueError, match="n_components"):
        SP.laplacian_eigenmaps(A, 6)                               # drop_first needs one more
    with pytest.raises(ValueError, match="tol"):
        SP.laplacian_eigenmaps(A, 2, tol=-1.0)
    with pytest.raises(ValueError, match="ncv"):
        SP.laplacian_eigenmaps(A, 2, ncv=0)
    with pytest.raises(ValueError, match="square"):
        SP.laplacian_eigenmaps(scipy.sparse.csr_matrix(np.ones((3, 4))), 1)
    with pytest.raises(ValueError, match="square"):
        SP.connected_components(np.ones(5))
    with pytest.raises(ValueError, match="NaN"):
        SP.connected_components(np.array([[0.0, np.nan], [np.nan, 0.0]]))
    X = np.zeros((30, 4))
    with pytest.raises(ValueError, match="The 'n_clusters' parameter of SpectralClustering must be an int in the range"):
        SP.SpectralClustering(n_clusters=0).fit(X)
    with pytest.raises(ValueError, match="The 'n_init' parameter of SpectralClustering"):
        SP.SpectralClustering(n_clusters=2, n_init=0).fit(X)
    with pytest.raises(ValueError, match="The 'n_neighbors' parameter of SpectralClustering"):
        SP.SpectralClustering(n_clusters=2, n_neighbors=0).fit(X)
    with pytest.raises(ValueError, match="The 'n_components' parameter of SpectralEmbedding"):
        SP.SpectralEmbedding(n_components=0).fit(X)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        SP.SpectralClustering(n_clusters=2, n_neighbors=31).fit(X)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        SP.SpectralEmbedding(n_neighbors=P.MAX_K + 1).fit(np.zeros((200, 4)))
    with pytest.raises(ValueError, match="The 'affinity' parameter"):
        SP.SpectralEmbedding(affinity='cosine').fit(X)
    with pytest.raises(ValueError, match="eigen_solver"):
        P.init_embedding(A, 'spectral', np.random.RandomState(0), eigen_solver='lobpcg')
    with pytest.raises(ValueError, match="eigen_solver"):
        P.UMAP(eigen_solver='arpack').fit(X)


@pytest.mark.parametrize("make, option", [
    (lambda: SP.SpectralClustering(2, eigen_solver='lobpcg'), "lobpcg"),
    (lambda: SP.SpectralClustering(2, eigen_solver='amg'), "amg"),
    (lambda: SP.SpectralEmbedding(2, eigen_solver='amg'), "amg"),
    (lambda: SP.SpectralClustering(2, assign_labels='discretize'), "discretize"),
    (lambda: SP.SpectralClustering(2, assign_labels='cluster_qr'), "cluster_qr"),
    (lambda: SP.SpectralClustering(2, affinity='rbf'), "rbf"),
    (lambda: SP.SpectralEmbedding(2, affinity='rbf'), "rbf"),
])
def test_options_not_on_the_device_are_named(make, option):
    with pytest.raises(NotImplementedError, match=option):
        make().fit(np.zeros((30, 4)))


def test_asymmetric_graph_warns_as_sklearn(monkeypatch):
    A = scipy.sparse.csr_matrix(np.array([[0.0, 1.0, 0.0], [0.5, 0.0, 1.0], [0.0, 1.0, 0.0]]))
    with pytest.warns(UserWarning, match="Array is not symmetric"):
        B = SP._check_graph(A)
    assert abs(B - B.T).nnz == 0 and B[0, 1] == 0.75


def test_no_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.AvaHipError):
        SP.laplacian_eigenmaps(SC.path_graph(6), 2)
    with pytest.raises(_lib.AvaHipError):
        SP.connected_components(SC.path_graph(6))
    with pytest.raises(_lib.AvaHipError):
        P.init_embedding(SC.path_graph(6), 'spectral', np.random.RandomState(0), eigen_solver='device')


def test_default_init_is_the_scipy_path():
    """the default keyword is the parent's code path: the same array as the explicit keyword, bit for bit"""
    A = SC.case_graph("wring")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = P.init_embedding(A, 'spectral', np.random.RandomState(3))
        b = P.init_embedding(A, 'spectral', np.random.RandomState(3), eigen_solver='scipy')
    Y = P._spectral(A)
    rs = np.random.RandomState(3)
    Y = Y * (10.0 / np.abs(Y).max()) + rs.normal(scale=0.0001, size=[A.shape[0], 2])
    want = 10.0 * (Y - Y.min(0)) / (Y.max(0) - Y.min(0))
    assert np.array_equal(a, b) and np.array_equal(a, want)
    assert P.UMAP().eigen_solver == 'scipy' and P.TransformableUMAP().eigen_solver == 'scipy'
    assert P.TransformableUMAP(eigen_solver='device').eigen_solver == 'device'


# ---- the header and its mirror ---------------------------------------------------------------------------------------------
def test_header_and_signatures_mirror_each_other():
    scalar = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64,
              "uint64_t": ctypes.c_uint64}
    header = open(os.path.join(ROOT, "include", "ava_spectral.h")).read()
    decls = re.findall(r"^((?:const )?\w+\s*\*?)\s*(ava_[a-z0-9_]+)\(([^;{]*)\);", header, flags=re.M)
    assert sorted(d[1] for d in decls) == sorted(_lib.SP_SIGNATURES) and len(decls) == 12
    assert all(name.startswith("ava_sp_") for name in _lib.SP_SIGNATURES)
    assert not set(_lib.SP_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EQ_SIGNATURES))
    assert '#include "ava_spectral.h"' in open(os.path.join(ROOT, "include", "ava_hip.h")).read()

    def mirrors(ctype, got):
        ctype = ctype.replace("const ", "").strip()
        if ctype == "ava_stream_t":
            return got is ctypes.c_void_p
        if ctype.endswith("*"):
            pointee = ctype[:-1].strip()
            return got is ctypes.c_void_p or (pointee in scalar and got is ctypes.POINTER(scalar[pointee]))
        return got is scalar[ctype]

    for res, name, args in decls:
        got_res, got_args = _lib.SP_SIGNATURES[name]
        assert mirrors(" ".join(res.split()), got_res), name
        want = [] if args.strip() == "void" else [" ".join(a.split()) for a in args.split(",")]
        assert len(got_args) == len(want), name
        for arg, got in zip(want, got_args):
            m = re.fullmatch(r"(.*?)\s*\b\w+(\[\d*\])?", arg)
            assert mirrors(m.group(1) + ("*" if m.group(2) else ""), got), (name, arg)
    lib = _lib.load()
    for name in _lib.SP_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.ava_sp_max_basis() == SP.MAX_BASIS and lib.ava_sp_max_n() == SP.MAX_N
    assert lib.ava_sp_workspace_bytes(0, 4) == 0 and lib.ava_sp_workspace_bytes(100, SP.MAX_BASIS + 1) == 0
    assert lib.ava_sp_workspace_bytes(100, 8) > 0
