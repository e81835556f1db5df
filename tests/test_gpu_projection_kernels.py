"""The kernels of csrc/projection.hip on the MI355X, one by one, at the shapes where their code takes another path:
the Gram kernel's row chunks and tiles, the projection at several component counts, the kNN kernel at its smallest and
fullest lists (and bit for bit against the other users of csrc/sqdist_tile.h), the bandwidth kernel at every branch of
local_connectivity, and the layout kernel's clamp, coincident points, isolated vertices and single partial workgroup.
The oracles are the fp64 / long double numpy restatements of tests/projection_cases.py; tests/test_cpu_projection.py
shows that the inputs are well conditioned at the tolerances used here."""
import functools
import warnings

import numpy as np
import pytest
import torch

import projection_cases as PC
from ava_amd import _lib
from ava_amd import neighbors as N
from ava_amd import projection as P

pytestmark = pytest.mark.gpu

AVA_OK, AVA_EINVAL, AVA_EWORKSPACE = 0, -1, -3
DTYPES = {"float32": np.float32, "float64": np.float64}


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _code(a):
    return 0 if a.dtype == np.float32 else 1


# ---- Gram ------------------------------------------------------------------------------------------------------------
# (n, d, row chunks, dtypes)
GRAM_CASES = [
    (3, 1, 1, ("float32", "float64")),                   # minimum
    (2048, 32, 1, ("float32", "float64")),               # exactly one chunk
    (2049, 32, 2, ("float32", "float64")),               # second chunk of one row
    (4159, 31, 3, ("float32", "float64")),               # D = 32: one tile exactly; ragged last 64-row stage
    (5000, 128, 3, ("float32", "float64")),              # D = 129: 5 x 5 tiles
    (70, 512, 1, ("float32", "float64")),                # the cap: 17 x 17 tiles
    (600001, 2, 254, ("float32",)),                      # rows_per_chunk = 2368 > 2048
]
GRAM_PARAMS = [pytest.param(n, d, chunks, dt, id="%dx%d-%s" % (n, d, dt))
               for n, d, chunks, dts in GRAM_CASES for dt in dts]


@functools.lru_cache(maxsize=None)
def _gram_case(n, d, dtype):
    """(X, want, absgram, last row of [X, 1] as long double); columns of different scales, none centred"""
    X = (PC.gaussian(n, d, 9900 + d, np.float64) * (1.0 + np.arange(d) % 7) + 0.5).astype(DTYPES[dtype])
    want, absgram = PC.gram(X)
    z = np.append(X[-1].astype(np.float64), 1.0).astype(np.longdouble)
    for a in (want, absgram, z):                          # shared by the tests: not to be changed
        a.setflags(write=False)
    return X, want, absgram, z


def _gram_device(xd, n, d, poison):
    lib = _lib.load()
    nbytes = lib.ava_pj_gram_workspace_bytes(n, d)
    ws = torch.full((nbytes,), poison, dtype=torch.uint8, device="cuda")
    gram = torch.full((d + 1, d + 1), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.ava_pj_gram(xd.data_ptr(), 0 if xd.dtype == torch.float32 else 1, n, d, gram.data_ptr(), ws.data_ptr(),
                         nbytes, _lib.stream())
    assert rc == AVA_OK
    return gram.cpu().numpy(), nbytes


@pytest.mark.parametrize("n, d, chunks, dtype", GRAM_PARAMS)
def test_gram(n, d, chunks, dtype):
    X, want, absgram, z = _gram_case(n, d, dtype)
    xd = _up(X)
    got, nbytes = _gram_device(xd, n, d, 0)
    assert nbytes == chunks * (d + 1) ** 2 * 8
    bound = PC.gram_bound(n, absgram)
    err = np.abs(got.astype(np.longdouble) - want)
    print("gram %dx%d %s: max err / bound %.3g" % (n, d, dtype, float((err / bound).max())))
    assert np.all(np.isfinite(got)) and np.all(err <= bound)
    np.testing.assert_array_equal(got, got.T)
    assert got[d, d] == n
    # the partial sums leave nothing behind: another call, over a workspace of NaN bit patterns, gives the same bits
    np.testing.assert_array_equal(_gram_device(xd, n, d, 0xFF)[0], got)
    # sensitivity: the Gram matrix of all rows but the last is outside the bound
    assert not np.all(np.abs(got.astype(np.longdouble) - (want - np.outer(z, z))) <= bound)


def test_gram_host_validation():
    lib = _lib.load()
    n, d = 2049, 32
    x = torch.zeros((n, d), dtype=torch.float64, device="cuda")
    need = lib.ava_pj_gram_workspace_bytes(n, d)
    assert need == 2 * 33 * 33 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    gram = torch.full((d + 1, d + 1), 7.0, dtype=torch.float64, device="cuda")
    st = _lib.stream()
    assert lib.ava_pj_gram(x.data_ptr(), 1, n, d, gram.data_ptr(), ws.data_ptr(), need - 1, st) == AVA_EWORKSPACE
    assert lib.ava_pj_gram_workspace_bytes(n, 513) == 0
    assert lib.ava_pj_gram(x.data_ptr(), 1, n, 513, gram.data_ptr(), ws.data_ptr(), need, st) == AVA_EINVAL
    assert lib.ava_pj_gram_workspace_bytes(n, 512) == 2 * 513 * 513 * 8
    assert bool((gram == 7.0).all())                      # nothing was launched


# ---- projection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("n, d, nc", [(1, 1, 1), (257, 5, 5), (1000, 32, 3), (3000, 128, 128)])
def test_project(n, d, nc, dtype):
    X = (PC.gaussian(n, d, 9910 + d, np.float64) * 3.0 + 0.5).astype(DTYPES[dtype])
    V = PC.gaussian(nc, d, 9911 + d, np.float64)
    muv = PC.gaussian(1, nc, 9912 + d, np.float64).ravel()
    L = np.longdouble
    want = X.astype(L) @ V.T.astype(L) - muv.astype(L)
    bound = (d + 2) * 2.0 ** -53 * (np.abs(X.astype(np.float64)) @ np.abs(V.T) + np.abs(muv))
    xd, Vd, mud = _up(X), _up(V), _up(muv)
    out = torch.full((n, nc), float("nan"), dtype=torch.float64, device="cuda")
    rc = _lib.load().ava_pj_project(xd.data_ptr(), _code(X), n, d, Vd.data_ptr(), mud.data_ptr(), nc, out.data_ptr(),
                                    _lib.stream())
    assert rc == AVA_OK
    got = out.cpu().numpy()
    err = np.abs(got.astype(L) - want)
    print("project %dx%d nc %d %s: max err / bound %.3g" % (n, d, nc, dtype, float((err / bound).max())))
    assert np.all(np.isfinite(got)) and np.all(err <= bound)


# ---- PCA end to end --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.PCA_KERNEL_CASES))
def test_pca_multi_chunk(name):
    X = PC.pca_input(name)
    want = PC.pca(X)
    got = P.pca_projection(X)
    assert got.dtype == np.float64 and got.shape == want.shape == (len(X), 2)
    print("pca %s: max err %.3g max|want|" % (name, np.abs(got - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max())
    np.testing.assert_array_equal(P.pca_projection(_up(X)), got)


# ---- kNN -------------------------------------------------------------------------------------------------------------
KNN_CASES = {
    "5x1-k5": (5, 1, 5),              # d = 1; k = n; n < 64
    "5x3-k1": (5, 3, 1),              # k = 1: no list, no dynamic LDS
    "63x33-k2": (63, 33, 2),          # one-slot list; a column stage with a tail of 1
    "64x32-k64": (64, 32, 64),        # exactly one tile, one stage; k = n = the cap
    "65x65-k20": (65, 65, 20),        # a second workgroup and reference tile of one row; 2 column stages and 1 more
    "130x64-k64": (130, 64, 64),      # the full list over three tiles
    "duplicates64-k64": None,         # ties across a full list
}


@functools.lru_cache(maxsize=None)
def _knn_case(name):
    if KNN_CASES[name] is None:
        X, k = PC.duplicates()[:64], 64
    else:
        n, d, k = KNN_CASES[name]
        X = PC.gaussian(n, d, 9920 + n + d)
    want_idx, want_dist = PC.knn(X, k)
    for a in (want_idx, want_dist):
        a.setflags(write=False)
    return X, k, want_idx, want_dist


@pytest.mark.parametrize("chunk_rows", [None, 5])
@pytest.mark.parametrize("name", sorted(KNN_CASES))
def test_knn_edges(name, chunk_rows):
    X, k, want_idx, want_dist = _knn_case(name)
    idx, dist = P.knn(X, k, chunk_rows=chunk_rows)
    assert idx.shape == dist.shape == (len(X), k)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)
    if k == len(X):                                       # every row lists every row once
        np.testing.assert_array_equal(np.sort(idx, axis=1), np.broadcast_to(np.arange(k), idx.shape))


# ---- one squared-distance tile (csrc/sqdist_tile.h) behind nearest, knn and knn_query --------------------------------
def _check_nearest_is_knn_query(Q, X):
    idx, dist = N.nearest(Q, X, 'euclidean')
    qidx, qdist = P.knn_query(Q, X, 1)
    np.testing.assert_array_equal(idx, qidx[:, 0])
    np.testing.assert_array_equal(dist, qdist[:, 0])
    return idx, dist


# a partial tile; a second tile of one row and a column stage with a tail of 1; three reference tiles, two full stages
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("m, n, d", [(5, 7, 1), (63, 65, 33), (65, 130, 64)])
def test_nearest_equals_knn_query_k1(m, n, d, dtype):
    Q = PC.gaussian(m, d, 9950 + m + d, DTYPES[dtype])
    X = PC.gaussian(n, d, 9951 + n + d, DTYPES[dtype])
    _check_nearest_is_knn_query(Q, X)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_nearest_equals_knn_query_k1_duplicates(dtype):
    """references 3 and 70 (another tile) are copies of query 2, references 64 and 129 of query 64: distance 0 twice,
    and both searches take the lower index"""
    Q = PC.gaussian(65, 33, 9960, DTYPES[dtype])
    X = PC.gaussian(130, 33, 9961, DTYPES[dtype])
    X[[3, 70]] = Q[2]
    X[[64, 129]] = Q[64]
    idx, dist = _check_nearest_is_knn_query(Q, X)
    assert idx[2] == 3 and idx[64] == 64 and dist[2] == 0.0 and dist[64] == 0.0


def test_knn_equals_knn_query_on_same_rows():
    """the self search and the query search of the same rows: the row itself first at 0.0, then (the case has no ties)
    the same neighbours at the same distances, bit for bit"""
    X, k, _, _ = _knn_case("65x65-k20")
    idx, dist = P.knn(X, k)
    qidx, qdist = P.knn_query(X, X, k)
    np.testing.assert_array_equal(qidx[:, 0], np.arange(len(X)))
    np.testing.assert_array_equal(qdist[:, 0], np.zeros(len(X)))
    np.testing.assert_array_equal(qidx[:, 1:], idx[:, 1:])
    np.testing.assert_array_equal(qdist[:, 1:], dist[:, 1:])


def test_knn_query_equals_pair_sqdist():
    """the tile's sum over k is the scalar kernel's: knn_query distances are the square roots of ava_pair_sqdist (called
    as mmd.estimate_median_sigma calls it) of the same index pairs, bit for bit"""
    n, z, k = 65, 33, 5
    X = PC.gaussian(n, z, 9970, np.float64)
    qidx, qdist = P.knn_query(X, X, k)
    L, a, b = _up(X), _up(np.repeat(np.arange(n, dtype=np.int64), k)), _up(qidx.ravel())
    out = torch.empty(n * k, dtype=torch.float64, device="cuda")
    rc = _lib.load().ava_pair_sqdist(L.data_ptr(), z, a.data_ptr(), b.data_ptr(), n * k, out.data_ptr(), _lib.stream())
    assert rc == AVA_OK
    np.testing.assert_array_equal(np.sqrt(out.cpu().numpy()).reshape(n, k), qdist)
    assert np.all(qdist[:, 1:] > 0)


# ---- bandwidths ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(case, k):
    X = PC.blobs(n=300, d=16, c=3, salt=9930)[0] if case == "blobs" else PC.duplicates()
    idx, dist = PC.knn(X, k)
    return X, idx, dist


def _check_bandwidths(idx, dist, lc):
    sigma, rho, w = P.smooth_knn(idx, dist, lc)
    want_sigma, want_rho, want_w = PC.smooth_knn(idx, dist, lc)
    np.testing.assert_allclose(rho, want_rho, rtol=1e-12, atol=0)
    np.testing.assert_allclose(sigma, want_sigma, rtol=1e-12, atol=0)
    np.testing.assert_allclose(w, want_w, rtol=0, atol=1e-12)
    return sigma, rho


@pytest.mark.parametrize("lc", [0.0, 0.5, 1.5, 2.0, 3.0])
@pytest.mark.parametrize("case", ["blobs", "duplicates"])
def test_bandwidths_local_connectivity(case, lc):
    _, idx, dist = _table(case, 20)
    _, rho = _check_bandwidths(idx, dist, lc)
    if case == "duplicates":                              # 20 equal rows: no nonzero distance among their 19 nearest
        assert np.all(rho[40:60] == 0)
    elif lc == 0.0:
        assert np.all(rho == 0)
    else:
        assert np.all(rho > 0)


@pytest.mark.parametrize("k", [2, 5, 64])
def test_bandwidths_list_lengths(k):
    _, idx, dist = _table("blobs", k)
    _check_bandwidths(idx, dist, 1.0)


def test_umap_passes_local_connectivity():
    X, _, _ = _table("blobs", 20)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # separate blobs: the random init
        model = P.UMAP(n_epochs=1, local_connectivity=1.5).fit(X)
    idx, dist = P.knn(X, 20)
    sigma, rho = _check_bandwidths(idx, dist, 1.5)
    np.testing.assert_array_equal(model.sigmas_, sigma)
    np.testing.assert_array_equal(model.rhos_, rho)
    assert not np.array_equal(rho, P.smooth_knn(idx, dist, 1.0)[1])


# ---- layout ----------------------------------------------------------------------------------------------------------
N_EPOCHS = 12


@functools.lru_cache(maxsize=None)
def _edge_case():
    G = PC.layout_edge_graph(N_EPOCHS)
    Y0, _ = PC.layout_edge_start(G)
    return G, Y0, PC.find_ab_params()


def _check_layout(G, Y0, isolated, **kwargs):
    _, _, (a, b) = _edge_case()
    for epochs in (1, 3):
        got = P.Layout(G, Y0, N_EPOCHS, a, b, salt=PC.LAYOUT_SALT, **kwargs).run(0, epochs).positions()
        want = PC.layout(G, Y0, N_EPOCHS, a, b, PC.LAYOUT_SALT, epochs=epochs, **kwargs)
        assert np.all(np.isfinite(got))
        assert np.array_equal(want, Y0) == (epochs == 1)      # epoch 0 samples nothing; epochs 1 and 2 move
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
        np.testing.assert_array_equal(got[isolated], Y0[isolated])


def test_layout_coincident_points_and_isolated_vertices():
    G, Y0, _ = _edge_case()
    _check_layout(G, Y0, PC.LAYOUT_ISOLATED)


def test_layout_gamma_learning_rate_and_sample_rate():
    G, Y0, _ = _edge_case()
    _check_layout(G, Y0, PC.LAYOUT_ISOLATED, gamma=2.0, learning_rate=0.5, negative_sample_rate=1)


def test_layout_single_partial_workgroup():
    G, Y0, _ = _edge_case()
    _check_layout(PC.induced(G, 40, N_EPOCHS), Y0[:40], [v for v in PC.LAYOUT_ISOLATED if v < 40])


def test_layout_clamps_negative_samples_and_flags():
    """negative_sample_rate = 40 (Layout takes it; UMAP refuses it): a period-1 edge is due 39 samples in epoch 1.  The
    kernel draws 16, advances the counter by 16 and raises the flag, which is a status word: the positions are those
    of the capped restatement, positions() refuses them, and the device goes on working."""
    G, Y0, (a, b) = _edge_case()
    lay = P.Layout(G, Y0, N_EPOCHS, a, b, negative_sample_rate=40, salt=PC.LAYOUT_SALT).run(0, 3)
    want, flagged = PC.layout(G, Y0, N_EPOCHS, a, b, PC.LAYOUT_SALT, epochs=3, negative_sample_rate=40, cap=True)
    assert flagged
    got = lay.y.cpu().numpy()
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    assert int(lay.flag.item()) == 1
    with pytest.raises(_lib.AvaHipError, match="negative samples"):
        lay.positions()
    torch.cuda.synchronize()
    ok = P.Layout(G, Y0, N_EPOCHS, a, b, salt=PC.LAYOUT_SALT).run(0, 3)
    assert int(ok.flag.item()) == 0 and not np.array_equal(ok.positions(), got)


def test_layout_without_edges():
    """nnz = 0 through the C ABI (Layout.run skips the call): three epochs, an odd count, so the result is copied back
    from the second buffer"""
    n = 5
    y0 = 10.0 * PC.syn.u01(2 * n, 9940).reshape(n, 2)
    y = _up(y0)
    y_tmp = torch.full_like(y, float("nan"))
    indptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    a, b = _edge_case()[2]
    rc = _lib.load().ava_pj_layout(y.data_ptr(), y_tmp.data_ptr(), indptr.data_ptr(), None, None, None, None, None,
                                   n, 0, 0, 3, N_EPOCHS, 1.0, a, b, 1.0, 7, flag.data_ptr(), _lib.stream())
    assert rc == AVA_OK
    np.testing.assert_array_equal(y.cpu().numpy(), y0)
    np.testing.assert_array_equal(y_tmp.cpu().numpy(), y0)
    assert int(flag.item()) == 0
