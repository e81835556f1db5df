"""The host path of the analysis modules on the MI355X: one small set of rows, presented in every form a caller may hold
it in, must give every entry point exactly the bits of the plain C-ordered float64 array.  The kernels are
bit-reproducible, so any difference is a difference of the host path: a lost ``contiguous()``, another dtype rule, a
wrong dtype code.

N = 65 rows is one row past a 64-row tile (the edge tile is live) and d = 3; every call finishes in milliseconds."""
import numpy as np
import pytest
import torch

from ava_amd import cluster_metrics, dbscan, hdbscan, knn_predict, mixture, neighbors, projection, tsne

pytestmark = pytest.mark.gpu
N, D = 65, 3
_rs = np.random.RandomState(65)
XI = _rs.randint(-40, 41, size=(N, D)).astype(np.float64)                 # integer-valued: exact in int16
X = XI / 8.0 + _rs.standard_normal((N, D))
LABELS = np.arange(N) % 3
FOLD = np.arange(N) % 4
RESP = np.abs(_rs.standard_normal((N, 2))) + 0.1
RESP /= RESP.sum(axis=1, keepdims=True)
EPS = 1.5


def precomputed(x):
    """the symmetric [N, N] matrix of euclidean distances of the rows ``x``, zero diagonal, in their dtype"""
    diff = x[:, None, :] - x[None, :, :]
    return np.sqrt((diff * diff).sum(axis=2)).astype(x.dtype)


CITY_BLOCK = np.abs(XI[:, None, :] - XI[None, :, :]).sum(axis=2)          # a matrix of integers: exact in int16


ENTRY_POINTS = {
    "projection.knn": lambda x: projection.knn(x, 4),
    "neighbors.nearest": lambda x: neighbors.nearest(x, x, metric='euclidean'),
    "dbscan.neighbor_counts": lambda x: dbscan.neighbor_counts(x, EPS),
    "hdbscan.mutual_reachability_mst": lambda x: hdbscan.mutual_reachability_mst(x, 3),
    "cluster_metrics.silhouette_samples": lambda x: cluster_metrics.silhouette_samples(x, LABELS),
    "knn_predict.masked_kneighbors": lambda x: knn_predict.masked_kneighbors(x, FOLD, 3),
    "tsne.squared_distances": lambda x: tsne.squared_distances(x),
    "mixture.m_step": lambda x: mixture.m_step(x, RESP),
}
PRECOMPUTED = {
    "dbscan.neighbor_counts": lambda m: dbscan.neighbor_counts(m, EPS, metric='precomputed'),
    "cluster_metrics.silhouette_samples": lambda m: cluster_metrics.silhouette_samples(m, LABELS, metric='precomputed'),
}


def forms(a):
    """``a`` (C-ordered numpy) in the other forms of the same dtype and values"""
    t = torch.from_numpy(a)
    return {"fortran": np.asfortranarray(a), "host tensor": t, "device tensor": t.cuda(),
            "transposed device view": torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()}


def bits(result):
    """what an entry point returned as a list of (dtype, shape, bytes)"""
    parts = result if isinstance(result, (tuple, list)) else [result]
    arrays = [p.cpu().numpy() if torch.is_tensor(p) else np.asarray(p) for p in parts]
    return [(a.dtype, a.shape, np.ascontiguousarray(a).tobytes()) for a in arrays]


def check_forms(call, a, a_int=None):
    want = bits(call(a))
    assert len(want[0][2]) > 0
    other = forms(a)
    assert not other["fortran"].flags.c_contiguous and not other["transposed device view"].is_contiguous()
    for name, form in other.items():
        assert bits(call(form)) == want, name
    if a_int is not None:                                   # int16 rows are read as the float64 rows of those values
        assert a_int.dtype == np.float64 and np.array_equal(a_int.astype(np.int16), a_int)
        assert bits(call(a_int.astype(np.int16))) == bits(call(a_int)), "int16"


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_rows_in_every_form_give_the_same_bits(name):
    check_forms(ENTRY_POINTS[name], X, XI)
    check_forms(ENTRY_POINTS[name], X.astype(np.float32))              # float32 forms against the float32 array


@pytest.mark.parametrize("name", sorted(PRECOMPUTED))
def test_precomputed_matrix_in_every_form_gives_the_same_bits(name):
    check_forms(PRECOMPUTED[name], precomputed(X), CITY_BLOCK)
    check_forms(PRECOMPUTED[name], precomputed(X.astype(np.float32)))
