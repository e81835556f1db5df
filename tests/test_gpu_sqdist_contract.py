"""The order contract of csrc/sqdist_tile.h across the kernels that form the tile: the same pair of rows gives the same
bits from ts_sqdist_kernel (the reference here), pj_knn_kernel, nn_eucl_kernel, the three dbscan kernels' counts,
hd_rowmin_kernel (with hd_core_kernel's scalar loop) and sil_sums_kernel.

The rows are continuous random numbers, not grid points, so the fp64 sums actually round; d sits on either side of the
32-feature stage and one feature into a third stage; 130 rows are two full 64-row tiles and an edge tile of two.  Every
comparison is ``==``: a kernel whose sum took another order, started elsewhere than 0 or skipped the fma would differ
in the last bits of some pair.  Square roots are one correctly rounded fp64 operation on either side."""
import functools

import numpy as np
import pytest

from ava_amd import cluster_metrics, dbscan, hdbscan, neighbors, projection, tsne

pytestmark = pytest.mark.gpu
equal = np.testing.assert_array_equal
N = 130
CASES = [(d, dtype) for d in (1, 32, 33, 65) for dtype in ("float32", "float64")]
case = pytest.mark.parametrize("d, dtype", CASES)


@functools.lru_cache(maxsize=None)
def rows_and_d2(d, dtype):
    """the rows and the reference: every pair's squared distance from ts_sqdist_kernel, not rounded to float32"""
    X = np.random.default_rng(0).standard_normal((N, d)).astype(dtype)
    D2 = tsne.squared_distances(X, round_float32=False).cpu().numpy()
    assert D2.dtype == np.float64 and D2.shape == (N, N)
    equal(D2, D2.T)
    equal(np.diagonal(D2), 0.0)
    D2.setflags(write=False)
    return X, D2


@case
def test_knn_distances(d, dtype):
    X, D2 = rows_and_d2(d, dtype)
    idx, dist = projection.knn(X, 8)
    equal(dist, np.sqrt(np.take_along_axis(D2, idx, axis=1)))


@case
def test_nearest_reference(d, dtype):
    X, D2 = rows_and_d2(d, dtype)
    idx, dist = neighbors.nearest(X[:65], X[65:], metric='euclidean')
    block = D2[:65, 65:]
    equal(dist, np.sqrt(block.min(axis=1)))
    equal(idx, block.argmin(axis=1))                                   # numpy's argmin: the first column at the minimum


@case
def test_dbscan_counts(d, dtype):
    X, D2 = rows_and_d2(d, dtype)
    off_diagonal = D2[~np.eye(N, dtype=bool)]
    radii = [float(np.sqrt(np.quantile(off_diagonal, q))) for q in (0.05, 0.5, 0.95)]
    got = dbscan.neighbor_counts(X, radii)
    pre = dbscan.neighbor_counts(D2.copy(), [eps * eps for eps in radii], metric='precomputed')
    equal(got, pre)
    equal(got, np.stack([(D2 <= eps * eps).sum(axis=1) for eps in radii]))


@case
def test_hdbscan_tree(d, dtype):
    X, D2 = rows_and_d2(d, dtype)
    # Edges are ordered by (w, m, i, j).  The square root is monotone, so every comparison of two keys has the same
    # outcome on the squared measures (euclidean) and on their roots (precomputed) unless two different squared
    # distances share a root; then, and only then, the two trees could differ.  On these rows none do, and no two
    # pairs tie at all.
    pairs = D2[np.triu_indices(N, 1)]
    assert len(np.unique(pairs)) == len(pairs)
    assert len(np.unique(np.sqrt(pairs))) == len(pairs)
    mst, core = hdbscan.mutual_reachability_mst(X, 5)
    mst_pre, core_pre = hdbscan.mutual_reachability_mst(np.sqrt(D2), 5, metric='precomputed')
    equal(mst[:, :2], mst_pre[:, :2])
    core2 = np.sort(D2, axis=1)[:, 4]                                   # the fifth smallest, the row itself (0) first
    i, j = mst[:, 0].astype(np.int64), mst[:, 1].astype(np.int64)
    want = np.sqrt(np.maximum(np.maximum(core2[i], core2[j]), D2[i, j]))
    equal(mst[:, 2], want)
    equal(mst_pre[:, 2], want)
    equal(core, np.sqrt(core2))
    equal(core_pre, np.sqrt(core2))


@case
def test_silhouette_samples(d, dtype):
    X, D2 = rows_and_d2(d, dtype)
    labels = np.arange(N) % 3
    equal(cluster_metrics.silhouette_samples(X, labels),
          cluster_metrics.silhouette_samples(np.sqrt(D2), labels, metric='precomputed'))
