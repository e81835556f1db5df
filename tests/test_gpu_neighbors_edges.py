"""The nearest-neighbour kernels (csrc/neighbors.hip, row f7) on the MI355X at their tile, stage and reduce edges:
neighbor_cases.EDGE_CASES against the fp64 numpy restatement, the four dtype instantiations, chunking at non-tile sizes,
workspace reuse, ava_nn_merge through the C ABI against the restated nn_better, and the refusals.

Bounds: indices compare with == (test_cpu_neighbors.py verifies that every case decides by more than 1e-9, the planted
ties apart, which are exact); distances are within the project's bounds of test_gpu_neighbors._check_against, 1e-12
absolute for correlation and 1e-12 relative for euclidean.  The near-constant rows are compared against an np.longdouble
restatement within max(1e-12, 4 x floor), the floor being the fp64 restatement's own error there."""
import numpy as np
import pytest
import torch

import neighbor_cases as NC
from gpu_util import p, stream
from ava_amd import _lib, neighbors as N

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -3


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _same_bits(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))


_single = {}


def _nearest(name):
    """the single-launch answer of a case, computed once"""
    if name not in _single:
        case = NC.edge_case(name)
        _single[name] = N.nearest(case["q"], case["r"], metric=case["metric"])
    return _single[name]


@pytest.mark.parametrize("name", sorted(NC.EDGE_CASES))
def test_edge_case(name):
    case = NC.edge_case(name)
    metric = case["metric"]
    idx, dist = _nearest(name)
    assert idx.dtype == np.int64 and dist.dtype == np.float64 and idx.shape == dist.shape == (len(case["q"]),)
    want = case["dist"]
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(dist - want) / (1.0 if metric == "correlation" else np.where(want == 0.0, 1.0, np.abs(want)))
    print("%s [%s, %s]: largest distance error %.3e (bound 1e-12 %s)"
          % (name, case["group"], metric, np.nanmax(err) if not np.isnan(err).all() else 0.0,
             "absolute" if metric == "correlation" else "relative"))
    np.testing.assert_array_equal(idx, case["idx"])
    np.testing.assert_array_equal(np.isnan(dist), np.isnan(want))
    if metric == "correlation":
        np.testing.assert_allclose(dist, want, rtol=0, atol=1e-12)
        assert (np.isnan(dist) | ((dist >= 0.0) & (dist <= 2.0))).all()
    else:
        np.testing.assert_allclose(dist, want, rtol=1e-12, atol=0)
    for query, low, _ in case["ties"]:
        assert idx[query] == low
    for query in case["same"]:
        assert 0.0 <= dist[query] <= 1e-12
    for query in case["mirror"]:
        assert 0.0 <= 2.0 - dist[query] <= 1e-12
    if case["group"] == "d1":
        assert np.isnan(dist).all() and (idx == 0).all()
    if name == "edge_corr_nan_query":
        assert np.isnan(dist[1]) and idx[1] == 0 and not np.isnan(dist[[0, 2]]).any()
    # device tensors in: the same bits
    _same_bits(N.nearest(torch.from_numpy(case["q"]).cuda(), torch.from_numpy(case["r"]).cuda(), metric=metric),
               (idx, dist))


def test_near_constant_rows_keep_their_precision():
    """corr_tile.h: the dot products are of the centred values, which keeps the precision of rows with a large mean and
    a small variation.  Against the np.longdouble restatement, within max(1e-12, 4 x floor)."""
    case = NC.edge_case(NC.NEAR_CONSTANT)
    floor, DL = NC.near_constant_floor()
    idx, dist = _nearest(NC.NEAR_CONSTANT)
    np.testing.assert_array_equal(idx, case["idx"])
    err = float(np.max(np.abs(dist.astype(np.longdouble) - DL[np.arange(len(idx)), idx])))
    bound = max(1e-12, 4.0 * floor)
    print("near-constant rows: floor of the fp64 restatement %.3e, device error against longdouble %.3e (bound %.3e)"
          % (floor, err, bound))
    assert err <= bound


@pytest.mark.parametrize("name", ["edge_eucl_q65_r65_d33_f32", "edge_corr_q129_r129_d17_f32", "edge_eucl_reduce_r8193",
                                  "edge_corr_reduce_r8193_dup"])
@pytest.mark.parametrize("metric", ["correlation", "euclidean"])
def test_four_dtype_combinations_give_the_same_bits(name, metric):
    """float32 rows and their exact float64 copies, in the four <TQ, TR> instantiations of both tile kernels"""
    case = NC.edge_case(name)
    q32, r32 = case["q"], case["r"]
    assert q32.dtype == np.float32 and r32.dtype == np.float32
    q64, r64 = q32.astype(np.float64), r32.astype(np.float64)
    assert np.array_equal(q64.astype(np.float32), q32) and np.array_equal(r64.astype(np.float32), r32)
    D = NC.distances(q32, r32, metric)
    want_idx, want_dist = NC.nearest_from_distances(D, metric)
    first = N.nearest(q32, r32, metric=metric)
    tied = NC.gap(D) <= 1e-9                        # planted ties, or near ones under the other metric
    np.testing.assert_array_equal(first[0][~tied], want_idx[~tied])
    if metric == "correlation":
        np.testing.assert_allclose(first[1], want_dist, rtol=0, atol=1e-12)
    else:
        np.testing.assert_allclose(first[1], want_dist, rtol=1e-12, atol=0)
    for q, r in [(q32, r64), (q64, r32), (q64, r64)]:
        _same_bits(N.nearest(q, r, metric=metric), first)
        _same_bits(N.nearest(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(), metric=metric), first)


@pytest.mark.parametrize("name", ["edge_corr_position_257_d17", "edge_eucl_reduce_r4097"])
@pytest.mark.parametrize("chunk", [1, 65, 129, -1])
def test_chunking_at_non_tile_sizes(name, chunk):
    """chunk_rows of 1, 65, 129 and nr - 1 give the bits of the single launch, from host arrays and device tensors"""
    case = NC.edge_case(name)
    chunk_rows = chunk if chunk > 0 else len(case["r"]) + chunk
    want = _nearest(name)
    _same_bits(N.nearest(case["q"], case["r"], metric=case["metric"], chunk_rows=chunk_rows), want)
    _same_bits(N.nearest(torch.from_numpy(case["q"]).cuda(), torch.from_numpy(case["r"]).cuda(), metric=case["metric"],
                         chunk_rows=chunk_rows), want)


def _argmin(q, r, metric, ws, ws_bytes, out_idx, out_dist):
    lib = _lib.load()
    rc = lib.ava_nn_argmin(p(q), _lib.dtype_code(q), q.shape[0], p(r), _lib.dtype_code(r), r.shape[0], q.shape[1],
                           N.METRICS[metric], p(out_idx), p(out_dist), p(ws), ws_bytes, stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", ["edge_eucl_reduce_r8193", "edge_corr_reduce_r8193"])
def test_workspace_reuse_reads_no_stale_partials(name):
    """a 129-tile (65-tile) launch, a one-reference launch and the first again in one workspace: the partials the
    first left beyond rtiles = 1 are not read by the second, nor what the second left by the third.  The workspace
    starts as zeros, which read as a partial (distance 0, index 0) would beat every candidate."""
    case = NC.edge_case(name)
    metric = case["metric"]
    lib = _lib.load()
    q, r = torch.from_numpy(case["q"]).cuda(), torch.from_numpy(case["r"]).cuda()
    nq, d = q.shape
    nbytes = lib.ava_nn_workspace_bytes(nq, r.shape[0], d, N.METRICS[metric])
    assert nbytes >= lib.ava_nn_workspace_bytes(nq, 1, d, N.METRICS[metric]) > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    runs = []
    for refs in (r, r[7:8].contiguous(), r):
        out_idx = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
        out_dist = torch.full((nq,), -7.0, dtype=torch.float64, device="cuda")
        assert _argmin(q, refs, metric, ws, nbytes, out_idx, out_dist) == 0
        runs.append((out_idx.cpu().numpy(), out_dist.cpu().numpy()))
    _same_bits(runs[0], _nearest(name))
    _same_bits(runs[2], runs[0])
    np.testing.assert_array_equal(runs[1][0], np.zeros(nq, dtype=np.int64))
    _same_bits(runs[1], N.nearest(case["q"], case["r"][7:8], metric=metric))
    # the same through the module, which sizes a workspace per call
    _same_bits(N.nearest(case["q"], case["r"], metric=metric), runs[0])


def _merge_table(offset):
    """every pair of distances from {0.0, -0.0, 1.0, NaN}, each with idx + offset below, equal to and above best_idx;
    repeated to 288 elements, so that nn_merge_kernel's second, partly filled workgroup runs too"""
    vals = [0.0, -0.0, 1.0, np.nan]
    best_idx, best_dist, idx, dist = [], [], [], []
    for bd in vals:
        for cd in vals:
            for ci in (9, 10, 11):
                best_idx.append(offset + 10)
                best_dist.append(bd)
                idx.append(ci)
                dist.append(cd)
    rep = 6
    return (np.tile(np.array(best_idx, dtype=np.int64), rep), np.tile(np.array(best_dist), rep),
            np.tile(np.array(idx, dtype=np.int64), rep), np.tile(np.array(dist), rep))


@pytest.mark.parametrize("metric", ["correlation", "euclidean"])
@pytest.mark.parametrize("offset", [0, 7, 2 ** 31 + 5])
def test_merge_is_the_restated_nn_better(metric, offset):
    lib = _lib.load()
    best_idx, best_dist, idx, dist = _merge_table(offset)
    assert len(idx) == 288 and (np.signbit(dist) & (dist == 0.0)).any()
    want_idx, want_dist = NC.merge(best_idx, best_dist, idx, dist, offset, 1 if metric == "euclidean" else 0)
    assert (want_idx != best_idx).any() and (want_idx == best_idx).any()
    bi, bd = torch.from_numpy(best_idx).cuda(), torch.from_numpy(best_dist).cuda()
    ci, cd = torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda()
    rc = lib.ava_nn_merge(p(bi), p(bd), p(ci), p(cd), len(idx), offset, N.METRICS[metric], stream())
    torch.cuda.synchronize()
    assert rc == 0
    np.testing.assert_array_equal(bi.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(_bits(bd.cpu().numpy()), _bits(want_dist))
    np.testing.assert_array_equal(ci.cpu().numpy(), idx)                 # the candidates are read only
    np.testing.assert_array_equal(_bits(cd.cpu().numpy()), _bits(dist))


@pytest.mark.parametrize("metric", ["correlation", "euclidean"])
def test_refusals_launch_nothing(metric):
    """a workspace one byte short is AVA_EWORKSPACE, a bad argument AVA_EINVAL, and the pre-filled outputs stay as they
    were.  Every pointer is valid and every buffer is as large as the valid call needs."""
    lib = _lib.load()
    code = N.METRICS[metric]
    case = NC.edge_case("edge_eucl_q65_r65_d33_f64" if metric == "euclidean" else "edge_corr_q129_r129_d17_f64")
    q, r = torch.from_numpy(case["q"]).cuda(), torch.from_numpy(case["r"]).cuda()
    nq, d = q.shape
    nr = r.shape[0]
    nbytes = lib.ava_nn_workspace_bytes(nq, nr, d, code)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out_idx = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    out_dist = torch.full((nq,), -7.0, dtype=torch.float64, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((out_idx == -7).all()) and bool((out_dist == -7.0).all())

    assert _argmin(q, r, metric, ws, nbytes - 1, out_idx, out_dist) == EWORKSPACE and untouched()
    assert _argmin(q, r, metric, ws, 0, out_idx, out_dist) == EWORKSPACE and untouched()
    good = dict(q_dtype=1, nq=nq, r_dtype=1, nr=nr, d=d, metric=code)
    for bad in [dict(nq=0), dict(nq=-1), dict(nr=0), dict(d=0), dict(d=65537), dict(metric=2), dict(metric=-1),
                dict(q_dtype=2), dict(r_dtype=-1)]:
        a = dict(good, **bad)
        rc = lib.ava_nn_argmin(p(q), a["q_dtype"], a["nq"], p(r), a["r_dtype"], a["nr"], a["d"], a["metric"],
                               p(out_idx), p(out_dist), p(ws), nbytes, stream())
        assert rc == EINVAL and untouched(), bad
    for null in range(5):
        ptrs = [p(q), p(r), p(out_idx), p(out_dist), p(ws)]
        ptrs[null] = None
        rc = lib.ava_nn_argmin(ptrs[0], 1, nq, ptrs[1], 1, nr, d, code, ptrs[2], ptrs[3], ptrs[4], nbytes, stream())
        assert rc == EINVAL and untouched(), null
    # the merge: the candidates are valid buffers that would win every query
    ci = torch.zeros(nq, dtype=torch.int64, device="cuda")
    cd = torch.full((nq,), -9.0, dtype=torch.float64, device="cuda")
    for n, offset, m in [(0, 0, code), (-1, 0, code), (nq, -1, code), (nq, 0, 2), (nq, 0, -1)]:
        assert lib.ava_nn_merge(p(out_idx), p(out_dist), p(ci), p(cd), n, offset, m, stream()) == EINVAL and untouched()
    # and the valid call still runs in the same buffers
    assert _argmin(q, r, metric, ws, nbytes, out_idx, out_dist) == 0
    _same_bits((out_idx.cpu().numpy(), out_dist.cpu().numpy()), _nearest(
        "edge_eucl_q65_r65_d33_f64" if metric == "euclidean" else "edge_corr_q129_r129_d17_f64"))
