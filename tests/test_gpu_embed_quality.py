"""GPU tests of the embedding-quality row (f26): the kernels of csrc/embed_quality.hip against the numpy restatement of
tests/embed_quality_cases.py, all integers compared exactly, and the functions of ava_amd.embedding_quality against
scikit-learn's floats of tests/golden/embed_quality.npz."""
import ctypes

import numpy as np
import pytest
import torch

import embed_quality_cases as EC
from conftest import load_golden
from gpu_util import p, stream
from ava_amd import _lib
from ava_amd import embedding_quality as EQ

pytestmark = pytest.mark.gpu


def call_ranks(X, tgt, col_splits=0, m=None):
    """(return code, rank table) of ava_eq_ranks on the rows X (float32 or float64 numpy) and the targets"""
    lib = _lib.load()
    xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(tgt, dtype=np.int64)).cuda()
    n, d = X.shape
    m = td.shape[1] if m is None else m
    nbytes = max(lib.ava_eq_workspace_bytes(n, max(min(m, 63), 1)), 512)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rank = torch.full((n, max(td.shape[1], 1)), -7, dtype=torch.int32, device="cuda")
    rc = lib.ava_eq_ranks(p(xd), _lib.dtype_code(xd), n, d, p(td), m, col_splits, p(rank), p(ws), nbytes, stream())
    torch.cuda.synchronize()
    return rc, rank.cpu().numpy()


def ranks(X, tgt, col_splits=0):
    rc, r = call_ranks(X, tgt, col_splits)
    assert rc == 0
    return r


def sweep(ks):
    return (ctypes.c_int * len(ks))(*ks)


def call_penalties(rank, ks):
    lib = _lib.load()
    rd = torch.from_numpy(np.ascontiguousarray(rank, dtype=np.int32)).cuda()
    n, m = rd.shape
    pen = torch.full((n, len(ks)), -7, dtype=torch.int64, device="cuda")
    tot = torch.full((len(ks),), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.ava_eq_penalties(p(rd), n, m, sweep(ks), len(ks), p(pen), p(tot), stream()), "ava_eq_penalties")
    torch.cuda.synchronize()
    return pen.cpu().numpy(), tot.cpu().numpy()


def call_overlap(A, B, ks):
    lib = _lib.load()
    ad = torch.from_numpy(np.ascontiguousarray(A, dtype=np.int64)).cuda()
    bd = torch.from_numpy(np.ascontiguousarray(B, dtype=np.int64)).cuda()
    n, m = ad.shape
    ov = torch.full((n, len(ks)), -7, dtype=torch.int32, device="cuda")
    tot = torch.full((len(ks),), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.ava_eq_overlap(p(ad), p(bd), n, m, sweep(ks), len(ks), p(ov), p(tot), stream()), "ava_eq_overlap")
    torch.cuda.synchronize()
    return ov.cpu().numpy(), tot.cpu().numpy()


def random_targets(n, m, seed):
    """m other rows of every row, drawn without regard to distance: far rows and the last partial tile's rows too"""
    rs = np.random.RandomState(seed)
    t = np.empty((n, m), dtype=np.int64)
    for i in range(n):
        t[i] = (i + 1 + rs.choice(n - 1, size=m, replace=m > n - 1)) % n
    return t


# ---- ava_eq_ranks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EC.RANK_N)
def test_ranks_at_tile_and_stage_edges(n):
    for d in EC.RANK_D:
        X = EC.rows(n, d, 10 * n + d)
        D2 = EC.sqd(X)
        assert EC.min_gap(D2) >= EC.MIN_GAP
        full = EC.ranks_of(EC.order(D2))
        for m in EC.RANK_M:
            tgt = random_targets(n, m, n + d + m)
            want = full[np.arange(n)[:, None], tgt].astype(np.int32)
            for cs in EC.COL_SPLITS:
                got = ranks(X, tgt, cs)
                assert np.array_equal(got, want), (n, d, m, cs)
            assert np.array_equal(ranks(X, tgt, 7), want), (n, d, m, "repeat")


@pytest.mark.parametrize("n,d,m", [(65, 3, 5), (129, 33, 63), (257, 32, 2), (130, 2, 1)])
def test_ranks_of_targets_that_are_no_neighbours(n, d, m):
    X = EC.rows(n, d, 77 + n)
    assert EC.min_gap(EC.sqd(X)) >= EC.MIN_GAP
    tgt = EC.far_targets(X, m)
    want = EC.target_ranks(X, tgt)
    assert (want[:, 0] == n - 1).all()                     # the farthest row
    if m > 1:
        assert np.array_equal(tgt[:, 0], tgt[:, 1])        # a repeated target
    for cs in (1, 2, 0):
        got = ranks(X, tgt, cs)
        assert np.array_equal(got, want), (n, d, m, cs)
    last = (n - 1) // 64 * 64                              # the rows of the last partial tile as targets of every row
    part = np.array([[j if j != i else last - 1 for j in range(last, n)][:63] for i in range(n)], dtype=np.int64)
    assert np.array_equal(ranks(X, part, 2), EC.target_ranks(X, part))


@pytest.mark.parametrize("n,d", [(65, 3), (129, 33), (257, 64)])
def test_float32_rows_and_their_float64_copy_give_one_table(n, d):
    X32 = EC.rows(n, d, 5).astype(np.float32)
    X64 = X32.astype(np.float64)
    assert EC.min_gap(EC.sqd(X64)) >= EC.MIN_GAP
    tgt = random_targets(n, 17, 3)
    a, b = ranks(X32, tgt), ranks(X64, tgt)
    assert a.dtype == np.int32 and np.array_equal(a, b)
    assert np.array_equal(a, EC.target_ranks(X64, tgt))


def test_every_row_stored_twice():
    h = 70
    X = EC.twins(h, 4, 9)
    n = 2 * h
    twin = (np.arange(n) + h) % n
    others = np.array([[(i + 1 + s) % n for s in range(40)] for i in range(n)], dtype=np.int64)
    tgt = np.concatenate([twin[:, None], others], axis=1)
    want = EC.target_ranks(X, tgt)
    assert (want[:, 0] == 1).all()                         # a row's twin is at distance 0: rank 1
    for cs in (1, 3, 0):
        assert np.array_equal(ranks(X, tgt, cs), want)
    # rows j and j + h are at equal distance from every other row: the smaller index comes first
    full = EC.ranks_of(EC.order(EC.sqd(X)))
    assert all(full[0, j + h] == full[0, j] + 1 for j in range(1, h))


def test_integer_grid():
    X = EC.grid()
    n = len(X)
    for seed in (0, 1):
        tgt = random_targets(n, 63, seed)
        want = EC.target_ranks(X, tgt)
        for cs in (1, 2):
            assert np.array_equal(ranks(X, tgt, cs), want)
        assert np.array_equal(ranks(X.astype(np.float32), tgt), want)


def test_target_tied_with_smaller_and_larger_indices():
    X = np.array([[0.0], [1.0], [-1.0], [1.0], [-1.0], [2.0], [-1.0]])
    tgt = EC.all_others(len(X))
    got = ranks(X, tgt, 1)
    assert np.array_equal(got, EC.target_ranks(X, tgt))
    assert list(got[0]) == [1, 2, 3, 4, 6, 5]              # rows 1, 2, 3, 4, 6 tie at distance 1: by index; row 5 last
    X3 = np.concatenate([X, X + 100.0, X - 300.0])
    tgt3 = EC.all_others(len(X3))
    assert np.array_equal(ranks(X3, tgt3, 2), EC.target_ranks(X3, tgt3))


def test_rank_rejections():
    X = EC.rows(70, 3, 1)
    ok = random_targets(70, 5, 0)
    assert call_ranks(X, ok)[0] == 0
    assert call_ranks(X, ok, m=0)[0] == -1
    assert call_ranks(X, random_targets(70, 64, 0), m=64)[0] == -1
    assert call_ranks(X, ok, col_splits=-1)[0] == -1
    own = ok.copy()
    own[69, 4] = 69                                        # a target equal to its row
    rc, table = call_ranks(X, own)
    assert rc == -1 and (table == -7).all()                # refused before anything is written
    out = ok.copy()
    out[3, 2] = 70                                         # a target equal to n
    assert call_ranks(X, out)[0] == -1
    out[3, 2] = -1
    assert call_ranks(X, out)[0] == -1


# ---- ava_eq_penalties ----------------------------------------------------------------------------------------------------
def test_penalties_at_ranks_k_and_k_plus_one():
    ks = [1, 2, 5, 63]
    table = np.concatenate([np.full((1, 63), k) for k in ks] + [np.full((1, 63), k + 1) for k in ks]).astype(np.int32)
    pen, tot = call_penalties(table, ks)
    want, wtot = EC.penalties(table, ks)
    assert np.array_equal(pen, want) and np.array_equal(tot, wtot)
    for a, k in enumerate(ks):
        assert pen[a, a] == 0 and pen[4 + a, a] == k       # rank k costs nothing, rank k + 1 one per slot
    assert np.array_equal(pen.sum(axis=0), tot)


def test_penalty_totals_pass_two_to_the_32():
    n = 300
    table = (2 ** 31 - 1 - np.arange(n * 5).reshape(n, 5) % 1000).astype(np.int32)
    ks = [1, 5, 3]
    pen, tot = call_penalties(table, ks)
    want, wtot = EC.penalties(table, ks)
    assert wtot[1] > 2 ** 32 and pen.dtype == np.int64 and tot.dtype == np.int64
    assert np.array_equal(pen, want) and np.array_equal(tot, wtot)
    assert np.array_equal(pen.sum(axis=0), tot)


# ---- ava_eq_overlap ------------------------------------------------------------------------------------------------------
def test_overlap_of_identical_disjoint_and_single_match_tables():
    n, m = 133, 63
    ks = [1, 2, 5, 63]
    A = np.array([(i + 1 + np.random.RandomState(i).permutation(300)[:m]) for i in range(n)], dtype=np.int64)
    ov, tot = call_overlap(A, A, ks)
    assert (ov == np.array(ks)[None, :]).all() and list(tot) == [n * k for k in ks]
    ov, tot = call_overlap(A, A + 1000, ks)
    assert (ov == 0).all() and (tot == 0).all()
    shuffled = A[:, ::-1].copy()
    ov, tot = call_overlap(A, shuffled, ks)
    want, wtot = EC.overlaps(A, shuffled, ks)
    assert np.array_equal(ov, want) and np.array_equal(tot, wtot)
    for s, t in [(0, 0), (3, 9), (9, 3), (62, 0), (30, 62)]:
        B = A + 1000
        B[:, t] = A[:, s]
        hi = max(s, t)
        sw = sorted({k for k in (hi, hi + 1, 63) if k >= 1})
        ov, tot = call_overlap(A, B, sw)
        for a, k in enumerate(sw):
            assert (ov[:, a] == (1 if k > hi else 0)).all(), (s, t, k)
        assert np.array_equal(ov.sum(axis=0), tot)


# ---- whole functions on the golden cases ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden("embed_quality.npz")


@pytest.mark.parametrize("i", range(len(EC.GOLDEN_CASES)))
def test_golden_cases_equal_sklearn_exactly(golden, i):
    n, d, k, seed = EC.GOLDEN_CASES[i]
    _, X = EC.golden_x(n, d, seed)
    Y = golden["c%d_Y" % i]
    trust, cont = float(golden["c%d_trust" % i]), float(golden["c%d_cont" % i])
    assert EQ.trustworthiness(X, Y, n_neighbors=k) == trust
    assert EQ.continuity(X, Y, n_neighbors=k) == cont
    xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    assert EQ.trustworthiness(xd, yd, n_neighbors=k) == trust        # device tensors: the same values
    nx, ny = EQ._neighbours_device(xd, k), EQ._neighbours_device(yd, k)
    rank_x, rank_y = EQ._ranks_device(xd, ny), EQ._ranks_device(yd, nx)
    _, tot_t = EQ._penalties_device(rank_x, [k])
    _, tot_c = EQ._penalties_device(rank_y, [k])
    assert int(tot_t[0]) == int(golden["c%d_pen_t" % i]) and int(tot_c[0]) == int(golden["c%d_pen_c" % i])
    if i < EC.GOLDEN_RANK_TABLES:
        assert np.array_equal(rank_x.cpu().numpy(), golden["c%d_rank_x" % i])
        assert np.array_equal(rank_y.cpu().numpy(), golden["c%d_rank_y" % i])
        assert np.array_equal(EQ.neighbor_ranks(X, ny.cpu().numpy()), golden["c%d_rank_x" % i])

    ks = sorted({1, 5, k})
    cur = EQ.quality_curve(X, Y, ks)
    for a, kk in enumerate(ks):
        assert cur["trustworthiness"][a] == EQ.trustworthiness(X, Y, n_neighbors=kk)
        assert cur["continuity"][a] == EQ.continuity(X, Y, n_neighbors=kk)
        assert cur["preservation"][a] == EQ.neighborhood_preservation(X, Y, n_neighbors=kk)
        assert cur["lcmc"][a] == cur["preservation"][a] - kk / (n - 1.0)
    assert cur["trustworthiness"][-1] == trust and cur["continuity"][-1] == cont
    assert EQ.neighborhood_preservation(X, X, n_neighbors=k) == 1.0
    cur_t = EQ.quality_curve(xd, yd, ks)
    assert all(np.array_equal(cur[key], cur_t[key]) for key in cur)


def test_curve_local_and_compare_against_the_restatement(golden):
    n, d, k, seed = EC.GOLDEN_CASES[1]
    _, X = EC.golden_x(n, d, seed)
    Y = golden["c1_Y"]
    ks = [1, 5, k]
    want = EC.Pair(X, Y, k).curve(ks)
    cur = EQ.quality_curve(X, Y, ks)
    for key in ("trustworthiness", "continuity", "preservation", "lcmc"):
        assert np.array_equal(cur[key], want[key]), key
    loc, wloc = EQ.local_quality(X, Y, 5), EC.Pair(X, Y, 5).local(5)
    for key in ("trustworthiness", "continuity", "overlap"):
        assert np.array_equal(loc[key], wloc[key]), key
    assert abs(loc["trustworthiness"].mean() - cur["trustworthiness"][1]) <= 1e-15
    Z = Y[:, ::-1] * np.array([1.0, 0.25])
    both = EQ.compare_projections(X, {"pca": Y, "squeezed": Z}, ks)
    assert list(both) == ["pca", "squeezed"]
    for name, E in (("pca", Y), ("squeezed", Z)):
        one = EQ.quality_curve(X, E, ks)
        assert all(np.array_equal(both[name][key], one[key]) for key in one)
