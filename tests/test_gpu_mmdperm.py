"""The MMD^2 permutation test on the device: the kernels of csrc/mmd_perm.hip against the numpy
restatement of tests/mmd_perm_cases.py -- membership bytes exactly, every term of every split to 1e-11 of the terms'
sum, the count behind the p-value exactly -- and the order contract of the kernels bit for bit."""
import numpy as np
import pytest
import torch

import mmd_matrix_cases as MC
import mmd_perm_cases as PC
from ava_amd import _lib, mmd

pytestmark = pytest.mark.gpu

T = mmd.PERM_TILE                       # columns of a workgroup of the statistic kernel
N_PERMS = [1, T - 1, T, T + 1, 2 * T + 3]


def _device_membership(pools, pairs, seed, p0, p1):
    """the bytes ``ava_mmd2_perm_membership`` writes for a table of pools: uint8 [p1 - p0, all positions]"""
    lib = _lib.load()
    n1, n2 = np.array([p[0] for p in pools]), np.array([p[1] for p in pools])
    table = mmd._perm_table(0, 0, n1, n2, pairs)
    dev = mmd._device()
    tab_dev = torch.from_numpy(table).to(dev)
    out = torch.full(((p1 - p0) * int(table[-1, 5]),), 7, dtype=torch.uint8, device=dev)
    _lib.check(lib.ava_mmd2_perm_membership(table.ctypes.data, tab_dev.data_ptr(), len(pools), p0, p1, seed,
                                            out.data_ptr(), _lib.stream()), "ava_mmd2_perm_membership")
    return out.cpu().numpy().reshape(p1 - p0, -1), table


@pytest.mark.parametrize("pool", PC.MEMBER_POOLS)
def test_membership_bytes_equal_the_restatement(pool):
    n1, n2 = pool
    got, _ = _device_membership([pool], [3], PC.SEED, 0, 21)
    want = np.stack([PC.membership(n1, n2, PC.SEED, 3, p) for p in range(21)])
    assert got.shape == want.shape and np.array_equal(got, want)
    later, _ = _device_membership([pool], [3], PC.SEED, 17, 21)            # a chunk that does not start at split 0
    assert np.array_equal(later, want[17:])


def test_membership_of_a_table_of_problems_and_the_seed_wrap():
    pools, pairs = PC.MEMBER_POOLS, [4, 0, 1, 2 ** 32 - 2, 7]
    seed = 2 ** 32 - 3                                                      # seed + pair wraps for some pairs
    got, table = _device_membership(pools, pairs, seed, 0, 6)
    for (n1, n2), pair, first in zip(pools, pairs, table[:-1, 5]):
        want = np.stack([PC.membership(n1, n2, seed, pair, p) for p in range(6)])
        assert np.array_equal(got[:, first:first + n1 + n2], want), (n1, n2)


def _reference(pool, z):
    latent, i1, i2 = PC.pool_case(*pool, z=z)
    return PC.cached(("values", pool, z),
                     lambda: PC.null_distribution(latent, i1, i2, PC.value_sigma(z), PC.SEED, N_PERMS[-1]))


@pytest.mark.parametrize("z", PC.VALUE_Z)
@pytest.mark.parametrize("pool", PC.VALUE_POOLS)
def test_terms_and_statistic_of_every_split_against_the_restatement(pool, z):
    latent, i1, i2 = PC.pool_case(*pool, z=z)
    sigma = PC.value_sigma(z)
    want_all = _reference(pool, z)
    worst = 0.0
    for n_perm in N_PERMS:
        got, cnt = mmd._perm_terms(latent, i1, i2, n_perm, PC.SEED, sigma)
        want = want_all[:n_perm + 1]
        assert got.shape == want.shape == (n_perm + 1, 4)
        scale = want[:, :3].sum(axis=1, keepdims=True)
        err = float((np.abs(got - want) / scale).max())
        worst = max(worst, err)
        assert err <= PC.BOUND, (n_perm, err)
        assert np.array_equal(got[:, 3], got[:, 0] + got[:, 1] - got[:, 2])
        assert cnt == PC.count(got[:, 3])                                  # the device's count of its own statistics
        mmd2, pvalue, null = mmd.mmd2_permutation_test(latent, i1, i2, n_perm=n_perm, seed=PC.SEED, sigma=sigma,
                                                       return_null=True)
        assert mmd2 == got[0, 3] and np.array_equal(null, got[1:, 3]) and pvalue == (1 + cnt) / (n_perm + 1)
        assert mmd.mmd2_permutation_test(latent, i1, i2, n_perm=n_perm, seed=PC.SEED, sigma=sigma) == (mmd2, pvalue)
    # split 0 against the estimator the project already has, on the same index arrays
    direct = mmd._terms(mmd._latent_dev(latent), i1, i2, sigma)
    assert np.abs(got[0] - direct).max() <= PC.BOUND * direct[:3].sum()
    assert abs(got[0, 3] - mmd._estimate_mmd2(latent, i1, i2, sigma=sigma)) <= PC.BOUND * direct[:3].sum()
    print("pool %s z %d: worst term error %.3g of t1 + t2 + t3 (bound %.0e)" % (pool, z, worst, PC.BOUND))


def test_equal_memberships_give_equal_bits_and_runs_repeat():
    latent, i1, i2 = PC.pool_case(2, 3, z=8)
    sigma = PC.value_sigma(8)
    got, _ = mmd._perm_terms(latent, i1, i2, PC.N_PERM, PC.SEED, sigma)
    M = PC.memberships(2, 3, PC.SEED, 0, PC.N_PERM)
    same = [p for p in range(1, PC.N_PERM + 1) if np.array_equal(M[p], M[0])]
    assert len(same) >= 5
    for p in same:                                                          # whatever tile and column p fell in
        assert np.array_equal(got[p], got[0]), p
    again, _ = mmd._perm_terms(latent, i1, i2, PC.N_PERM, PC.SEED, sigma)
    assert np.array_equal(again, got)


@pytest.mark.parametrize("pool", [(2, 3), (129, 70)])
def test_chunks_of_any_size_give_the_bits_of_one_chunk(pool):
    latent, i1, i2 = PC.pool_case(*pool, z=32)
    sigma = PC.value_sigma(32)
    n_perm = 2 * T + 3
    table = mmd._perm_table(0, pool[0], pool[0], pool[1], 0)
    assert mmd._perm_chunk(table, n_perm + 1, None) == n_perm + 1          # the default is a single chunk here
    whole, cnt = mmd._perm_terms(latent, i1, i2, n_perm, PC.SEED, sigma)
    out = mmd.mmd2_permutation_test(latent, i1, i2, n_perm=n_perm, seed=PC.SEED, sigma=sigma, return_null=True)
    for k in (1, T, T + 1):
        max_bytes = mmd._perm_bytes(table, k)
        assert mmd._perm_chunk(table, n_perm + 1, max_bytes) == k
        got, c = mmd._perm_terms(latent, i1, i2, n_perm, PC.SEED, sigma, max_bytes=max_bytes)
        assert np.array_equal(got, whole) and c == cnt, k
        res = mmd.mmd2_permutation_test(latent, i1, i2, n_perm=n_perm, seed=PC.SEED, sigma=sigma, return_null=True,
                                        max_bytes=max_bytes)
        assert res[0] == out[0] and res[1] == out[1] and np.array_equal(res[2], out[2])


@pytest.mark.parametrize("name", PC.PVALUE_CASES)
def test_pvalue_count_equals_the_restatements(name):
    latent, i1, i2, sigma = PC.pvalue_case(name)
    want = PC.pvalue_null(name)
    assert PC.ambiguous(want) == 0                                          # asserted by tests/test_cpu_mmdperm.py too
    got, cnt = mmd._perm_terms(latent, i1, i2, PC.N_PERM, PC.SEED, sigma)
    err = float((np.abs(got - want) / want[:, :3].sum(axis=1, keepdims=True)).max())
    print("%s: count %d, p = %g, worst term error %.3g" % (name, cnt, (1 + cnt) / (PC.N_PERM + 1), err))
    assert err <= PC.BOUND
    assert cnt == PC.count(want[:, 3])
    mmd2, pvalue = mmd.mmd2_permutation_test(latent, i1, i2, n_perm=PC.N_PERM, seed=PC.SEED, sigma=sigma)
    assert pvalue == PC.pvalue(want[:, 3]) == {"AB": 0.165, "AC": 0.005, "DE": 0.375}[name]
    assert abs(mmd2 - want[0, 3]) <= PC.BOUND * want[0, :3].sum()


def test_sigma_none_uses_the_median_heuristic():
    latent, i1, i2, _ = PC.pvalue_case("AB")
    sigma = mmd.estimate_median_sigma(latent)
    assert mmd.mmd2_permutation_test(latent, i1, i2, n_perm=5) == \
        mmd.mmd2_permutation_test(latent, i1, i2, n_perm=5, sigma=sigma)


def test_matrix_entries_equal_the_per_pair_test_bit_for_bit(tmp_path, capsys):
    latent, condition = MC.edge_case(32)
    sigma = MC.edge_sigma(32)
    n_perm, seed = T + 1, 11
    mmd2, pvalue, conditions = mmd.mmd2_permutation_matrix(latent, condition, n_perm=n_perm, seed=seed, sigma=sigma)
    all_conditions, idx = MC.pair_indices(condition)
    C = len(idx)
    assert sorted(len(i) for i in idx) == sorted(MC.EDGE_COUNTS) and C == 6
    assert np.array_equal(conditions, all_conditions) and mmd2.shape == pvalue.shape == (C, C)
    assert np.array_equal(mmd2, mmd2.T) and np.array_equal(pvalue, pvalue.T)
    assert np.array_equal(np.diag(mmd2), np.zeros(C)) and np.array_equal(np.diag(pvalue), np.ones(C))
    pair = 0
    for i in range(C - 1):
        for j in range(i + 1, C):
            want = mmd.mmd2_permutation_test(latent, idx[i], idx[j], n_perm=n_perm, seed=seed + pair, sigma=sigma)
            assert (mmd2[i, j], pvalue[i, j]) == want, (i, j)
            pair += 1
    assert len(np.unique(pvalue)) > 2                                       # not all at one end
    # the statistic of split 0 is the matrix the project already computes, to the terms' bound
    within, cross, _ = mmd.mmd2_block_terms(latent, condition, sigma=sigma)
    M = within[:, None] + within[None, :] - cross
    scale = within[:, None] + within[None, :] + cross
    off = ~np.eye(C, dtype=bool)
    assert (np.abs(mmd2 - M)[off] <= PC.BOUND * scale[off]).all()
    # another chunking: the same bits
    plan = mmd._group_plan(condition)
    a, b = np.triu_indices(C, 1)
    table = mmd._perm_table(plan["offsets"][a], plan["offsets"][b], plan["counts"][a], plan["counts"][b],
                            np.arange(len(a)))
    again = mmd.mmd2_permutation_matrix(latent, condition, n_perm=n_perm, seed=seed, sigma=sigma,
                                        max_bytes=mmd._perm_bytes(table, T))
    assert np.array_equal(again[0], mmd2) and np.array_equal(again[1], pvalue)
    capsys.readouterr()

    pvalue_fn, condition_fn = str(tmp_path / "pvalue.npy"), str(tmp_path / "cond.npy")
    dc = MC.StubDC(latent, condition)
    r2, rp, rc = mmd._calculate_mmd2_pvalues(dc, MC.condition_from_fn, pvalue_fn=pvalue_fn, condition_fn=condition_fn,
                                             n_perm=n_perm, seed=seed, sigma=sigma)
    out = capsys.readouterr().out.splitlines()
    assert dc.requested == ['latent_means', 'audio_filenames']
    assert np.array_equal(r2, mmd2) and np.array_equal(rp, pvalue) and np.array_equal(rc, conditions)
    assert rc.dtype == np.dtype('int')
    assert np.array_equal(np.load(pvalue_fn), pvalue) and np.array_equal(np.load(condition_fn), conditions)
    assert out == ["Estimating an MMD p-value matrix...", "\tn_perm: %d" % n_perm, "\tseed: %d" % seed,
                   "\tconditions found: 6", "\tsigma: %s" % sigma, "\tSaving p-values to: " + pvalue_fn,
                   "\tSaving conditions to: " + condition_fn, "\tDone."]


def test_matrix_across_a_launch_boundary():
    """twelve conditions of 2 or 3 rows, 2^20 - 1 permutations in one chunk: 66 pairs x 2^20 membership workgroups (66
    launches) and 66 row tiles x 16 385 column tiles = 1 081 410 workgroups of the statistic kernel, more than the 2^20
    one launch covers, so the second launch starts inside the last pairs; pools of 4 to 6 rows keep it short"""
    from ava_amd import synthetic as syn
    counts = [2, 3] * 6
    condition = np.repeat(np.arange(12), counts)
    latent = syn.gauss(len(condition) * 2, 9900).reshape(-1, 2) + 0.2 * condition[:, None]
    n_perm, seed = (1 << 20) - 1, 3
    mmd2, pvalue, _ = mmd.mmd2_permutation_matrix(latent, condition, n_perm=n_perm, seed=seed, sigma=1.3,
                                                  max_bytes=1 << 32)
    _, idx = MC.pair_indices(condition)
    for (i, j), pair in {(0, 1): 0, (9, 11): 64, (10, 11): 65}.items():
        want = mmd.mmd2_permutation_test(latent, idx[i], idx[j], n_perm=n_perm, seed=seed + pair, sigma=1.3)
        assert (mmd2[i, j], pvalue[i, j]) == want, (i, j)
