"""The MMD^2 permutation test without a GPU: the numpy restatement of tests/mmd_perm_cases.py against
oracle/mmd_oracle.py, the identities the kernels of csrc/mmd_perm.hip rest on, the conditions the GPU cases of
tests/test_gpu_mmdperm.py need, and the error paths that are decided before any launch."""
import numpy as np
import pytest

import mmd_matrix_cases as MC
import mmd_perm_cases as PC
from oracle import mmd_oracle as MO
from ava_amd import mmd, synthetic as syn


@pytest.mark.parametrize("pool", [(2, 3), (65, 129), (129, 70)])
def test_split_zero_of_the_restatement_is_the_oracles_estimate(pool):
    latent, i1, i2 = PC.pool_case(*pool, z=8)
    sigma = PC.value_sigma(8)
    got = PC.null_distribution(latent, i1, i2, sigma, seed=3, n_perm=2)[0]
    want = MO.estimate_mmd2_terms(latent, i1, i2, sigma)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-13 * sum(want[:3])


def test_keys_are_the_hash_stream_of_synthetic_u01():
    for seed, pair, p in [(0, 0, 1), (5, 3, 199), (2 ** 32 - 1, 2, 7)]:
        salt = (((seed + pair) % 2 ** 32) << 32) + p
        k = PC.keys(300, seed, pair, p)
        assert k.dtype == np.uint64 and len(np.unique(k)) == 300
        assert np.array_equal((k >> np.uint64(11)).astype(np.float64) / float(1 << 53), syn.u01(300, salt))


@pytest.mark.parametrize("pool", PC.MEMBER_POOLS)
def test_memberships_have_exactly_n1_members(pool):
    n1, n2 = pool
    M = PC.memberships(n1, n2, PC.SEED, 0, 20)
    assert M.shape == (21, n1 + n2) and M.dtype == np.uint8
    assert np.array_equal(M.sum(axis=1), np.full(21, n1))
    assert np.array_equal(M[0], np.arange(n1 + n2) < n1)
    assert len({m.tobytes() for m in M[1:]}) > 1                            # the splits differ
    assert not np.array_equal(PC.membership(n1, n2, PC.SEED, 1, 1), M[1])   # and so do the pairs of a matrix


def test_memberships_under_forced_key_ties_go_to_the_smaller_position():
    tied = lambda n, seed, pair, p: PC.keys(n, seed, pair, p) >> np.uint64(62)      # four distinct keys
    for n1, n2 in [(2, 3), (65, 129), (129, 70)]:
        for p in (1, 2, 3):
            m = PC.membership(n1, n2, 9, 0, p, key_fn=tied)
            assert m.sum() == n1
            k = tied(n1 + n2, 9, 0, p)
            worst = k[m == 1].max()                                         # the key of the n1-th smallest
            assert (k[m == 0] >= worst).all()
            at = np.flatnonzero(k == worst)
            taken = int(m[at].sum())
            assert np.array_equal(m[at], np.arange(len(at)) < taken)        # among equal keys: ascending position


@pytest.mark.parametrize("pool", [(2, 129), (129, 2), (64, 64), (129, 70)])
def test_gemm_identity_with_the_smaller_set_marked_reproduces_the_brute_force_terms(pool):
    n1, n2 = pool
    latent, i1, i2 = PC.pool_case(n1, n2, z=8)
    K = PC.kernel_matrix(latent[np.concatenate([i1, i2])], PC.value_sigma(8))
    for p in range(6):
        member = PC.membership(n1, n2, PC.SEED, 0, p)
        want, got = PC.split_terms(K, member), PC.gemm_terms(K, member)
        bound = PC.BOUND * sum(want[:3])
        assert max(abs(g - w) for g, w in zip(got, want)) <= bound


@pytest.mark.parametrize("name", PC.PVALUE_CASES)
def test_pvalue_cases_have_no_permuted_statistic_near_stat_zero(name):
    """the condition under which the device's count must equal the restatement's exactly"""
    latent, i1, i2, sigma = PC.pvalue_case(name)
    assert len(i1) != len(i2)
    terms = PC.pvalue_null(name)
    assert terms.shape == (PC.N_PERM + 1, 4) and PC.ambiguous(terms) == 0
    for p in range(1, PC.N_PERM + 1):
        assert len(np.unique(PC.keys(len(i1) + len(i2), PC.SEED, 0, p))) == len(i1) + len(i2)
    p = PC.pvalue(terms[:, 3])
    print(name, "p =", p, "count =", PC.count(terms[:, 3]))
    assert p == {"AB": 0.165, "AC": 0.005, "DE": 0.375}[name]


def test_contract_case_has_permuted_splits_equal_to_split_zero():
    M = PC.memberships(2, 3, PC.SEED, 0, PC.N_PERM)
    same = [p for p in range(1, PC.N_PERM + 1) if np.array_equal(M[p], M[0])]
    assert 5 <= len(same) <= 40                                             # about 1 in C(5, 2) = 10 of 199
    terms = PC.null_distribution(*PC.pool_case(2, 3, 8), PC.value_sigma(8), PC.SEED, PC.N_PERM)
    assert all(terms[p, 3] == terms[0, 3] for p in same)


def test_problem_table_and_chunking():
    table = mmd._perm_table([0, 10], [3, 0], [3, 129], [5, 70], [0, 1])
    assert table.dtype == np.int64 and table.shape == (3, 8)
    assert table.tolist() == [[0, 3, 3, 5, 0, 0, 0, 0], [10, 0, 129, 70, 1, 8, 1, 0], [0, 0, 0, 0, 0, 207, 5, 0]]
    assert mmd.PERM_TILE == 64 and mmd.PERM_MAX_BYTES == 256 << 20
    for k in (1, 63, 64, 65, 1000):
        assert mmd._perm_bytes(table, k) == k * 207 + 5 * (k + 1) * 16 + 256
        assert mmd._perm_chunk(table, 5000, mmd._perm_bytes(table, k)) == k
        assert mmd._perm_chunk(table, 5000, mmd._perm_bytes(table, k + 1) - 1) == k
    assert mmd._perm_chunk(table, 5000, 0) == 1 and mmd._perm_chunk(table, 40, None) == 40
    assert "mmd2_permutation_test" in mmd.__all__ and "mmd2_permutation_matrix" in mmd.__all__
    assert "_calculate_mmd2_pvalues" in mmd.__all__


def test_bad_arguments_raise_before_anything_touches_the_device():
    """none of these reaches the device: they pass on a machine without one"""
    latent = np.zeros((6, 3))
    two, one = np.array([0, 1]), np.array([2])
    for i1, i2 in [(two, one), (one, two), (two, np.zeros(0, dtype=int))]:
        with pytest.raises(ZeroDivisionError):
            mmd.mmd2_permutation_test(latent, i1, i2, n_perm=10, sigma=2.0)
        with pytest.raises(ZeroDivisionError):
            mmd.mmd2_permutation_test(latent, i1, i2, n_perm=10)                # before sigma is estimated
    for n_perm in (0, -3):
        with pytest.raises(ValueError):
            mmd.mmd2_permutation_test(latent, two, np.array([2, 3]), n_perm=n_perm, sigma=2.0)
        with pytest.raises(ValueError):
            mmd.mmd2_permutation_matrix(latent, np.array([0, 0, 0, 1, 1, 1]), n_perm=n_perm, sigma=2.0)
    single = np.array([4, 4, 9, 4, 4, 4])                                       # condition 9 has one row
    with pytest.raises(ZeroDivisionError):
        mmd.mmd2_permutation_matrix(latent, single, n_perm=10, sigma=2.0)
    with pytest.raises(ZeroDivisionError):
        mmd.mmd2_permutation_matrix(latent, single, n_perm=10)
    dc = MC.StubDC(latent, single)
    with pytest.raises(AssertionError):
        mmd._calculate_mmd2_pvalues(dc, MC.condition_from_fn, pvalue_fn=None, sigma=2.0, verbose=False)
    assert dc.requested == []
    # fewer than two conditions: nothing to test, nothing launched
    m2, pv, conditions = mmd.mmd2_permutation_matrix(latent, np.full(6, -6), n_perm=10, sigma=2.0)
    assert np.array_equal(m2, [[0.0]]) and np.array_equal(pv, [[1.0]]) and conditions.tolist() == [-6]
    m2, pv, conditions = mmd.mmd2_permutation_matrix(np.zeros((0, 3)), np.zeros(0, dtype=int), sigma=2.0)
    assert m2.shape == (0, 0) and pv.shape == (0, 0) and len(conditions) == 0


def test_install_adds_the_pvalue_function_only_on_request():
    import types
    module = types.SimpleNamespace()
    mmd.install(module, matrix=True)
    assert not hasattr(module, "_calculate_mmd2_pvalues")
    mmd.install(module, pvalues=True)
    assert module._calculate_mmd2_pvalues is mmd._calculate_mmd2_pvalues and module._calculate_mmd2 is mmd._calculate_mmd2


def test_c_abi_checks_the_table_and_sizes_the_workspace_on_the_host():
    """argument checks and the workspace formula of include/ava_hip.h run before any HIP call"""
    from ava_amd import _lib
    lib = _lib.load()
    assert lib.ava_mmd2_perm_tile() == mmd.PERM_TILE
    good = mmd._perm_table([0, 10], [3, 0], [3, 129], [5, 70], [0, 1])
    need = lib.ava_mmd2_perm_workspace_bytes
    assert need(good.ctypes.data, 2, 65) == 5 * 66 * 16 + 256 == mmd._perm_bytes(good, 65) - 65 * 207
    assert need(good.ctypes.data, 2, 0) == 0 and need(None, 2, 4) == 0 and need(good.ctypes.data, 0, 4) == 0
    small = mmd._perm_table(0, 1, 1, 5, 0)                                       # n1 < 2
    wrong = good.copy()
    wrong[1, 5] += 1                                                            # sums that disagree
    assert need(small.ctypes.data, 1, 4) == 0 and need(wrong.ctypes.data, 2, 4) == 0

    fake = 4096                                                                 # never dereferenced: all rejected

    def call(z=8, table=good, n_problems=2, n_idx=300, p0=0, p1=10, sigma=1.0, ws_bytes=1 << 20):
        return lib.ava_mmd2_perm(fake, z, fake, n_idx, table.ctypes.data, fake, n_problems, p0, p1, 0, sigma, fake, fake,
                                 fake, fake, fake, fake, ws_bytes, None)
    assert call(z=0) == -1 and call(z=129) == -1 and call(sigma=0.0) == -1 and call(sigma=float("nan")) == -1
    assert call(p1=0) == -1 and call(p0=-1) == -1 and call(p0=10, p1=10) == -1 and call(p1=2 ** 31) == -1
    assert call(table=small, n_problems=1) == -1 and call(table=wrong) == -1 and call(n_problems=0) == -1
    assert call(n_idx=138) == -1                                                # the second list leaves the index list
    assert call(ws_bytes=5 * 11 * 16 + 255) == -3
    assert lib.ava_mmd2_perm_membership(good.ctypes.data, fake, 2, 3, 3, 0, fake, None) == -1
    assert lib.ava_mmd2_perm_membership(small.ctypes.data, fake, 1, 0, 3, 0, fake, None) == -1
