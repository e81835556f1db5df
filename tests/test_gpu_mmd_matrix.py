"""The one-pass MMD^2 matrix on the device: ``_calculate_mmd2`` against the golden of the reference's own
function, and the kernels of csrc/mmd.hip bit for bit between a launch sequence over all conditions and the two-condition
calls that serve the per-pair estimators -- and against tests/golden/mmd_pair_gpu.npz, the results of the per-pair
kernels those calls replaced."""
import types

import numpy as np
import pytest

import mmd_matrix_cases as MC
import test_mmd as TM
from conftest import load_golden
from oracle import mmd_oracle as MO

pytestmark = pytest.mark.gpu


def _pairwise_terms(mmd, latent, condition, sigma):
    """(all_conditions, {(a, b): the four terms of ``mmd._terms``}) of every pair a < b, latent uploaded once"""
    all_conditions, idx = MC.pair_indices(condition)
    L = mmd._latent_dev(latent)
    C = len(idx)
    return all_conditions, {(a, b): mmd._terms(L, idx[a], idx[b], sigma) for a in range(C - 1) for b in range(a + 1, C)}


@pytest.mark.parametrize("alg", ["quadratic", "linear"])
def test_calculate_mmd2_matches_reference_golden(alg, tmp_path, capsys):
    from ava_amd import mmd
    G = load_golden("mmd_matrix.npz")
    latent, condition = MC.golden_case()
    module = mmd.install(types.SimpleNamespace(), matrix=True)
    mmd2_fn, condition_fn = str(tmp_path / "mmd2.npy"), str(tmp_path / "cond.npy")
    dc = MC.StubDC(latent, condition)
    result, conditions = module._calculate_mmd2(dc, MC.condition_from_fn, mmd2_fn=mmd2_fn, condition_fn=condition_fn,
                                                alg=alg, sigma=MC.GOLDEN_SIGMA)
    out = capsys.readouterr().out.splitlines()
    assert dc.requested == ['latent_means', 'audio_filenames']
    assert np.array_equal(conditions, G["conditions"]) and conditions.dtype == np.dtype('int')
    rel = MC.max_rel(result, G[alg])
    assert rel < 1e-11, rel
    assert np.array_equal(np.diag(result), np.zeros(4)) and np.array_equal(result, result.T)
    assert np.array_equal(np.load(mmd2_fn), result) and np.array_equal(np.load(condition_fn), conditions)
    assert out[:6] == ["Estimating an MMD matrix...", "\talg: " + alg, "\tparallel: False", "\tmax_n: None",
                       "\tconditions found: 4", "\tsigma: 2.0"]
    assert out[6:] == ["\tSaving MMD^2 to: " + mmd2_fn, "\tSaving conditions to: " + condition_fn, "\tDone."]

    # parallel=True: no workers, the reference's "i j mmd2" lines in (i, j) order
    again, _ = mmd._calculate_mmd2(MC.StubDC(latent, condition), MC.condition_from_fn, mmd2_fn=mmd2_fn, parallel=True,
                                   alg=alg, sigma=MC.GOLDEN_SIGMA, verbose=False)
    text = capsys.readouterr().out
    assert [line.split(' ')[:2] for line in text.splitlines()] == [[str(i), str(j)] for i in range(3) for j in range(i + 1, 4)]
    assert np.array_equal(again, result) and np.array_equal(MC.matrix_from_lines(text), result)
    print("one-pass %s vs the reference's _calculate_mmd2: %.3g relative" % (alg, rel))


@pytest.mark.parametrize("z", [1, 32, 128])
def test_block_terms_and_matrix_bitwise_equal_to_the_per_pair_path_at_tile_edges(z):
    from ava_amd import mmd
    latent, condition = MC.edge_case(z)
    sigma = MC.edge_sigma(z)
    within, cross, conditions = mmd.mmd2_block_terms(latent, condition, sigma=sigma)
    all_conditions, terms = _pairwise_terms(mmd, latent, condition, sigma)
    C = len(all_conditions)
    assert np.array_equal(conditions, all_conditions) and conditions.tolist() == sorted(MC.EDGE_LABELS)
    assert within.shape == (C,) and cross.shape == (C, C)
    assert np.array_equal(cross, cross.T) and np.array_equal(np.diag(cross), np.zeros(C))
    for (a, b), t in terms.items():
        assert within[a] == t[0] and within[b] == t[1] and cross[a, b] == t[2], (a, b)

    M, conds = mmd.mmd2_matrix_one_pass(latent, condition, sigma=sigma)
    loop, loop_conds = mmd.mmd2_matrix(latent, condition, sigma=sigma)
    assert np.array_equal(conds, loop_conds) and np.array_equal(M, loop)
    assert np.array_equal(M, M.T) and np.array_equal(np.diag(M), np.zeros(C))
    _, idx = MC.pair_indices(condition)
    for (a, b) in terms:
        want = MO.estimate_mmd2_terms(latent, idx[a], idx[b], sigma)
        got = (within[a], within[b], cross[a, b], M[a, b])
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-11 * max(abs(w), 1e-3), (a, b, got, want)
    # fixed-order reductions: the same bits again
    within2, cross2, _ = mmd.mmd2_block_terms(latent, condition, sigma=sigma)
    assert np.array_equal(within, within2) and np.array_equal(cross, cross2)
    assert np.array_equal(mmd.mmd2_matrix_one_pass(latent, condition, sigma=sigma)[0], M)


@pytest.mark.parametrize("case", ["edge", "two_workgroups"])
def test_linear_matrix_bitwise_equal_to_the_per_pair_estimator(case):
    from ava_amd import mmd
    latent, condition = MC.edge_case(32) if case == "edge" else MC.linear_case()
    sigma = MC.edge_sigma(32)
    M, conditions = mmd.mmd2_matrix_one_pass(latent, condition, alg='linear', sigma=sigma)
    all_conditions, idx = MC.pair_indices(condition)
    C = len(idx)
    assert np.array_equal(conditions, all_conditions) and M.shape == (C, C)
    assert np.array_equal(M, M.T) and np.array_equal(np.diag(M), np.zeros(C))
    L = mmd._latent_dev(latent)
    for a in range(C - 1):
        for b in range(a + 1, C):
            assert M[a, b] == mmd._estimate_mmd2_linear_time(L, idx[a], idx[b], sigma=sigma), (a, b)
            want = MO.estimate_mmd2_linear_time(latent, idx[a], idx[b], sigma=sigma)
            assert abs(M[a, b] - want) <= 1e-11 * max(abs(want), 1e-3), (a, b)
    assert np.array_equal(mmd.mmd2_matrix(latent, condition, alg='linear', sigma=sigma)[0], M)
    assert np.array_equal(mmd.mmd2_matrix_one_pass(latent, condition, alg='linear', sigma=sigma)[0], M)


def test_linear_matrix_at_the_grid_cap():
    """m = 262 150 quadruples > 1024 * 256: the pair's workgroup count is capped and 6 threads take a second stride"""
    from ava_amd import mmd, synthetic as syn
    n_a, n_b, z = 524800, 524300, 2
    latent = syn.gauss((n_a + n_b) * z, 9500).reshape(n_a + n_b, z)
    latent[n_a:] += 0.3
    condition = np.repeat([3, -1], [n_a, n_b])                       # condition -1 sorts first
    M, conditions = mmd.mmd2_matrix_one_pass(latent, condition, alg='linear', sigma=1.2)
    assert conditions.tolist() == [-1, 3] and M.shape == (2, 2) and M[0, 0] == 0 and M[1, 1] == 0
    i1, i2 = n_a + np.arange(n_b), np.arange(n_a)
    assert M[0, 1] == M[1, 0] == mmd._estimate_mmd2_linear_time(mmd._latent_dev(latent), i1, i2, sigma=1.2)
    want = MO.estimate_mmd2_linear_time(latent, i1, i2, sigma=1.2)
    assert abs(M[0, 1] - want) <= 1e-11 * max(abs(want), 1e-3)


def test_block_terms_across_a_launch_boundary():
    """two conditions of 46 400 rows: 2 * 725 * 726 / 2 + 725^2 = 1 051 975 tiles, more than the 2^20 workgroups one
    launch of the pairwise kernel covers, so the second launch starts inside the last block; z = 1 keeps it short"""
    from ava_amd import mmd, synthetic as syn
    n = 46400
    latent = syn.gauss(2 * n, 9600).reshape(2 * n, 1)
    latent[1::2] += 0.5
    condition = np.arange(2 * n) % 2
    plan = mmd._group_plan(condition)
    assert plan["blocks"][-1, 0] == 1051975 > 1 << 20 > plan["blocks"][2, 0]
    within, cross, _ = mmd.mmd2_block_terms(latent, condition, sigma=0.8)
    t = mmd._terms(mmd._latent_dev(latent), np.arange(0, 2 * n, 2), np.arange(1, 2 * n, 2), 0.8)
    assert within[0] == t[0] and within[1] == t[1] and cross[0, 1] == cross[1, 0] == t[2]
    assert 0.0 < t[3] < 1.0


def test_max_n_keeps_the_one_pass_path_unless_a_condition_is_larger():
    from ava_amd import mmd
    latent, condition = MC.edge_case(32)
    sigma = MC.edge_sigma(32)
    M, _ = mmd.mmd2_matrix_one_pass(latent, condition, sigma=sigma)
    capped, conditions = mmd.mmd2_matrix_one_pass(latent, condition, sigma=sigma, max_n=200)     # no condition is larger
    assert np.array_equal(capped, M)
    sub, conditions = mmd.mmd2_matrix_one_pass(latent, condition, sigma=sigma, max_n=50)         # the per-pair loop
    C = len(MC.EDGE_COUNTS)
    assert conditions.tolist() == sorted(MC.EDGE_LABELS) and sub.shape == (C, C)
    assert np.array_equal(sub, sub.T) and np.isfinite(sub).all() and np.array_equal(np.diag(sub), np.zeros(C))


def test_sigma_none_uses_the_median_heuristic_of_the_whole_latent_set():
    from ava_amd import mmd
    latent, condition = MC.golden_case()
    sigma = mmd.estimate_median_sigma(latent)
    assert np.array_equal(mmd.mmd2_matrix_one_pass(latent, condition)[0],
                          mmd.mmd2_matrix_one_pass(latent, condition, sigma=sigma)[0])


def test_bits_of_the_retired_per_pair_kernels():
    """tests/golden/mmd_pair_gpu.npz (tests/golden/make_golden_mmd_pair.py) was recorded on the MI355X at the last commit
    whose ``_terms`` and ``_estimate_mmd2_linear_time`` ran kernels of their own.  The estimators, the block terms and
    the one-pass matrices must reproduce it bit for bit: 2 and 3 rows in one tile, 64, 65, a 129-row symmetric block with
    tiles below the diagonal, 260 quadruples over two workgroups.  A pin for this toolchain's ``exp``; the portable check
    is the 1e-11 comparison with oracle/mmd_oracle.py of the tests above."""
    from ava_amd import mmd, synthetic as syn
    G = load_golden("mmd_pair_gpu.npz")
    pairs = lambda C: [(a, b) for a in range(C - 1) for b in range(a + 1, C)]
    for z in (1, 32, 128):
        latent, condition = MC.edge_case(z)
        sigma = MC.edge_sigma(z)
        _, terms = _pairwise_terms(mmd, latent, condition, sigma)
        within, cross, _ = mmd.mmd2_block_terms(latent, condition, sigma=sigma)
        M, _ = mmd.mmd2_matrix_one_pass(latent, condition, sigma=sigma)
        want = G["terms_z%d" % z]
        assert want.shape == (15, 4) and len(terms) == 15
        for (a, b), w in zip(pairs(len(MC.EDGE_COUNTS)), want):
            assert terms[a, b].dtype == np.float64 and np.array_equal(terms[a, b], w), (z, a, b)
            assert np.array_equal([within[a], within[b], cross[a, b], M[a, b]], w), (z, a, b)
    sigma = MC.edge_sigma(32)
    for key, (latent, condition) in (("linear_edge", MC.edge_case(32)), ("linear_two_workgroups", MC.linear_case())):
        _, idx = MC.pair_indices(condition)
        L = mmd._latent_dev(latent)
        M, _ = mmd.mmd2_matrix_one_pass(latent, condition, alg='linear', sigma=sigma)
        assert G[key].shape == (len(pairs(len(idx))),)
        for (a, b), w in zip(pairs(len(idx)), G[key]):
            assert mmd._estimate_mmd2_linear_time(L, idx[a], idx[b], sigma=sigma) == w == M[a, b], (key, a, b)
    # the quadratic calls of test_mmd.py::test_hip_matches_reference_golden_and_oracle that name their sigma
    latent, idx = TM._sets()
    sigma = float(load_golden("mmd.npz")["sigma_default_seed"])
    quad = [mmd._estimate_mmd2(latent, idx[a].copy(), idx[b].copy(), sigma=sigma) for a, b in pairs(3)]
    quad.append(mmd._estimate_mmd2(latent, idx[0].copy(), idx[2].copy(), sigma=sigma, max_n=40, seed=3))
    quad.append(mmd._estimate_mmd2(latent, idx[1][:26].copy(), idx[1][26:].copy(), sigma=0.5 * sigma))
    assert np.array_equal(quad, G["quad"])
    M, _ = mmd.mmd2_matrix_one_pass(latent, syn.latent_conditions()[1], sigma=sigma)
    assert [M[0, 1], M[0, 2], M[1, 2]] == G["quad"][:3].tolist()
