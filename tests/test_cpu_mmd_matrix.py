"""The one-pass MMD^2 matrix without a GPU: the numpy restatement of tests/mmd_matrix_cases.py against the
golden written by the reference's own ``_calculate_mmd2``, the grouping plan of ``ava_amd.mmd._group_plan`` and the
error paths that are decided before any launch."""
import types

import numpy as np
import pytest

import mmd_matrix_cases as MC
from conftest import load_golden
from ava_amd import mmd


@pytest.mark.parametrize("alg", ["quadratic", "linear"])
def test_restatement_matches_reference_golden(alg):
    G = load_golden("mmd_matrix.npz")
    latent, condition = MC.golden_case()
    want, conditions = MC.matrix_oracle(latent, condition, alg, MC.GOLDEN_SIGMA)
    assert np.array_equal(conditions, G["conditions"]) and conditions.tolist() == [-3, 0, 7, 40]
    assert np.array_equal(np.diag(want), np.zeros(4)) and np.array_equal(want, want.T)
    assert MC.max_rel(want, G[alg]) < 1e-11


def _cases():
    return [MC.golden_case()[1], MC.edge_case(1)[1], MC.linear_case()[1]]


@pytest.mark.parametrize("case", range(3))
def test_group_plan_lists_offsets_and_tables(case):
    condition = _cases()[case]
    plan = mmd._group_plan(condition)
    all_conditions, idx = MC.pair_indices(condition)
    C = len(all_conditions)
    assert np.array_equal(plan["all_conditions"], all_conditions)
    offsets, index = plan["offsets"], plan["index"]
    assert index.dtype == np.int64 and offsets.dtype == np.int64 and offsets.shape == (C + 1,)
    assert offsets[0] == 0 and offsets[-1] == len(condition)
    for c in range(C):
        assert np.array_equal(index[offsets[c]:offsets[c + 1]], idx[c])
    counts = np.array([len(i) for i in idx])
    assert np.array_equal(plan["counts"], counts)
    tiles = plan["tiles"]
    assert np.array_equal(tiles, -(-counts // 64))

    blocks = plan["blocks"]
    assert blocks.dtype == np.int64 and blocks.shape == (C * (C + 1) // 2 + 1, 4)
    rows = [(a, b) for a in range(C) for b in range(a, C)]
    assert [tuple(r) for r in blocks[:-1, 2:]] == rows
    launched = [tiles[a] * (tiles[a] + 1) // 2 if a == b else tiles[a] * tiles[b] for a, b in rows]
    full = [tiles[a] * tiles[b] for a, b in rows]
    assert blocks[0, 0] == 0 and blocks[0, 1] == 0
    assert np.array_equal(np.diff(blocks[:, 0]), launched) and min(launched) >= 1      # strictly increasing
    assert np.array_equal(np.diff(blocks[:, 1]), full)

    pairs = plan["pairs"]
    rows = [(a, b) for a in range(C) for b in range(a + 1, C)]
    assert pairs.shape == (len(rows) + 1, 4) and [tuple(r) for r in pairs[:-1, 2:]] == rows
    groups = [min(-(-(min(counts[a], counts[b]) // 2) // 256), 1024) for a, b in rows]
    assert pairs[0, 0] == 0 and np.array_equal(np.diff(pairs[:, 0]), groups) and min(groups) >= 1
    assert np.array_equal(pairs[:, 1], pairs[:, 0])


def test_group_plan_of_the_edge_and_linear_cases_has_the_shapes_their_tests_rely_on():
    plan = mmd._group_plan(MC.edge_case(1)[1])
    assert sorted(plan["counts"].tolist()) == sorted(MC.EDGE_COUNTS) and sorted(plan["tiles"].tolist()) == [1, 1, 1, 2, 2, 3]
    plan = mmd._group_plan(MC.linear_case()[1])
    assert sorted(np.diff(plan["pairs"][:, 0]).tolist()) == [1, 1, 2]
    big = mmd._group_plan(np.repeat([1, 0], [524800, 524300]))
    assert big["pairs"][:, 0].tolist() == [0, 1024] and 524300 // 2 > 1024 * 256


def test_group_plan_empty_and_single():
    plan = mmd._group_plan(np.zeros(0, dtype=int))
    assert len(plan["all_conditions"]) == 0 and plan["offsets"].tolist() == [0] and plan["blocks"].shape == (1, 4)
    plan = mmd._group_plan(np.full(5, 9))
    assert plan["all_conditions"].tolist() == [9] and plan["offsets"].tolist() == [0, 5]
    assert plan["index"].tolist() == [0, 1, 2, 3, 4] and plan["blocks"].tolist() == [[0, 0, 0, 0], [1, 1, 0, 0]]


def test_errors_and_trivial_matrices_are_decided_before_any_launch():
    """none of these reaches the device: they pass on a machine without one"""
    latent = np.zeros((5, 3))
    single = np.array([4, 4, 9, 4, 4])                               # condition 9 has one row
    with pytest.raises(ZeroDivisionError):
        mmd.mmd2_matrix_one_pass(latent, single, alg='quadratic', sigma=2.0)
    with pytest.raises(ZeroDivisionError):
        mmd.mmd2_matrix_one_pass(latent, single, alg='quadratic', sigma=2.0, max_n=2)
    with pytest.raises(ZeroDivisionError):
        mmd.mmd2_block_terms(latent, single, sigma=2.0)
    with pytest.raises(AssertionError):
        mmd.mmd2_matrix_one_pass(latent, single, alg='linear', sigma=2.0)
    with pytest.raises(NotImplementedError):
        mmd.mmd2_matrix_one_pass(latent, np.array([0, 0, 1, 1, 1]), alg='cubic', sigma=2.0)
    result, conditions = mmd.mmd2_matrix_one_pass(np.zeros((0, 3)), np.zeros(0, dtype=int), sigma=2.0)
    assert result.shape == (0, 0) and len(conditions) == 0
    for alg in ('quadratic', 'linear'):
        result, conditions = mmd.mmd2_matrix_one_pass(latent, np.full(5, -6), alg=alg, sigma=2.0)
        assert np.array_equal(result, [[0.0]]) and conditions.tolist() == [-6]
    dc = MC.StubDC(latent, single)
    with pytest.raises(AssertionError):
        mmd._calculate_mmd2(dc, MC.condition_from_fn, mmd2_fn="unused.npy", alg='cubic', sigma=2.0, verbose=False)
    with pytest.raises(AssertionError):
        mmd._calculate_mmd2(dc, MC.condition_from_fn, mmd2_fn=None, sigma=2.0, verbose=False)
    assert dc.requested == []


def test_calculate_mmd2_single_condition_saves_and_prints_like_the_reference(tmp_path, capsys):
    latent, condition = np.zeros((4, 3)), np.full(4, 12)
    mmd2_fn, condition_fn = str(tmp_path / "mmd2.npy"), str(tmp_path / "cond.npy")
    result, conditions = mmd._calculate_mmd2(MC.StubDC(latent, condition), MC.condition_from_fn, mmd2_fn=mmd2_fn,
                                             condition_fn=condition_fn, parallel=True, sigma=2.0)
    assert np.array_equal(result, [[0.0]]) and conditions.tolist() == [12] and conditions.dtype == np.dtype('int')
    assert np.array_equal(np.load(mmd2_fn), result) and np.array_equal(np.load(condition_fn), conditions)
    assert capsys.readouterr().out.splitlines() == [
        "Estimating an MMD matrix...", "\talg: quadratic", "\tparallel: True", "\tmax_n: None", "\tconditions found: 1",
        "\tsigma: 2.0", "\tSaving MMD^2 to: " + mmd2_fn, "\tSaving conditions to: " + condition_fn, "\tDone."]


def test_install_swaps_calculate_mmd2_only_on_request():
    module = types.SimpleNamespace()
    assert mmd.install(module) is module
    assert module._estimate_mmd2 is mmd._estimate_mmd2 and not hasattr(module, "_calculate_mmd2")
    mmd.install(module, matrix=True)
    assert module._calculate_mmd2 is mmd._calculate_mmd2 and module.estimate_median_sigma is mmd.estimate_median_sigma


def test_c_abi_checks_scalars_and_sizes_the_workspace_on_the_host():
    """argument checks and the workspace formula of include/ava_hip.h run before any HIP call"""
    from ava_amd import _lib
    lib = _lib.load()
    plan = mmd._group_plan(MC.edge_case(1)[1])
    off, C = np.ascontiguousarray(plan["offsets"]), len(plan["counts"])
    blocks, pairs = plan["blocks"], plan["pairs"]
    need = lib.ava_mmd2_matrix_workspace_bytes
    assert need(off.ctypes.data, C, 0) == (int(blocks[-1, 1]) + 8) * 8
    assert need(off.ctypes.data, C, 1) == (int(pairs[-1, 1]) + 8) * 8
    single = np.array([0, 5, 6, 9], dtype=np.int64)                  # the middle condition has one row
    assert need(single.ctypes.data, 3, 0) == 0 and need(off.ctypes.data, 1, 0) == 0 and need(None, C, 0) == 0

    fake = 4096                                                      # never dereferenced: every call below is rejected

    def quad(z=8, offsets=off, C=C, total=int(blocks[-1, 0]), sigma=1.0, ws_bytes=1 << 20):
        return lib.ava_mmd2_matrix(fake, z, fake, offsets.ctypes.data, fake, C, fake, total, sigma, fake, fake, fake,
                                   ws_bytes, None)

    def lin(z=8, offsets=off, C=C, total=int(pairs[-1, 0]), sigma=1.0, ws_bytes=1 << 20):
        return lib.ava_mmd2_matrix_linear(fake, z, fake, offsets.ctypes.data, fake, C, fake, total, sigma, fake, fake,
                                          ws_bytes, None)
    for call in (quad, lin):
        assert call(z=0) == -1 and call(z=129) == -1 and call(sigma=0.0) == -1 and call(sigma=float("nan")) == -1
        assert call(C=1) == -1 and call(offsets=single, C=3) == -1
        assert call(total=call.__defaults__[3] + 1) == -1            # a table that disagrees with the offsets
        assert call(ws_bytes=64) == -3
    assert lib.ava_mmd2_matrix(fake, 8, fake, off.ctypes.data, fake, C, fake, int(blocks[-1, 0]), 1.0, None, fake, fake,
                               1 << 20, None) == -1
