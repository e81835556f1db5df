"""CPU tests of the warp parameter searches: everything of ava_amd.warp_search and of the
grouped fit's argument checks that launches no kernel -- the bin splits, the sampled settings, the schedule and group
checks, the anchor score and the choice of the best sample -- and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import warpsearch_cases as SC
from ava_amd import warp_fit as wf
from ava_amd import warp_search as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["ava_warpfit_group_loss", "ava_warpfit_group_pl_loss", "ava_warpfit_group_mean",
                    "ava_warpfit_group_pl_mean"]


@pytest.mark.parametrize("F,folds", [(10, (3, 1, 1)), (128, (3, 1, 1)), (13, (2, 2, 1)), (5, (3, 1, 1)), (7, (1, 1, 3))])
def test_every_bin_lands_in_exactly_one_part(F, folds):
    rng = np.random.RandomState(3)
    for _ in range(5):
        train, valid, test = ws.split_bins(F, *folds, rng)
        both = np.concatenate([train, valid, test])
        assert sorted(both.tolist()) == list(range(F))                              # each bin once
        for part in (train, valid, test):
            assert part.dtype.kind == 'i' and (np.diff(part) > 0).all()             # sorted, no repeats
        sizes = [len(p) for p in np.array_split(np.arange(F), sum(folds))]          # the proportions of np.array_split
        a, b = folds[0], folds[0] + folds[1]
        assert [len(train), len(valid), len(test)] == [sum(sizes[:a]), sum(sizes[a:b]), sum(sizes[b:])]


def test_a_split_is_the_permutation_of_its_random_state():
    train, valid, test = ws.split_bins(10, 3, 1, 1, np.random.RandomState(11))
    perm = np.random.RandomState(11).permutation(10)
    assert train.tolist() == sorted(perm[:6].tolist()) and valid.tolist() == sorted(perm[6:8].tolist())
    assert test.tolist() == sorted(perm[8:].tolist())


def test_too_few_bins_point_to_the_anchor_search():
    with pytest.raises(ValueError, match="anchor_point_warp_parameter_search"):
        ws.split_bins(4, 3, 1, 1, np.random.RandomState(0))
    with pytest.raises(ValueError, match="anchor_point_warp_parameter_search"):
        ws.search_plan(1)                                                            # an amplitude trace: one bin
    with pytest.raises(ValueError):
        ws.split_bins(10, 3, 0, 1, np.random.RandomState(0))


def test_settings_are_reproducible_and_inside_their_ranges():
    p = dict(samples_per_knot=4, n_valid_samples=3, knot_range=(-1, 3), shift_range=(0.5, 2.0), slope_range=(1e-2, 1e-1))
    one, two, other = ws.search_plan(20, p, seed=5), ws.search_plan(20, p, seed=5), ws.search_plan(20, p, seed=6)
    knots, a, b, schedules, splits = one
    assert knots.tolist() == [-1] * 4 + [0] * 4 + [1] * 4 + [2] * 4 and knots.dtype.kind == 'i'
    assert a.shape == b.shape == (16,) and len(schedules) == 16 and len(splits) == 16 and len(splits[0]) == 3
    assert (a >= 0.5).all() and (a <= 2.0).all() and (b >= 1e-2).all() and (b <= 1e-1).all()
    assert len(set(a.tolist())) == 16 and len(set(b.tolist())) == 16
    assert np.array_equal(a, two[1]) and np.array_equal(b, two[2]) and schedules == two[3]
    for s in range(16):
        for v in range(3):
            for x, y in zip(splits[s][v], two[4][s][v]):
                assert np.array_equal(x, y)
    assert not np.array_equal(a, other[1])
    assert any(not np.array_equal(splits[0][0][0], splits[s][v][0]) for s in range(16) for v in range(3))


def test_a_schedule_is_scale_times_base_and_minus_one_is_shift_only():
    base_shift, base_slope = list(wf.DEFAULT_SHIFT_LAMBDAS), list(wf.DEFAULT_SLOPE_LAMBDAS)
    knots, a, b, schedules, _ = ws.search_plan(10, dict(samples_per_knot=2), seed=1)
    assert knots.tolist() == [-1, -1, 0, 0, 1, 1]                                    # the reference's knot_range (-1, 2)
    for s in range(6):
        shift, slope = schedules[s]
        assert shift == [a[s] * v if v != 0 else 0.0 for v in base_shift]
        if knots[s] == -1:
            assert slope == [np.inf] * len(base_slope)
        else:
            assert slope == [v if (v == 0 or np.isinf(v)) else b[s] * v for v in base_slope]
            assert [np.isinf(v) for v in slope] == [np.isinf(v) for v in base_slope]
        wf.check_schedule(shift, slope)
    with pytest.raises(ValueError):
        ws.search_plan(10, dict(knot_range=(-2, 1)))
    with pytest.raises(ValueError):
        ws.search_plan(10, dict(samples_per_knot=0))


def test_the_inf_pattern_of_a_grouped_schedule_is_one_per_iteration():
    inf = np.inf
    a, b = wf.check_group_schedule([[0.1, 0.2], [0.0, 0.0]], [[inf, inf], [1.0, 0.0]], 2)
    assert a.shape == b.shape == (2, 2) and a.dtype == b.dtype == np.float64
    with pytest.raises(ValueError, match="every group or for none"):
        wf.check_group_schedule([[0.1, 0.2], [0.0, 0.0]], [[inf, 1.0], [1.0, 0.0]], 2)
    for shift, slope in [([[0.1, 0.2]], [[1.0]]), ([[0.1]], [[1.0]]), ([], []), ([[inf, 0.0]], [[1.0, 1.0]]),
                         ([[-1.0, 0.0]], [[1.0, 1.0]]), ([[0.0, 0.0]], [[-1.0, 1.0]]), ([[0.0, 0.0]], [[np.nan, 1.0]]),
                         ([0.0, 0.0], [1.0, 1.0])]:
        with pytest.raises(ValueError):
            wf.check_group_schedule(shift, slope, 2)


def test_group_lists_are_checked_on_the_host():
    good = wf.check_groups([(None, None), ([0, 2], [1]), None, (np.array([4]), np.array([0, 8]))], 5, 9)
    assert [(r.tolist(), b.tolist()) for r, b in good] == [(list(range(5)), list(range(9))), ([0, 2], [1]),
                                                           (list(range(5)), list(range(9))), ([4], [0, 8])]
    assert all(r.dtype == np.int32 and b.dtype == np.int32 for r, b in good)
    for bad in [[], [([], [0])], [([0], [])], [([1, 0], [0])], [([0, 0], [0])], [([0], [3, 3])], [([5], [0])],
                [([0], [9])], [([-1], [0])], [([0.5], [0])], [([[0]], [0])], [([0], [0], [0])]]:
        with pytest.raises(ValueError):
            wf.check_groups(bad, 5, 9)


def test_anchor_errors_against_the_restatement():
    rng = np.random.RandomState(2)
    for K in (2, 4):
        n, m, dur = 5, 3, 0.73
        y = np.tile(np.linspace(0, 1, K), (n, 1))
        x = y + 0.03 * rng.randn(n, K)
        x.sort(axis=1)
        anchors = np.sort(rng.uniform(-0.05, 0.8, size=(n, m)), axis=1)               # some beyond the outer knots
        got, want = ws.anchor_errors(x, y, anchors, dur), SC.anchor_errors(x, y, anchors, dur)
        assert isinstance(float(got), float) and abs(got / want - 1) <= 1e-12


def test_anchor_errors_by_hand():
    dur = 0.5
    base = np.array([0.1, 0.2, 0.35])
    offsets = np.array([0.0, 0.02, -0.015, 0.03])
    anchors = base[None, :] + offsets[:, None]
    # pure-shift knots whose shifts are the anchor offsets: x = y + offset / dur maps every file's anchors onto base
    y = np.tile([0.0, 1.0], (4, 1))
    x = y + (offsets / dur)[:, None]
    assert ws.anchor_errors(x, y, anchors, dur) <= 1e-9                              # ms: rounding only
    # identity knots: the printed null-warp value
    null = 1e3 * np.mean(np.abs(anchors.mean(axis=0, keepdims=True) - anchors))
    assert abs(ws.anchor_errors(y, y, anchors, dur) / null - 1) <= 1e-12
    assert null > 10.0


def test_best_warp_params_takes_the_best_median_validation_score():
    inf = np.inf
    res = {'knots': np.array([-1, 0, 1, 2]),
           'valid_rsq': np.array([[0.9, 0.1, 0.2], [0.5, 0.6, 0.4], [0.7, 0.55, 0.0], [0.3, 0.3, 0.99]]),
           'train_rsq': np.ones((4, 3)), 'test_rsq': np.array([1.0, 0.0, 0.0, 0.0]),
           'schedules': [([1.0, 0.0], [inf, inf]), ([2.0, 0.0], [inf, 0.5]), ([3.0, 0.0], [inf, 0.7]), ([4.0, 0.0], [inf, 0.9])]}
    assert ws.best_warp_params(res) == {'n_knots': 1, 'shift_lambdas': [3.0, 0.0], 'slope_lambdas': [inf, 0.7]}
    res['valid_rsq'][0] = [0.9, 0.8, 0.1]                                            # the shift-only sample now leads
    assert ws.best_warp_params(res) == {'n_knots': 0, 'shift_lambdas': [1.0, 0.0], 'slope_lambdas': [inf, inf]}
    wf.check_schedule(**{k.replace('lambdas', 'λs'): v for k, v in ws.best_warp_params(res).items() if k != 'n_knots'})


def test_install_points_a_module_here():
    class Module:
        pass
    m = ws.install(Module())
    assert m.cross_validation_warp_parameter_search is ws.cross_validation_warp_parameter_search
    assert m.anchor_point_warp_parameter_search is ws.anchor_point_warp_parameter_search


def test_the_grouped_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ava_hip.h")).read()
    source = open(os.path.join(ROOT, "autoencoded-vocal-analysis_amd", "csrc", "warp_fit.hip")).read()
    from ava_amd import _lib
    bound = open(_lib.__file__).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert re.search(r'extern "C" int %s\(' % name, source), name
        assert '"%s"' % name in bound, name
