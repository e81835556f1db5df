"""Host side of the piecewise-linear warp fit: the numpy oracle of tests/warppl_cases.py
against the pinned shift-and-slope objective, its search on planted knots (which shows the recipe is well-posed), the
search plan and the knots convention of ``ava_amd.warp_fit``.  Nothing here launches a kernel."""
import numpy as np
import pytest

import warpfit_cases as FC
import warppl_cases as PC


@pytest.mark.parametrize("name", ['spec_T37', 'spec_T130', 'amp_T130'])
def test_two_knots_are_the_shift_and_slope_objective(name):
    """K = 2 at u = (shift, shift + exp(log slope) (T - 1)) against warpfit_cases.objective, to 1e-14 relative"""
    r = FC.RECIPES[name]
    specs, pts, T = FC.specs(name), FC.loss_points(name), r['T']
    target = specs.mean(axis=0)
    for shift_λ, slope_λ in [(1e-2, 0.5), (1e-2, np.inf), (0.0, 0.0)]:
        worst = 0.0
        for n in range(r['N']):
            u = np.stack([pts[n, :, 0], pts[n, :, 0] + np.exp(pts[n, :, 1]) * (T - 1)], axis=1)
            got = PC.objective(specs[n], target, u, shift_λ, slope_λ)
            want = FC.objective(specs[n], target, pts[n], shift_λ, slope_λ)
            worst = max(worst, float(np.abs(got / want - 1).max()))
        print("%s λ=(%g, %g): max rel %.3e" % (name, shift_λ, slope_λ, worst))
        assert worst <= 1e-14


def test_positions_on_and_between_the_knots():
    T, K = 13, 4                                             # t = 0, 4, 8, 12: columns fall exactly on the knots
    u = np.array([-1.0, 4.5, 7.0, 13.0])
    p = PC.positions(u, T)
    assert np.array_equal(PC.knot_columns(T, K), [0.0, 4.0, 8.0, 12.0])
    assert np.array_equal(p[[0, 4, 8, 12]], u)
    assert np.allclose(p[[2, 6, 10]], [1.75, 5.75, 10.0], rtol=0, atol=1e-15)
    assert np.array_equal(PC.positions(u, T, fixed_slope=True), -1.0 + np.arange(T))
    q = PC.positions(np.array([0.5, 3.0, 9.0]), 10)         # T - 1 not divisible by K - 1: t = 0, 4.5, 9
    assert np.allclose(q[[0, 4, 5, 9]], [0.5, 0.5 + 2.5 / 4.5 * 4, 3.0 + 6.0 / 4.5 * 0.5, 9.0], rtol=0, atol=1e-14)


def test_knots_out_of_order_cost_infinity():
    specs = PC.planted_specs()
    target, T = specs.mean(axis=0), specs.shape[2]
    t = PC.knot_columns(T, 4)
    cands = np.stack([t, t + [0.0, 40.0, 0.0, 0.0], t + [0.0, 32.0, 0.0, 0.0], t + [0.0, 0.0, 0.0, -33.0], t + 0.25])
    for slope_λ in (0.0, 0.5):
        loss = PC.objective(specs[0], target, cands, 0.01, slope_λ)
        assert np.isfinite(loss[[0, 4]]).all() and np.isposinf(loss[[1, 2, 3]]).all()         # crossed, equal, crossed
    assert np.isfinite(PC.objective(specs[0], target, cands, 0.01, np.inf)).all()            # slope 1 whatever the knots


def test_search_plan_matches_the_module():
    from ava_amd import warp_fit as wf
    assert (PC.XTOL, PC.GRID_KS, PC.GRID_KL, PC.LINE_KS, PC.KNOT_KS, PC.SHIFT_SPAN, PC.LOG_SLOPE_SPAN) == \
        (wf.XTOL, wf.GRID_KS, wf.GRID_KL, wf.LINE_KS, wf.KNOT_KS, wf.SHIFT_SPAN, wf.LOG_SLOPE_SPAN)
    for T, K in [(97, 4), (128, 6), (512, 16), (37, 3)]:
        rounds = wf.knot_rounds(T, K)
        assert rounds == PC.knot_rounds(T, K)
        assert rounds[0] == T * wf.SHIFT_SPAN / (wf.KNOT_KS * (K - 1))
        assert all(b == a / 2 for a, b in zip(rounds, rounds[1:])) and rounds[-1] >= wf.XTOL > rounds[-1] / 2
        assert np.array_equal(wf.knot_columns(T, K), PC.knot_columns(T, K))
        assert wf.search_rounds(T, False) == PC.search_rounds(T, False) and wf.search_rounds(T, True) == PC.search_rounds(T, True)


def test_knots_from_warp_params_with_knots():
    from ava_amd import warp_fit as wf
    from ava_amd import warped_window as ww
    T = 41
    u = np.array([[0.0, 10.0, 20.0, 30.0, 40.0], [-2.0, 9.0, 21.5, 30.0, 43.0]])
    xk, yk = wf.knots_from_warp_params({'knots': u, 'shifts': np.zeros(2), 'slopes': np.ones(2)}, T)
    assert xk.shape == yk.shape == (2, 5) and xk.dtype == yk.dtype == np.float64
    assert np.array_equal(xk, u / T) and np.array_equal(yk, np.tile(np.arange(5) * 10.0 / T, (2, 1)))
    # through the dataset's inverse warp: template bin j comes out at frame p(j), the outer segments extrapolated
    ds = ww.DeviceWarpedWindowDataset.__new__(ww.DeviceWarpedWindowDataset)
    ds.x_knots, ds.y_knots = xk, yk
    j = np.arange(T, dtype=np.float64)
    for n in range(2):
        assert np.abs(ds._get_unwarped_times(j / T, n) * T - PC.positions(u[n], T)).max() <= 1e-12 * T
    beyond = ds._get_unwarped_times(np.array([-4.0, 44.0]) / T, 1) * T
    assert np.allclose(beyond, [-2.0 - 4 * 1.1, 43.0 + 4 * 1.3], rtol=0, atol=1e-12 * T)
    with pytest.raises(ValueError):
        wf.knots_from_warp_params({'knots': np.array([[0.0, 5.0, 5.0, 9.0]])}, 10)
    with pytest.raises(ValueError):
        wf.knots_from_warp_params({'knots': np.zeros(4)}, 10)


def test_planted_recipe_keeps_the_stated_margins():
    r = PC.PLANTED
    T = r['T']
    assert min(r['widths']) * T >= 5.0 and r['max_move'] < min(r['widths']) * T
    assert min(r['centres']) * T >= 3 * max(r['widths']) * T and (1 - max(r['centres'])) * T >= 3 * max(r['widths']) * T
    u, t = PC.planted_knots(), PC.knot_columns(T, r['n_knots'] + 2)
    assert u.shape == (r['N'], 4) and np.abs(u - t).max() <= r['max_move'] and (np.diff(u, axis=1) > 0).all()
    assert len(PC.SHIFT_LAMBDAS) == len(PC.SLOPE_LAMBDAS) and 6 <= len(PC.SHIFT_LAMBDAS) <= 8
    assert PC.SHIFT_LAMBDAS[-1] == PC.SLOPE_LAMBDAS[-1] == 0.0
    # the recipe's own inverse: warping motif n by its planted knots gives the base back, up to noise and interpolation
    specs = PC.planted_specs()
    assert FC.spread(PC.apply_warp(specs, u)) <= 0.002 * FC.spread(specs)
    PC.check_knots(5, 3)
    for T_, K in [(4, 3), (97, 17), (97, 1)]:
        with pytest.raises(ValueError):
            PC.check_knots(T_, K)


def test_numpy_search_recovers_the_planted_knots():
    """what makes the inputs of the device test well-posed: from the unaligned motifs the search ends within 0.5 bins of
    the planted knots and within a factor of two of the spread AT the planted knots (the noise floor)"""
    specs, planted = PC.planted_specs(), PC.planted_knots()
    warped, knots = PC.align_specs(specs, PC.SHIFT_LAMBDAS, PC.SLOPE_LAMBDAS, PC.PLANTED['n_knots'])
    floor, got, err = FC.spread(PC.apply_warp(specs, planted)), FC.spread(warped), PC.knot_error(knots, planted)
    print("spread: unaligned %.4g, fitted %.4g, at the planted knots %.4g; knot error %.3f bins"
          % (FC.spread(specs), got, floor, err))
    assert (np.diff(knots, axis=1) > 0).all()
    assert err <= 0.5 and got <= 2 * floor
