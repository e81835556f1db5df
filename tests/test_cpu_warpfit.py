"""Host logic of the warp-fit row: the knots convention, the schedule checks, the search plan,
``install`` and the fixture pin.  No library call: everything here runs without the device."""
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest

import warpfit_cases as FC
from conftest import ROOT


@pytest.fixture(scope="module")
def G():
    return FC.load()


def test_knots_from_warp_params_on_hand_values():
    from ava_amd import warp_fit as wf
    xk, yk = wf.knots_from_warp_params({'shifts': np.array([0.0, 4.0, -2.0]), 'slopes': np.array([1.0, 1.25, 0.5])}, 40)
    assert xk.shape == yk.shape == (3, 2) and xk.dtype == yk.dtype == np.float64
    assert np.array_equal(yk, np.tile([0.0, 1.0], (3, 1)))
    assert np.array_equal(xk, np.array([[0.0, 1.0], [0.1, 1.35], [-0.05, 0.45]]))
    with pytest.raises(ValueError):
        wf.knots_from_warp_params({'shifts': np.zeros(2), 'slopes': np.array([1.0, 0.0])}, 40)
    with pytest.raises(ValueError):
        wf.knots_from_warp_params({'shifts': np.zeros(2), 'slopes': np.ones(3)}, 40)


def test_knots_round_trip_through_the_dataset_inverse_warp():
    """template bin j (quantile j / T) must come out of ``_get_unwarped_times`` at frame ``shift + slope * j``"""
    from ava_amd import warp_fit as wf
    from ava_amd import warped_window as ww
    T = 50
    shifts, slopes = np.array([1.5, -3.0, 0.0]), np.array([0.9, 1.1, 1.0])
    xk, yk = wf.knots_from_warp_params({'shifts': shifts, 'slopes': slopes}, T)
    ds = ww.DeviceWarpedWindowDataset.__new__(ww.DeviceWarpedWindowDataset)
    ds.x_knots, ds.y_knots = xk, yk
    j = np.arange(-5, T + 5, dtype=np.float64)              # the dataset draws beyond [0, 1] too
    for n in range(3):
        frames = ds._get_unwarped_times(j / T, n) * T
        assert np.abs(frames - (shifts[n] + slopes[n] * j)).max() <= 1e-12 * T


def test_bin_time_convention_of_the_fit_inputs():
    """bin j of the fit inputs is the frame at j * frame_step: template_dur is num_time_bins frame steps"""
    from ava_amd import segment as seg
    from ava_amd import warped_window as ww
    p, fs = dict(nperseg=512, noverlap=256), 32000
    lengths = [16000, 15000]
    bins = int(seg.frame_count(np.array(lengths), 512, 256).min())
    assert ww.template_duration(lengths, fs, p) == bins * seg.frame_step(fs, 512, 256)


def test_schedule_validation():
    from ava_amd import warp_fit as wf
    a, b = wf.check_schedule([1.0, 0.5, 0], [np.inf, 2, 0.0])
    assert a == [1.0, 0.5, 0.0] and b == [np.inf, 2.0, 0.0] and all(type(v) is float for v in a + b)
    wf.check_schedule(wf.DEFAULT_SHIFT_LAMBDAS, wf.DEFAULT_SLOPE_LAMBDAS)
    assert wf.DEFAULT_SLOPE_LAMBDAS[0] == np.inf and wf.DEFAULT_SLOPE_LAMBDAS[-1] == 0.0
    with pytest.raises(ValueError, match="one entry per iteration"):
        wf.check_schedule([1.0, 0.5], [np.inf])
    with pytest.raises(ValueError, match="empty"):
        wf.check_schedule([], [])
    with pytest.raises(ValueError, match="only slope_λ may be inf"):
        wf.check_schedule([np.inf], [1.0])
    for bad in ([np.nan], [-1.0]):
        with pytest.raises(ValueError):
            wf.check_schedule(bad, [1.0])
        with pytest.raises(ValueError):
            wf.check_schedule([1.0], bad)


def test_search_plan():
    """the grid steps halve from the documented spans down to Powell's xtol, and the cases module scans those spans"""
    from ava_amd import warp_fit as wf
    assert (wf.SHIFT_SPAN, wf.LOG_SLOPE_SPAN) == (FC.SEARCH_SHIFT_SPAN, FC.SEARCH_LOG_SLOPE_SPAN)
    for T in (37, 130, 512):
        ks, kl, rounds = wf.search_rounds(T, False)
        assert (ks, kl) == (wf.GRID_KS, wf.GRID_KL)
        assert rounds[0] == (T * wf.SHIFT_SPAN / ks, wf.LOG_SLOPE_SPAN / kl)
        assert all(b[0] == a[0] / 2 and b[1] == a[1] / 2 for a, b in zip(rounds, rounds[1:]))
        assert max(rounds[-1]) >= wf.XTOL > max(rounds[-1]) / 2
        ks, kl, line = wf.search_rounds(T, True)
        assert (ks, kl) == (wf.LINE_KS, 0) and line[0][0] == T * wf.SHIFT_SPAN / ks
        assert line[-1][0] >= wf.XTOL > line[-1][0] / 2


def test_module_imports_without_the_optional_packages():
    code = textwrap.dedent('''
        import sys
        for m in ("affinewarp", "umap", "h5py", "bokeh"):
            sys.modules[m] = None
        import ava_amd.warp_fit as wf
        print(sorted(n for n in wf.__all__ if not hasattr(wf, n)), wf.WARNING_MSG)
    ''')
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.startswith("[] ava.preprocessing.warping is experimental")


def test_install_points_the_reference_names_here(tmp_path):
    from ava_amd import warp_fit as wf
    mod = types.ModuleType("warping")
    assert wf.install(mod) is mod
    assert mod.align_specs is wf.align_specs and mod.apply_warp is wf.apply_warp
    # the default target, on a stand-in for the reference package found behind this repository on sys.path
    ref = tmp_path / "reference"
    (ref / "ava" / "preprocessing").mkdir(parents=True)
    (ref / "ava" / "__init__.py").write_text('__version__ = "0.3.1"\n')
    (ref / "ava" / "preprocessing" / "__init__.py").write_text("")
    (ref / "ava" / "preprocessing" / "warping.py").write_text(
        "def apply_warp(*a, **k):\n    pass\n\n\ndef align_specs(*a, **k):\n    pass\n\n\ndef _get_shift_objective():\n    pass\n")
    code = textwrap.dedent('''
        import ava.preprocessing.warping as w
        import ava_amd.warp_fit as wf
        own = w._get_shift_objective
        assert wf.install() is w
        print(w.align_specs.__module__, w.apply_warp.__module__, w._get_shift_objective is own, w.__file__)
    ''')
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, str(ref)])),
                         cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = res.stdout.split()
    assert out[:3] == ["ava_amd.warp_fit", "ava_amd.warp_fit", "True"] and out[3].startswith(str(ref))


def test_dataset_fit_argument_is_checked():
    from ava_amd import warped_window as ww
    with pytest.raises(AssertionError):
        ww.DeviceWarpedWindowDataset([], {}, fit='powell')
    with pytest.raises(AssertionError):
        ww.get_warped_window_data_loaders([], {}, fit='powell')


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_numpy_objective_equals_the_golden_losses(name, G):
    """the fixture belongs to the recipe: warpfit_cases.objective on the regenerated spectrograms gives the losses the
    reference's objective functions gave, within the summation-order bound 4 F T 2^-52 of the device test"""
    r = FC.RECIPES[name]
    specs, pts = FC.specs(name), FC.loss_points(name)
    target = specs.mean(axis=0)
    assert np.array_equal(target, G[name + '.float64.target'])
    bound = 4 * r['F'] * r['T'] * 2.0 ** -52
    for shift_λ, slope_λ in FC.LOSS_LAMBDAS:
        want = G["%s.float64.loss.%s" % (name, FC.lam_key(shift_λ, slope_λ))]
        got = np.stack([FC.objective(specs[n], target, pts[n], shift_λ, slope_λ) for n in range(r['N'])])
        assert got.shape == want.shape == (r['N'], FC.N_POINTS)
        rel = float(np.abs(got / want - 1).max())
        print("%s λ=(%g, %g): max rel %.3e (bound %.3e)" % (name, shift_λ, slope_λ, rel, bound))
        assert rel <= bound


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_fixture_recipe_keeps_the_stated_margins(name):
    """bump widths of at least 5 bins and shifts below a bump width"""
    r = FC.RECIPES[name]
    assert min(r['widths']) * r['T'] >= 5.0 and r['max_shift'] < min(r['widths']) * r['T']
    shifts, slopes = FC.true_warps(r)
    assert np.abs(shifts).max() <= r['max_shift'] and slopes.min() >= r['slopes'][0] and slopes.max() <= r['slopes'][1]
