"""Writes tests/golden/warpfit.npz: the reference's ``ava/preprocessing/warping.py`` (``apply_warp``, the two
objectives, Powell exactly as ``align_specs`` calls it, and ``align_specs`` end to end) on the synthetic cases of
tests/warpfit_cases.py.  Needs the reference package, numpy and scipy; run from the repository root as
``python tests/golden/make_golden_warpfit.py /path/to/reference``.  The tests only read the npz.

Per case and input dtype (float64, float32; ``loss`` and ``min`` for float64 only):
  ``apply``     ``apply_warp`` under parameters that run off both ends and hit column T - 1 exactly
  ``loss``      the objective functions at 16 recorded points per spectrogram, finite ``slope_λ`` and ``inf``; target:
                the mean spectrogram
  ``min``       ``minimize(objective, x0, method='Powell')`` per spectrogram for three λ pairs: end point and loss
  ``align``     ``align_specs`` under the schedule of warpfit_cases: parameters, the spread
                ``sum((warped - mean) ** 2)`` before and after, and the margin ``m`` of the end-to-end test:
                twice the relative difference between that spread and the spread of a second run with Powell's
                ``xtol`` and ``ftol`` tightened to 1e-8 (the module's ``minimize`` replaced by a partial), at least 1e-3

Validity checks made here, so that no test has to skip a case:
  * ``align_specs`` reduces the spread at least tenfold on every end-to-end case;
  * for every minimisation a dense scan of the objective over the first-round span of the device search (about ``x0``:
    ``shift ± T / 8``, and ``log slope ± 0.25`` pivoting about the middle column) finds nothing below Powell's loss
    beyond what Powell's own ``ftol`` = 1e-4 allows, and its lowest point lies within three scan cells of where Powell
    ended: Powell found the minimum of the span.
"""
import functools
import io
import json
import os
import sys
import warnings
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AVA_REFERENCE", "../reference"))

import warpfit_cases as FC                                      # noqa: E402
import ava.preprocessing.warping as W                           # noqa: E402
from scipy.interpolate import interp1d                          # noqa: E402
from scipy.optimize import minimize                             # noqa: E402

OUT = {}
SCAN_SHIFT_CELL, SCAN_SLOPE_CELL = 0.05, 0.005


def _interp(spec):
    """the interpolant of warping.py:112-113"""
    return interp1d(np.arange(spec.shape[1]), spec, assume_sorted=True, bounds_error=False,
                    fill_value=(spec[:, 0], spec[:, -1]))


def _objective(spec, target, shift_λ, slope_λ):
    """the objective align_specs builds (warping.py:123-128)"""
    if slope_λ == np.inf:
        return W._get_shift_objective(spec, target, _interp(spec), shift_λ)
    return W._get_linear_objective(spec, target, _interp(spec), shift_λ, slope_λ)


def _align(specs, tight):
    """align_specs under the schedule of the cases, quietly; ``tight``: Powell with xtol = ftol = 1e-8"""
    keep = W.minimize
    if tight:
        W.minimize = functools.partial(minimize, options=dict(xtol=1e-8, ftol=1e-8))
    try:
        with warnings.catch_warnings(), redirect_stdout(io.StringIO()):
            warnings.simplefilter("ignore")
            warped, wp = W.align_specs(specs, FC.SHIFT_LAMBDAS, FC.SLOPE_LAMBDAS, verbose=False)
    finally:
        W.minimize = keep
    assert warped is not None, "the reference's optimiser failed"
    return warped, wp


def _scan(spec, target, x0, shift_λ, slope_λ, T):
    """lowest point of a dense scan over the device search's first-round span: (loss, shift, log_slope)"""
    a = np.arange(-T * FC.SEARCH_SHIFT_SPAN, T * FC.SEARCH_SHIFT_SPAN + 1e-9, SCAN_SHIFT_CELL)
    if slope_λ == np.inf:
        cands = np.stack([x0[0] + a, np.full_like(a, x0[1])], axis=1)
        loss = FC.objective(spec, target, cands, shift_λ, slope_λ)
    else:
        b = np.arange(-FC.SEARCH_LOG_SLOPE_SPAN, FC.SEARCH_LOG_SLOPE_SPAN + 1e-9, SCAN_SLOPE_CELL)
        ls = x0[1] + b
        pivot = (np.exp(ls) - np.exp(x0[1])) * (0.5 * (T - 1))
        cands = np.stack([(x0[0] + a[:, None] - pivot[None, :]).ravel(), np.broadcast_to(ls, (len(a), len(b))).ravel()], axis=1)
        loss = np.concatenate([FC.objective(spec, target, c, shift_λ, slope_λ) for c in np.array_split(cands, 64)])
    k = int(np.argmin(loss))
    return float(loss[k]), float(cands[k, 0]), float(cands[k, 1])


def case(name, dtype):
    r = FC.RECIPES[name]
    N, T = r['N'], r['T']
    specs = FC.specs(name, dtype)
    key = "%s.%s" % (name, dtype)

    shifts, slopes = FC.apply_params(T)
    OUT[key + '.apply'] = W.apply_warp(specs, {'shifts': shifts, 'slopes': slopes})

    if dtype == 'float64':
        target = np.mean(specs, axis=0)
        OUT[key + '.target'] = target
        pts = FC.loss_points(name)
        for shift_λ, slope_λ in FC.LOSS_LAMBDAS:
            loss = np.array([[_objective(specs[n], target, shift_λ, slope_λ)(pts[n, c]) for c in range(FC.N_POINTS)]
                             for n in range(N)], dtype=np.float64)
            OUT["%s.loss.%s" % (key, FC.lam_key(shift_λ, slope_λ))] = loss

        x0 = FC.min_x0(name)
        for shift_λ, slope_λ in FC.MIN_LAMBDAS:
            xs, funs = [], []
            for n in range(N):
                res = minimize(_objective(specs[n], target, shift_λ, slope_λ), x0[n], method='Powell')    # warping.py:130
                assert res.success
                xs.append(res.x)
                funs.append(float(res.fun))
                # validity: Powell ended at the minimum of the span the device search covers
                lo, s_at, l_at = _scan(specs[n], target, x0[n], shift_λ, slope_λ, T)
                assert abs(res.x[0] - x0[n, 0]) < T * FC.SEARCH_SHIFT_SPAN, (key, n, res.x)
                assert lo >= res.fun * (1 - 1e-4), (key, n, shift_λ, slope_λ, lo, res.fun)
                if slope_λ == np.inf:
                    assert abs(s_at - res.x[0]) <= 3 * SCAN_SHIFT_CELL, (key, n, s_at, res.x)
                else:
                    assert abs(res.x[1] - x0[n, 1]) < FC.SEARCH_LOG_SLOPE_SPAN, (key, n, res.x)
                    mid = 0.5 * (T - 1)                         # the scan's shift axis moves the middle column
                    assert abs((s_at + np.exp(l_at) * mid) - (res.x[0] + np.exp(res.x[1]) * mid)) <= 3 * SCAN_SHIFT_CELL, \
                        (key, n, s_at, l_at, res.x)
                    assert abs(l_at - res.x[1]) <= 3 * SCAN_SLOPE_CELL, (key, n, l_at, res.x)
            OUT["%s.min_x.%s" % (key, FC.lam_key(shift_λ, slope_λ))] = np.array(xs)
            OUT["%s.min_loss.%s" % (key, FC.lam_key(shift_λ, slope_λ))] = np.array(funs)

    warped, wp = _align(specs, tight=False)
    warped2, _ = _align(specs, tight=True)
    assert warped.dtype == specs.dtype
    s0, s1, s2 = FC.spread(specs), FC.spread(warped), FC.spread(warped2)
    assert s1 * 10 <= s0, "%s: the reference reduces the spread only from %g to %g; fix the recipe" % (key, s0, s1)
    m = max(1e-3, 2 * abs(s1 - s2) / s2)
    OUT[key + '.align_shifts'], OUT[key + '.align_slopes'] = wp['shifts'], wp['slopes']
    OUT[key + '.align_spread'] = np.array([s0, s1, s2])
    OUT[key + '.align_margin'] = np.array(m)
    print("%-20s spread %.4g -> %.4g (tight %.4g)  m = %.3e  slopes %.3f..%.3f" %
          (key, s0, s1, s2, m, wp['slopes'].min(), wp['slopes'].max()))


def main():
    for name in FC.CASE_NAMES:
        for dtype in FC.DTYPES:
            case(name, dtype)
    OUT['case_names.json'] = np.array(json.dumps(FC.CASE_NAMES))
    path = os.path.join(HERE, "warpfit.npz")
    np.savez_compressed(path, **OUT)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
