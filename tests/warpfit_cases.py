"""Cases of tests/golden/warpfit.npz (written by tests/golden/make_golden_warpfit.py from the reference's
``ava.preprocessing.warping``): seeded synthetic spectrograms regenerated from the recipes below, so that the fixture
holds only parameters and results.  Also a numpy restatement of the reference's objectives (warping.py:148-163) for
many candidates at once, which pins the fixture to the recipe (tests/test_cpu_warpfit.py) and which the golden script
uses for its dense scans.

A spectrogram is a sum of WIDE Gaussian bumps in time with a per-row gain, plus a little hashed noise, warped by known
shifts and slopes: ``spec_n(u) = base((u - shift_n) / slope_n)``, so that ``spec_n(shift_n + slope_n j) = base(j)``.
Bump widths are at least 5 time bins and the shifts stay below a bump width: with narrow bumps the shift objective has
several local minima within the search span and the reference's own Powell ends in a bad one."""
import json

import numpy as np

from ava_amd import synthetic as syn

# centres and widths as fractions of T; shifts in time bins
RECIPES = {
    'amp_T130': dict(N=6, F=1, T=130, centres=[0.25, 0.5, 0.8], widths=[0.06, 0.09, 0.05], max_shift=4.0,
                     slopes=[0.93, 1.10], noise=0.01, salt=1201),
    'amp_T37': dict(N=6, F=1, T=37, centres=[0.3, 0.72], widths=[0.15, 0.17], max_shift=2.0, slopes=[0.95, 1.06],
                    noise=0.01, salt=1202),
    'spec_T130': dict(N=6, F=3, T=130, centres=[0.25, 0.5, 0.8], widths=[0.06, 0.09, 0.05], max_shift=4.0,
                      slopes=[0.93, 1.10], noise=0.01, salt=1203),
    'spec_T37': dict(N=6, F=3, T=37, centres=[0.3, 0.72], widths=[0.15, 0.17], max_shift=2.0, slopes=[0.95, 1.06],
                     noise=0.01, salt=1204),
}
CASE_NAMES = list(RECIPES)
DTYPES = ['float64', 'float32']

# the schedule of the end-to-end cases: three shift-only iterations, then five with decreasing penalties
SHIFT_LAMBDAS = [1e-2, 1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 0.0, 0.0]
SLOPE_LAMBDAS = [np.inf, np.inf, np.inf, 10.0, 1.0, 0.1, 0.0, 0.0]

# (shift_λ, slope_λ) of the recorded objective values and of the Powell minimisations
LOSS_LAMBDAS = [(1e-2, 0.5), (1e-2, np.inf)]
MIN_LAMBDAS = [(1e-2, np.inf), (0.0, 0.0), (1e-3, 1.0)]
N_POINTS = 16

# the first-round half-spans of ava_amd.warp_fit.minimize_warp about x0 (shift as a fraction of T; log slope), over which
# the golden script scans the objective densely (tests/test_cpu_warpfit.py pins them to the module's)
SEARCH_SHIFT_SPAN = 0.125
SEARCH_LOG_SLOPE_SPAN = 0.25


def true_warps(recipe):
    """the shifts and slopes the motifs were made with"""
    u = syn.u01(2 * recipe['N'], recipe['salt'])
    shifts = (2 * u[:recipe['N']] - 1) * recipe['max_shift']
    lo, hi = recipe['slopes']
    return shifts, lo + u[recipe['N']:] * (hi - lo)


def specs(name, dtype='float64'):
    """the spectrograms [N, F, T] of a case"""
    r = RECIPES[name]
    N, F, T = r['N'], r['F'], r['T']
    shifts, slopes = true_warps(r)
    gains = 0.5 + syn.u01(F * len(r['centres']), r['salt'] + 1).reshape(F, -1)
    u = (np.arange(T)[None, :] - shifts[:, None]) / slopes[:, None]                  # [N, T] template positions
    out = np.zeros((N, F, T))
    for k, (c, w) in enumerate(zip(r['centres'], r['widths'])):
        out += gains[None, :, k, None] * np.exp(-0.5 * ((u - c * T) / (w * T)) ** 2)[:, None, :]
    out += r['noise'] * syn.u01(N * F * T, r['salt'] + 2).reshape(N, F, T)
    return out.astype(dtype)


def apply_params(T):
    """shifts and slopes of the apply_warp cases: off both ends, slopes below and above 1, integer positions, and
    positions that hit T - 1 exactly"""
    shifts = np.array([0.0, -3.5, 5.25, 2.0, -(T - 1.0), 0.5])
    slopes = np.array([1.0, 0.9, 1.1, 1.0, 2.0, 0.75])
    return shifts, slopes


def loss_points(name):
    """the recorded (shift, log_slope) points [N, N_POINTS, 2]: hashed, with the origin and an integer shift first"""
    r = RECIPES[name]
    u = syn.u01(r['N'] * N_POINTS * 2, r['salt'] + 3).reshape(r['N'], N_POINTS, 2)
    pts = np.stack([(2 * u[..., 0] - 1) * 1.5 * r['max_shift'], (2 * u[..., 1] - 1) * 0.15], axis=-1)
    pts[:, 0] = 0.0
    pts[:, 1] = [3.0, 0.0]
    pts[:, 2] = [-float(r['T']), 0.05]                       # most positions below the first column
    return pts


def min_x0(name):
    """the starting points [N, 2] of the minimisations: the origin for the first half, hashed for the rest"""
    r = RECIPES[name]
    u = syn.u01(r['N'] * 2, r['salt'] + 4).reshape(r['N'], 2)
    x0 = np.stack([(2 * u[:, 0] - 1) * 1.0, (2 * u[:, 1] - 1) * 0.03], axis=1)
    x0[:r['N'] // 2] = 0.0
    return x0


def interp_rows(spec, pos):
    """scipy's interp1d(arange(T), spec, fill_value=(spec[:, 0], spec[:, -1])) at ``pos`` [...]: [F, ...]"""
    T = spec.shape[1]
    i = np.clip(np.ceil(pos), 1, T - 1).astype(np.int64)
    lo = i - 1
    val = (spec[:, i] - spec[:, lo]) * (pos - lo) + spec[:, lo]
    val = np.where(pos < 0, spec[:, :1].reshape((-1,) + (1,) * pos.ndim), val)
    return np.where(pos > T - 1, spec[:, -1:].reshape((-1,) + (1,) * pos.ndim), val)


def objective(spec, target, cands, shift_λ, slope_λ):
    """warping.py:148-163 at the candidates ``cands`` [C, 2] = (shift, log_slope) of one spectrogram [F, T]: [C]"""
    spec, target, cands = np.asarray(spec, np.float64), np.asarray(target, np.float64), np.asarray(cands, np.float64)
    T = spec.shape[1]
    slope = np.ones(len(cands)) if slope_λ == np.inf else np.exp(cands[:, 1])
    pos = cands[:, :1] + slope[:, None] * np.arange(T)[None, :]                      # [C, T]
    pred = interp_rows(spec, pos)                                                    # [F, C, T]
    loss = ((pred - target[:, None, :]) ** 2).sum(axis=(0, 2)) + shift_λ * cands[:, 0] ** 2
    return loss if slope_λ == np.inf else loss + slope_λ * cands[:, 1] ** 2


def spread(warped):
    """sum((warped - mean over spectrograms) ** 2) in float64"""
    w = np.asarray(warped, dtype=np.float64)
    return float(((w - w.mean(axis=0)) ** 2).sum())


def lam_key(shift_λ, slope_λ):
    return "l%g_%g" % (shift_λ, slope_λ)


def load():
    """the golden as a dict, JSON entries decoded"""
    from conftest import load_golden
    g = load_golden("warpfit.npz")
    return {k: (json.loads(str(v)) if k.endswith('.json') else v) for k, v in g.items()}
