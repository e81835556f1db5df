"""The piecewise-linear warp fit restated in numpy: the oracle of tests/test_gpu_warppl.py.
Neither affinewarp nor the reference's ``warping.py`` has this model, so the objective and the search are written out
here from their definition (the docstring of ``ava_amd.warp_fit``), on top of ``warpfit_cases.interp_rows`` and
``warpfit_cases.objective``, which tests/test_cpu_warpfit.py pins to the reference's interp1d and objectives.
tests/test_cpu_warppl.py checks this module against those and shows that the search recovers planted knots.

The planted recipe, in the style of ``warpfit_cases.RECIPES``: a base of WIDE Gaussian bumps (at least 5 bins) with
per-row gains; motif n is ``spec_n(u) = base(w_n^-1(u))`` with ``w_n`` piecewise linear through ``(t_k, t_k + d[n, k])``
on the template knots ``t_k`` (outer segments extrapolated), so that ``spec_n(w_n(j)) = base(j)``; the displacements
``d`` stay below a bump width; a little hashed noise is added to every motif."""
import numpy as np

import warpfit_cases as FC
from ava_amd import synthetic as syn

# the search constants of ava_amd.warp_fit, restated (tests/test_cpu_warppl.py pins them to the module's)
XTOL = 1e-4
GRID_KS, GRID_KL, LINE_KS, KNOT_KS = 3, 2, 7, 3
SHIFT_SPAN, LOG_SLOPE_SPAN = 0.125, 0.25
MAX_KNOTS = 16

# the outer bumps stay 3 widths clear of the ends: a motif whose outer knot lies off the grid reads held end columns there
PLANTED = dict(N=6, F=3, T=97, n_knots=2, centres=[0.2, 0.35, 0.5, 0.65, 0.8], widths=[0.06, 0.055, 0.06, 0.055, 0.06],
               max_move=3.0, noise=0.01, salt=1401)
# two shift-only iterations, two with penalties, three maximum-likelihood ones
SHIFT_LAMBDAS = [1e-2, 1e-2, 1e-3, 1e-3, 0.0, 0.0, 0.0]
SLOPE_LAMBDAS = [np.inf, np.inf, 1.0, 0.1, 0.0, 0.0, 0.0]


def knot_columns(T, K):
    """t_k = k (T - 1) / (K - 1)"""
    return np.arange(K) * (T - 1) / (K - 1)


def slopes(u, T):
    """s_k = (u_{k+1} - u_k) / (t_{k+1} - t_k) of knots u [..., K]: [..., K - 1]"""
    t = knot_columns(T, u.shape[-1])
    return (u[..., 1:] - u[..., :-1]) / (t[1:] - t[:-1])


def positions(u, T, fixed_slope=False):
    """p(j) of knots u [..., K] for the columns j = 0 .. T - 1: [..., T]; ``fixed_slope``: u_0 + j"""
    u = np.asarray(u, dtype=np.float64)
    K, j = u.shape[-1], np.arange(T)
    if fixed_slope:
        return u[..., :1] + 1.0 * j
    t = knot_columns(T, K)
    k = np.minimum(j * (K - 1) // (T - 1), K - 2)
    return u[..., k] + slopes(u, T)[..., k] * (j - t[k])


def objective(spec, target, cands, shift_λ, slope_λ):
    """sum((interp(spec)(p) - target) ** 2) + shift_λ u_0 ** 2 + slope_λ mean_k log(s_k) ** 2 at the candidates
    ``cands`` [C, K] of one spectrogram [F, T]: [C]; inf where some s_k <= 0.  ``slope_λ = inf``: the shift objective."""
    spec, target, cands = np.asarray(spec, np.float64), np.asarray(target, np.float64), np.asarray(cands, np.float64)
    T, K = spec.shape[1], cands.shape[1]
    fixed = slope_λ == np.inf
    pred = FC.interp_rows(spec, positions(cands, T, fixed))                          # [F, C, T]
    loss = ((pred - target[:, None, :]) ** 2).sum(axis=(0, 2)) + shift_λ * cands[:, 0] ** 2
    if fixed:
        return loss
    s = slopes(cands, T)
    with np.errstate(invalid='ignore', divide='ignore'):
        sq = np.zeros(len(cands))
        for k in range(K - 1):
            sq = sq + np.log(s[:, k]) ** 2
        loss = loss + slope_λ * (sq / (K - 1))
    return np.where((s <= 0).any(axis=1), np.inf, loss)


def apply_warp(specs, knots):
    """warped [N, F, T] of specs [N, F, T] under knots [N, K], in the dtype of ``specs``"""
    specs = np.asarray(specs)
    T = specs.shape[2]
    out = np.stack([FC.interp_rows(specs[n].astype(np.float64), positions(knots[n], T)) for n in range(len(specs))])
    return out.astype(specs.dtype)


def _offsets(k):
    """0, -1, +1, -2, +2, ..., -k, +k"""
    return np.array([0] + [s * o for o in range(1, k + 1) for s in (-1, 1)], dtype=np.float64)


def _argmin(loss):
    """lowest index of the least loss, NaN never winning"""
    return int(np.argmin(np.where(np.isnan(loss), np.inf, loss)))


def search_rounds(T, fixed_slope):
    ks, kl = (LINE_KS, 0) if fixed_slope else (GRID_KS, GRID_KL)
    hs, hl = T * SHIFT_SPAN / ks, LOG_SLOPE_SPAN / max(kl, 1)
    rounds = []
    while hs >= XTOL or (not fixed_slope and hl >= XTOL):
        rounds.append((hs, hl))
        hs, hl = hs / 2, hl / 2
    return ks, kl, rounds


def knot_rounds(T, K):
    h, rounds = T * SHIFT_SPAN / (KNOT_KS * (K - 1)), []
    while h >= XTOL:
        rounds.append(h)
        h = h / 2
    return rounds


def stage_a(spec, target, x, shift_λ, slope_λ):
    """the shift-and-slope grid search of ``minimize_warp`` for one spectrogram from x = (shift, log slope)"""
    T = spec.shape[1]
    ks, kl, rounds = search_rounds(T, slope_λ == np.inf)
    oa, ob = np.repeat(_offsets(ks), 2 * kl + 1), np.tile(_offsets(kl), 2 * ks + 1)
    x = np.array(x, dtype=np.float64)
    for hs, hl in rounds:
        ls = np.where(ob != 0, x[1] + ob * hl, x[1])
        shift = x[0] + oa * hs - np.where(ob != 0, (np.exp(ls) - np.exp(x[1])) * (0.5 * (T - 1)), 0.0)
        cands = np.stack([shift, ls], axis=1)
        x = cands[_argmin(FC.objective(spec, target, cands, shift_λ, slope_λ))]
    return x


def stage_b(spec, target, u, shift_λ, slope_λ):
    """the coordinate search over single knots for one spectrogram from the knots u [K]: ``(u, loss)``"""
    T, K = spec.shape[1], len(u)
    u, off, loss = np.array(u, dtype=np.float64), _offsets(KNOT_KS), None
    for h in knot_rounds(T, K):
        for k in range(K):
            cands = np.tile(u, (len(off), 1))
            cands[1:, k] = u[k] + off[1:] * h
            losses = objective(spec, target, cands, shift_λ, slope_λ)
            best = _argmin(losses)
            u, loss = cands[best], losses[best]
    return u, loss


def check_knots(T, K):
    if K < 2 or K > MAX_KNOTS or T - 1 < 2 * (K - 1):
        raise ValueError("unsupported number of knots")


def align_specs(specs, shift_λs, slope_λs, n_knots):
    """``ava_amd.warp_fit.align_specs(..., n_knots=n_knots)`` in numpy, float64: ``(warped, knots [N, K])``"""
    specs = np.asarray(specs, dtype=np.float64)
    N, F, T = specs.shape
    K = n_knots + 2
    check_knots(T, K)
    t = knot_columns(T, K)
    x = np.zeros((N, 2))
    knots = np.tile(t, (N, 1))
    warped = specs.copy()
    for shift_λ, slope_λ in zip(shift_λs, slope_λs):
        target = warped.mean(axis=0)
        for n in range(N):
            x[n] = stage_a(specs[n], target, x[n], shift_λ, slope_λ)
            if slope_λ == np.inf:
                x[n, 1] = 0.0
            knots[n] = x[n, 0] + np.exp(x[n, 1]) * t
            if slope_λ != np.inf:
                knots[n], _ = stage_b(specs[n], target, knots[n], shift_λ, slope_λ)
        warped = apply_warp(specs, knots)
    return warped, knots


# ---- the planted recipe ------------------------------------------------------------------------------------------------

def planted_knots(r=PLANTED):
    """the knots [N, K] the motifs were made with: t_k + d[n, k], |d| <= max_move"""
    K = r['n_knots'] + 2
    d = (2 * syn.u01(r['N'] * K, r['salt']).reshape(r['N'], K) - 1) * r['max_move']
    return knot_columns(r['T'], K) + d


def planted_specs(r=PLANTED, dtype='float64'):
    """the motifs [N, F, T] of the recipe"""
    N, F, T = r['N'], r['F'], r['T']
    t, u = knot_columns(T, r['n_knots'] + 2), planted_knots(r)
    gains = 0.5 + syn.u01(F * len(r['centres']), r['salt'] + 1).reshape(F, -1)
    cols = np.arange(T, dtype=np.float64)
    out = np.zeros((N, F, T))
    for n in range(N):
        # w_n^-1: source position -> template position, the outer segments extrapolated
        k = np.clip(np.searchsorted(u[n], cols, side='right') - 1, 0, len(t) - 2)
        v = t[k] + (cols - u[n, k]) * (t[k + 1] - t[k]) / (u[n, k + 1] - u[n, k])
        for b, (c, w) in enumerate(zip(r['centres'], r['widths'])):
            out[n] += gains[:, b, None] * np.exp(-0.5 * ((v - c * T) / (w * T)) ** 2)[None, :]
    out += r['noise'] * syn.u01(N * F * T, r['salt'] + 2).reshape(N, F, T)
    return out.astype(dtype)


def knot_error(fitted, planted):
    """max |fitted - planted| once the per-knot mean over motifs is removed from each: a displacement shared by all
    motifs moves the template, not the alignment"""
    a, b = np.asarray(fitted, np.float64), np.asarray(planted, np.float64)
    return float(np.abs((a - a.mean(axis=0)) - (b - b.mean(axis=0))).max())
