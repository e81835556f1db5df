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


# ---- the bits of the loss, apply and grouped-mean kernels (tests/golden/warpfit_bits.npz) ---------------------------------
# main: three row passes 4 + 4 + 1, three candidate blocks (the last holds 3 of 8), columns past one 64-lane stride;
# grouped: the shape and groups of the grouped-kernel tests; cap: T and K at their caps, the loss kernels' LDS over 64 KB.
# A group is (rows, bins); every shape has three, so that the per-group λ below serve all of them.
BITS_SHAPES = {
    'main': (dict(N=3, F=9, T=200, C=19, K=4), [([1], [4]), ([0, 2], [0, 2, 3, 5, 8]), (None, None)], 7101),
    'grouped': (None, None, 7201),                           # warpsearch_cases.KERNEL_SHAPE / KERNEL_GROUPS
    'cap': (dict(N=2, F=2, T=512, C=9, K=16), [([1], [1]), ([0], None), (None, None)], 7301),
}
BITS_LAMBDAS = {'finite': (0.01, 0.5), 'inf': (0.01, np.inf)}        # the plain entry points' (shift_λ, slope_λ)


def bits_record():
    """``{key: int64 bit patterns}`` of what the loss, apply and grouped-mean entry points of csrc/warp_fit.hip give,
    called through the C ABI alone, on hashed inputs: for every shape of ``BITS_SHAPES`` and both dtypes the plain and
    grouped losses of both forms under a finite ``slope_λ`` and under ``inf``, the grouped ones also with ``raw = 1``;
    at the cap shape both apply kernels; at the grouped shape the three modes of the grouped mean.  Candidate [0, 1] of
    every knots batch has knots 1 and 2 swapped: crossed, ``+inf`` unless ``slope_λ = inf``.  A float32 output's 32 bits
    are widened to int64.  Needs the device."""
    import ctypes

    import torch

    import warpsearch_cases as SC
    from ava_amd import _lib
    from ava_amd.warp_fit import check_groups

    lib, st = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                          # noqa: E731
    new = lambda *shape: torch.full(shape, -123.0, dtype=torch.float64, device="cuda")       # noqa: E731
    out = {}

    def keep(key, t):
        bits = t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)
        out[key] = bits.cpu().numpy().astype(np.int64)

    for name, (shape, groups, salt) in BITS_SHAPES.items():
        if shape is None:
            shape, groups = SC.KERNEL_SHAPE, SC.KERNEL_GROUPS
        N, F, T, C, K = (shape[k] for k in 'NFTCK')
        groups = check_groups(groups, N, F)
        rows, bins = [g[0] for g in groups], [g[1] for g in groups]
        row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        bin_off = np.concatenate([[0], np.cumsum([len(b) for b in bins])]).astype(np.int32)
        G, V, max_bins = len(groups), int(row_off[-1]), max(len(b) for b in bins)
        row_src, all_bins = dev(np.concatenate(rows)), dev(np.concatenate(bins))
        row_group = dev(np.repeat(np.arange(G, dtype=np.int32), np.diff(row_off)))
        d_row_off, d_bin_off = dev(row_off), dev(bin_off)
        target = dev(syn.u01(F * T, salt + 1))
        targets = dev(syn.u01(int(bin_off[-1]) * T, salt + 2))
        knots = SC.hashed_knots(max(N, V), C, T, K, salt + 4)
        knots[0, 1, [1, 2]] = knots[0, 1, [2, 1]]
        cands = {'ss': dev(SC.hashed_params(max(N, V), C, T, salt + 3)), 'pl': dev(knots)}
        x = SC.hashed_params(max(N, V), 1, T, salt + 5)[:, 0, :]
        params = dev(np.stack([x[:, 0], np.exp(x[:, 1])], axis=1))                            # (shift, slope)
        one_knots = dev(SC.hashed_knots(max(N, V), 1, T, K, salt + 6)[:, 0, :] * 1.0)
        for code, dtype in enumerate(('float32', 'float64')):
            specs = dev(syn.u01(N * F * T, salt).reshape(N, F, T).astype(dtype))
            head = (specs.data_ptr(), code, N, F, T)
            plan = head + (row_src.data_ptr(), row_group.data_ptr(), d_bin_off.data_ptr(), all_bins.data_ptr(), V,
                           targets.data_ptr())
            for form, cand in cands.items():
                k = (K,) if form == 'pl' else ()
                plain = lib.ava_warpfit_pl_loss if form == 'pl' else lib.ava_warpfit_loss
                grouped = lib.ava_warpfit_group_pl_loss if form == 'pl' else lib.ava_warpfit_group_loss
                for lam, (shift_λ, slope_λ) in BITS_LAMBDAS.items():
                    loss = new(N, C)
                    assert plain(*head, target.data_ptr(), cand.data_ptr(), C, *k, shift_λ, slope_λ, loss.data_ptr(), st) == 0
                    keep("%s.%s.%s_loss.%s" % (name, dtype, form, lam), loss)
                    fixed = slope_λ == np.inf
                    d_shift = dev(np.array(SC.KERNEL_SHIFT_LAMBDAS))
                    d_slope = dev(np.array([np.inf] * G if fixed else SC.KERNEL_SLOPE_LAMBDAS))
                    loss = new(V, C)
                    assert grouped(*plan, cand.data_ptr(), C, *k, d_shift.data_ptr(), d_slope.data_ptr(), int(fixed), 0,
                                   loss.data_ptr(), st) == 0
                    keep("%s.%s.group_%s_loss.%s" % (name, dtype, form, lam), loss)
                loss = new(V)
                assert grouped(*plan, None, 1, *k, None, None, 0, 1, loss.data_ptr(), st) == 0
                keep("%s.%s.group_%s_loss.raw" % (name, dtype, form), loss)
            if name == 'cap':                                # columns over the apply kernels' stride of 256, K = 16
                warped = torch.full_like(specs, -123.0)
                assert lib.ava_warpfit_apply(*head, params.data_ptr(), warped.data_ptr(), st) == 0
                keep("%s.%s.ss_apply" % (name, dtype), warped)
                warped = torch.full_like(specs, -123.0)
                assert lib.ava_warpfit_pl_apply(*head, one_knots.data_ptr(), K, warped.data_ptr(), st) == 0
                keep("%s.%s.pl_apply" % (name, dtype), warped)
            if name != 'grouped':
                continue
            mean = head + (row_src.data_ptr(), d_row_off.data_ptr(), d_bin_off.data_ptr(), all_bins.data_ptr(), G, max_bins)
            for mode in ('ss', 'pl', 'raw'):
                tgt = torch.full_like(targets, -123.0)
                if mode == 'pl':
                    rc = lib.ava_warpfit_group_pl_mean(*mean, one_knots.data_ptr(), K, 0, tgt.data_ptr(), st)
                else:
                    rc = lib.ava_warpfit_group_mean(*mean, params.data_ptr() if mode == 'ss' else None, int(mode == 'raw'),
                                                    tgt.data_ptr(), st)
                assert rc == 0
                keep("%s.%s.group_mean.%s" % (name, dtype, mode), tgt)
    torch.cuda.synchronize()
    return out


def load():
    """the golden as a dict, JSON entries decoded"""
    from conftest import load_golden
    g = load_golden("warpfit.npz")
    return {k: (json.loads(str(v)) if k.endswith('.json') else v) for k, v in g.items()}
