"""GPU tests of the piecewise-linear warp fit: the ``pl`` kernels of csrc/warp_fit.hip through
ava_amd.warp_fit against the numpy restatement of tests/warppl_cases.py (pinned by tests/test_cpu_warppl.py), and the
dataset wiring ``fit='device'`` with ``n_knots``.

Tolerances (u = 2^-52 for float64 inputs, 2^-23 for float32 inputs, whose outputs are float32):
  pl_warp_loss    relative 4 F T 2^-52, the order of an F T-term sum: positions, taps and every term are the oracle's
                  operation for operation, only the order of the sum differs; two runs bit-identical
  apply_warp      |dev - ref| <= 8 u max|spec|: three rounded operations on operands bounded by 2 max|spec|
  align_specs     against the planted knots and the numpy search, see the test
"""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import warpfit_cases as FC
import warppl_cases as PC
from ava_amd import synthetic as syn

pytestmark = pytest.mark.gpu

U = {'float64': 2.0 ** -52, 'float32': 2.0 ** -23}
EINVAL = -1


@pytest.fixture(scope="module")
def wf():
    from ava_amd import warp_fit
    return warp_fit


def _lib_and_stream():
    from ava_amd import _lib
    return _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hashed_knots(N, C, T, K, salt):
    """[N, C, K] knots in order: every knot within 0.3 segments of its template column, the whole warp shifted by up to
    0.3 T, so that positions leave the grid at both ends"""
    seg = (T - 1) / (K - 1)
    move = (2 * syn.u01(N * C * K, salt).reshape(N, C, K) - 1) * 0.3 * seg
    shift = (2 * syn.u01(N * C, salt + 1).reshape(N, C, 1) - 1) * 0.3 * T
    return PC.knot_columns(T, K) + move + shift


@pytest.mark.parametrize("shape", [(3, 9, 200, 19, 4), (2, 5, 512, 9, 16), (5, 2, 37, 1, 3)])
@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_pl_loss_against_the_numpy_objective(shape, dtype, wf):
    """T - 1 not divisible by K - 1 (200 / 4, 512 / 16), columns exactly on a knot (37 / 3), F over the 4 staged rows, C
    over and off the 8 candidates of a workgroup, T and K at their caps"""
    N, F, T, C, K = shape
    specs = syn.u01(N * F * T, 4301).reshape(N, F, T).astype(dtype)
    target = syn.u01(F * T, 4302).reshape(F, T)
    cands = _hashed_knots(N, C, T, K, 4303)
    bound = 4 * F * T * 2.0 ** -52
    for shift_λ, slope_λ in [(0.01, 0.5), (0.0, np.inf)]:
        want = np.stack([PC.objective(specs[n], target, cands[n], shift_λ, slope_λ) for n in range(N)])
        assert np.isfinite(want).all()
        got = wf.pl_warp_loss(torch.from_numpy(specs).cuda(), target, cands, shift_λ, slope_λ)
        again = wf.pl_warp_loss(torch.from_numpy(specs).cuda(), target, cands, shift_λ, slope_λ)
        assert torch.is_tensor(got) and got.dtype == torch.float64 and tuple(got.shape) == (N, C)
        rel = float(np.abs(got.cpu().numpy() / want - 1).max())
        print("%s %s λ=(%g, %g): max rel err %.3e (bound %.3e)" % (shape, dtype, shift_λ, slope_λ, rel, bound))
        assert rel <= bound
        assert torch.equal(got.view(torch.int64), again.view(torch.int64))


@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_two_knots_through_the_pl_kernel_are_the_shift_and_slope_loss(dtype, wf):
    N, F, T, C = 3, 9, 200, 19
    specs = syn.u01(N * F * T, 4311).reshape(N, F, T).astype(dtype)
    target = syn.u01(F * T, 4312).reshape(F, T)
    u = syn.u01(N * C * 2, 4313).reshape(N, C, 2)
    x = np.stack([(2 * u[..., 0] - 1) * 0.3 * T, (2 * u[..., 1] - 1) * 0.3], axis=-1)          # (shift, log slope)
    knots = np.stack([x[..., 0], x[..., 0] + np.exp(x[..., 1]) * (T - 1)], axis=-1)
    bound = 4 * F * T * 2.0 ** -52
    for shift_λ, slope_λ in [(0.01, 0.5), (0.0, 0.0), (0.01, np.inf)]:
        want = wf.warp_loss(specs, target, x, shift_λ, slope_λ)
        got = wf.pl_warp_loss(specs, target, knots, shift_λ, slope_λ)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape
        rel = float(np.abs(got / want - 1).max())
        print("%s λ=(%g, %g): pl / f12 - 1 = %.3e (bound %.3e)" % (dtype, shift_λ, slope_λ, rel, bound))
        assert rel <= bound
        if slope_λ == np.inf:                                # positions u_0 + j in both kernels: the same bits
            assert np.array_equal(got, want)


def test_crossed_knots_cost_infinity_and_never_win(wf):
    N, F, T, K = 2, 3, 41, 4
    specs = syn.u01(N * F * T, 4321).reshape(N, F, T)
    target = syn.u01(F * T, 4322).reshape(F, T)
    t = PC.knot_columns(T, K)
    cands = np.tile(t, (N, 10, 1)) + 0.1 * np.arange(10)[None, :, None]
    cands[:, 0, 1] = cands[:, 0, 2] + 1.0                    # candidate 0: knots 1 and 2 crossed
    cands[:, 5, 3] = cands[:, 5, 2]                          # candidate 5: a segment of slope 0
    cands[1, 9, 0] = cands[1, 9, 1] + 7.0                    # candidate 9 of motif 1: knots 0 and 1 crossed
    for slope_λ in (0.0, 0.5):
        loss = wf.pl_warp_loss(specs, target, cands, 0.01, slope_λ)
        want = np.stack([PC.objective(specs[n], target, cands[n], 0.01, slope_λ) for n in range(N)])
        assert np.array_equal(np.isposinf(loss), np.isposinf(want))
        assert np.isposinf(loss[:, 0]).all() and np.isposinf(loss[:, 5]).all() and np.isposinf(loss[1, 9])
        assert np.isfinite(loss[0, 9]) and np.isfinite(loss[:, 1:5]).all()
        # the kernels in a row, as the search chains them: the crossed centre loses to the finite candidates
        lib, st = _lib_and_stream()
        d_loss, d_cand = torch.from_numpy(loss).cuda(), torch.from_numpy(cands).cuda()
        best = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        u = torch.zeros((N, K), dtype=torch.float64, device="cuda")
        bl = torch.zeros(N, dtype=torch.float64, device="cuda")
        assert lib.ava_warpfit_pl_argmin(d_loss.data_ptr(), d_cand.data_ptr(), N, 10, K, best.data_ptr(), u.data_ptr(),
                                         bl.data_ptr(), st) == 0
        finite = np.where(np.isfinite(loss), loss, np.inf)
        assert best.tolist() == finite.argmin(axis=1).tolist() and 0 not in best.tolist()
        assert np.array_equal(u.cpu().numpy(), cands[np.arange(N), finite.argmin(axis=1)])
        assert np.array_equal(bl.cpu().numpy(), finite.min(axis=1))
    assert np.isfinite(wf.pl_warp_loss(specs, target, cands, 0.01, np.inf)).all()              # slope 1 whatever the knots


def test_pl_candidates_layout_and_argmin_rules_at_stride_k():
    lib, st = _lib_and_stream()
    N, K, ks, h = 3, 5, 3, 0.375
    C = 2 * ks + 1
    u = torch.tensor([[0.0, 10.0, 20.0, 30.0, 40.0], [-1.5, 9.0, 21.0, 30.5, 42.0], [2.0, 12.0, 22.0, 32.0, 42.0]],
                     dtype=torch.float64, device="cuda")
    off = np.array([0, -1, 1, -2, 2, -3, 3], dtype=np.float64)
    for axis in (-1, 0, 2, K - 1):
        cand = torch.full((N, C, K), -123.0, dtype=torch.float64, device="cuda")
        assert lib.ava_warpfit_pl_candidates(u.data_ptr(), N, K, axis, ks, h, cand.data_ptr(), st) == 0
        want = np.tile(u.cpu().numpy()[:, None, :], (1, C, 1))
        if axis < 0:
            want += (off * h)[None, :, None]
        else:
            want[:, :, axis] += off * h
        assert np.array_equal(cand.cpu().numpy(), want), axis                                 # candidate 0 is the centre
    # argmin over candidates of K parameters: ties to the lowest index, NaN never wins, +inf loses to any finite loss
    nan, inf = float('nan'), float('inf')
    loss = torch.full((5, 70), 5.0, dtype=torch.float64, device="cuda")
    loss[0, 69] = 1.0
    loss[0, 3] = 1.0
    loss[1, :] = nan
    loss[1, 66] = 7.0
    loss[2, :] = nan
    loss[3, 0] = inf
    loss[4, :] = nan
    loss[4, 65] = inf
    cand = torch.arange(5 * 70 * K, dtype=torch.float64, device="cuda").reshape(5, 70, K)
    best = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    uo = torch.full((5, K), -1.0, dtype=torch.float64, device="cuda")
    lo = torch.zeros(5, dtype=torch.float64, device="cuda")
    assert lib.ava_warpfit_pl_argmin(loss.data_ptr(), cand.data_ptr(), 5, 70, K, best.data_ptr(), uo.data_ptr(), lo.data_ptr(),
                                     st) == 0
    assert best.tolist() == [3, 66, 0, 1, 65]
    assert torch.equal(uo, cand[torch.arange(5), best.long()])
    assert lo[:2].tolist() == [1.0, 7.0] and bool(torch.isnan(lo[2])) and float(lo[3]) == 5.0 and float(lo[4]) == inf


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("name,K", [('spec_T130', 4), ('spec_T37', 16), ('amp_T37', 3)])
def test_apply_warp_with_knots_against_numpy(name, K, dtype, wf):
    specs = FC.specs(name, dtype)
    N, F, T = specs.shape
    knots = _hashed_knots(N, 1, T, K, 4331)[:, 0, :]
    knots[0] = PC.knot_columns(T, K)                         # the identity: whole positions, weight 1 on column j
    knots[1] = PC.knot_columns(T, K) * 0.9 - 3.5             # below the first column for j < 4
    knots[2] = PC.knot_columns(T, K) * 1.1 + 5.25            # above the last column at the end
    want = PC.apply_warp(specs, knots)
    got = wf.apply_warp(specs, {'knots': knots})
    assert isinstance(got, np.ndarray) and got.dtype == specs.dtype and got.shape == want.shape
    err, bound = float(np.abs(got.astype(np.float64) - want).max()), 8 * U[dtype] * float(np.abs(specs).max())
    print("%s K=%d %s: max abs err %.3e (bound %.3e)" % (name, K, dtype, err, bound))
    assert err <= bound
    assert np.array_equal(got[1, :, :3], np.repeat(specs[1, :, :1], 3, axis=1))
    assert np.array_equal(got[2, :, -3:], np.repeat(specs[2, :, -1:], 3, axis=1))
    dev = wf.apply_warp(torch.from_numpy(specs).cuda(), {'knots': torch.from_numpy(knots).cuda()})
    assert torch.is_tensor(dev) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)


@pytest.fixture(scope="module")
def planted():
    """the planted motifs, their knots and the numpy search's result, computed once"""
    specs = PC.planted_specs()
    warped, knots = PC.align_specs(specs, PC.SHIFT_LAMBDAS, PC.SLOPE_LAMBDAS, PC.PLANTED['n_knots'])
    return specs, PC.planted_knots(), FC.spread(warped), knots


def test_align_specs_recovers_planted_knots(planted, wf, capsys):
    """N = 6, F = 3, T = 97, 4 knots planted within 3 bins of the template's.
    (a) spread <= 0.1 x the spread of the shift-and-slope fit; (b) knots within 0.5 bins of the planted ones once the
    per-knot mean over motifs is removed; (c) spread <= 1.05 x the numpy search's; (d) apply_warp reproduces the warped
    spectrograms; (e) n_knots = 0 is the call without the keyword."""
    specs, planted_knots, ref_spread, ref_knots = planted
    n_knots = PC.PLANTED['n_knots']
    with pytest.warns(UserWarning, match="experimental"):
        warped, wp = wf.align_specs(specs, PC.SHIFT_LAMBDAS, PC.SLOPE_LAMBDAS, verbose=True, n_knots=n_knots)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Iteration ")]
    assert len(lines) == len(PC.SHIFT_LAMBDAS)
    with pytest.warns(UserWarning):
        w0, wp0 = wf.align_specs(specs, PC.SHIFT_LAMBDAS, PC.SLOPE_LAMBDAS, verbose=False, n_knots=0)
    with pytest.warns(UserWarning):
        w1, wp1 = wf.align_specs(specs, PC.SHIFT_LAMBDAS, PC.SLOPE_LAMBDAS, verbose=False)
    assert isinstance(warped, np.ndarray) and warped.dtype == specs.dtype and warped.shape == specs.shape
    assert sorted(wp) == ['knots', 'shifts', 'slopes'] and wp['knots'].shape == (len(specs), n_knots + 2)
    assert wp['shifts'].shape == wp['slopes'].shape == (len(specs),) and (np.diff(wp['knots'], axis=1) > 0).all()
    got, line = FC.spread(warped), FC.spread(w0)
    err = PC.knot_error(wp['knots'], planted_knots)
    print("spread: unaligned %.5g, n_knots=0 %.5g, n_knots=%d %.5g (ratio %.4f), numpy search %.5g (dev / ref = %.5f); knot "
          "error %.3f bins (numpy search %.3f); max |dev - numpy| knot %.2e"
          % (FC.spread(specs), line, n_knots, got, got / line, ref_spread, got / ref_spread, err,
             PC.knot_error(ref_knots, planted_knots), np.abs(wp['knots'] - ref_knots).max()))
    assert got <= 0.1 * line                                                                  # (a)
    assert err <= 0.5                                                                         # (b)
    assert got <= 1.05 * ref_spread                                                           # (c)
    assert np.array_equal(wf.apply_warp(specs, wp), warped)                                   # (d)
    assert sorted(wp0) == ['shifts', 'slopes'] and np.array_equal(w0, w1)                     # (e)
    assert np.array_equal(wp0['shifts'], wp1['shifts']) and np.array_equal(wp0['slopes'], wp1['slopes'])
    # device tensors and float32 in, the same kind out, and (d) again
    s32 = torch.from_numpy(specs.astype(np.float32)).cuda()
    with pytest.warns(UserWarning):
        w32, wp32 = wf.align_specs(s32, PC.SHIFT_LAMBDAS, PC.SLOPE_LAMBDAS, verbose=False, n_knots=n_knots)
    assert torch.is_tensor(w32) and w32.dtype == torch.float32 and wp32['knots'].is_cuda and wp32['knots'].dtype == torch.float64
    assert torch.equal(wf.apply_warp(s32, wp32), w32)
    assert PC.knot_error(wp32['knots'].cpu().numpy(), planted_knots) <= 0.5


def test_pl_minimize_warp_never_raises_the_loss(planted, wf):
    specs = planted[0]
    N, F, T = specs.shape
    target = specs.mean(axis=0)
    u0 = np.tile(PC.knot_columns(T, 4), (N, 1))
    for shift_λ, slope_λ in [(1e-3, 0.1), (0.0, 0.0)]:
        u, loss = wf.pl_minimize_warp(specs, target, u0, shift_λ, slope_λ)
        at_u0 = wf.pl_warp_loss(specs, target, u0[:, None, :], shift_λ, slope_λ)[:, 0]
        at_u = wf.pl_warp_loss(specs, target, u[:, None, :], shift_λ, slope_λ)[:, 0]
        ref = np.array([PC.stage_b(specs[n], target, u0[n], shift_λ, slope_λ)[1] for n in range(N)])
        print("λ=(%g, %g): loss / loss at u0 %s, dev / numpy - 1 %s" % (shift_λ, slope_λ, np.array2string(loss / at_u0, precision=3),
                                                                        np.array2string(loss / ref - 1, precision=2)))
        assert u.shape == (N, 4) and np.array_equal(at_u, loss) and np.all(loss <= at_u0) and (np.diff(u, axis=1) > 0).all()
    u, loss = wf.pl_minimize_warp(specs, target, u0 + [0.0, 1.0, -1.0, 0.5], 1e-2, np.inf)      # a common shift only
    x, _ = wf.minimize_warp(specs, target, np.zeros((N, 2)), 1e-2, np.inf)                  # the same line of shifts
    print("common shift %s, minimize_warp's %s" % (np.array2string(u[:, 0], precision=5), np.array2string(x[:, 0], precision=5)))
    assert np.array_equal(u, u[:, :1] + PC.knot_columns(T, 4))
    x[:, 0] = u[:, 0]
    assert np.array_equal(loss, wf.warp_loss(specs, target, x[:, None, :], 1e-2, np.inf)[:, 0])
    assert np.all(loss <= wf.pl_warp_loss(specs, target, u0[:, None, :], 1e-2, np.inf)[:, 0])


def test_python_errors_come_before_any_launch(wf):
    with pytest.raises(NotImplementedError):
        wf.apply_warp(np.zeros((1, 1, 513)), {'knots': [[0.0, 256.0, 512.0]]})
    with pytest.warns(UserWarning), pytest.raises(NotImplementedError):
        wf.align_specs(np.zeros((2, 1, 513)), [0.0], [0.0], verbose=False, n_knots=2)
    cap = wf._lib.load().ava_warpfit_max_knots()
    assert cap == 16
    with pytest.warns(UserWarning), pytest.raises(ValueError, match="knots"):
        wf.align_specs(np.zeros((2, 1, 100)), [0.0], [0.0], verbose=False, n_knots=cap - 1)    # K = 17
    with pytest.warns(UserWarning), pytest.raises(ValueError, match="time bins"):
        wf.align_specs(np.zeros((2, 1, 6)), [0.0], [0.0], verbose=False, n_knots=2)            # T - 1 = 5 < 6
    with pytest.warns(UserWarning), pytest.raises(ValueError):
        wf.align_specs(np.zeros((2, 1, 100)), [0.0], [0.0], verbose=False, n_knots=-1)
    with pytest.raises(ValueError):
        wf.apply_warp(np.zeros((2, 1, 8)), {'knots': np.zeros((3, 3))})
    with pytest.raises(ValueError):
        wf.apply_warp(np.zeros((2, 1, 8)), {'knots': np.zeros((2, 5))})                        # T - 1 = 7 < 8
    with pytest.raises(ValueError):
        wf.pl_warp_loss(np.zeros((2, 1, 40)), np.zeros((1, 40)), np.zeros((2, 3, 17)), 0.0, 0.0)
    with pytest.raises(ValueError):
        wf.pl_warp_loss(np.zeros((2, 1, 40)), np.zeros((1, 40)), np.zeros((2, 3, 4)), np.inf, 0.0)
    with pytest.raises(ValueError):
        wf.pl_minimize_warp(np.zeros((2, 1, 40)), np.zeros((1, 40)), np.zeros((2, 1)), 0.0, 0.0)


def test_c_abi_argument_checks_launch_nothing():
    lib, st = _lib_and_stream()
    N, F, T, C, K = 2, 3, 16, 5, 4
    spec = torch.ones((N, F, T), dtype=torch.float64, device="cuda")
    target = torch.ones((F, T), dtype=torch.float64, device="cuda")
    cand = torch.zeros((N, C, 16), dtype=torch.float64, device="cuda")
    knots = torch.zeros((N, 16), dtype=torch.float64, device="cuda")
    sentinel = -123.0
    out = torch.full((N, F, T), sentinel, dtype=torch.float64, device="cuda")
    loss = torch.full((N, C), sentinel, dtype=torch.float64, device="cuda")
    cand_out = torch.full((N, 63, 17), sentinel, dtype=torch.float64, device="cuda")
    best = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    u_out = torch.full((N, 17), sentinel, dtype=torch.float64, device="cuda")
    s, t, c, k, o, ls, co, b, uo = (v.data_ptr() for v in (spec, target, cand, knots, out, loss, cand_out, best, u_out))
    cap_t, cap_k = lib.ava_warpfit_max_t(), lib.ava_warpfit_max_knots()
    assert (cap_t, cap_k) == (512, 16)
    bad = [
        lib.ava_warpfit_pl_apply(None, 1, N, F, T, k, K, o, st),
        lib.ava_warpfit_pl_apply(s, 1, N, F, T, None, K, o, st),
        lib.ava_warpfit_pl_apply(s, 1, N, F, T, k, K, None, st),
        lib.ava_warpfit_pl_apply(s, 2, N, F, T, k, K, o, st),
        lib.ava_warpfit_pl_apply(s, 1, 0, F, T, k, K, o, st),
        lib.ava_warpfit_pl_apply(s, 1, N, F, cap_t + 1, k, K, o, st),
        lib.ava_warpfit_pl_apply(s, 1, N, F, T, k, 1, o, st),
        lib.ava_warpfit_pl_apply(s, 1, N, F, T, k, cap_k + 1, o, st),
        lib.ava_warpfit_pl_apply(s, 1, N, F, T, k, 9, o, st),                                  # T - 1 = 15 < 2 * 8
        lib.ava_warpfit_pl_candidates(None, N, K, 0, 3, 1.0, co, st),
        lib.ava_warpfit_pl_candidates(k, N, K, 0, 3, 1.0, None, st),
        lib.ava_warpfit_pl_candidates(k, 0, K, 0, 3, 1.0, co, st),
        lib.ava_warpfit_pl_candidates(k, N, 1, 0, 3, 1.0, co, st),
        lib.ava_warpfit_pl_candidates(k, N, cap_k + 1, 0, 3, 1.0, co, st),
        lib.ava_warpfit_pl_candidates(k, N, K, K, 3, 1.0, co, st),
        lib.ava_warpfit_pl_candidates(k, N, K, -2, 3, 1.0, co, st),
        lib.ava_warpfit_pl_candidates(k, N, K, 0, -1, 1.0, co, st),
        lib.ava_warpfit_pl_candidates(k, N, K, 0, 32, 1.0, co, st),
        lib.ava_warpfit_pl_candidates(k, N, K, 0, 3, float('nan'), co, st),
        lib.ava_warpfit_pl_loss(None, 1, N, F, T, t, c, C, K, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, None, c, C, K, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, None, C, K, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, c, C, K, 0.0, 0.0, None, st),
        lib.ava_warpfit_pl_loss(s, 3, N, F, T, t, c, C, K, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, 0, T, t, c, C, K, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, cap_t + 1, t, c, C, K, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, c, 0, K, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, c, 4097, K, 0.0, 0.0, ls, st),                 # C above WF_MAX_C
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, c, C, 1, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, c, C, cap_k + 1, 0.0, 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, c, C, 9, 0.0, 0.0, ls, st),                    # T - 1 = 15 < 2 * 8
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, c, C, K, float('nan'), 0.0, ls, st),
        lib.ava_warpfit_pl_loss(s, 1, N, F, T, t, c, C, K, 0.0, float('nan'), ls, st),
        lib.ava_warpfit_pl_argmin(None, c, N, C, K, b, uo, None, st),
        lib.ava_warpfit_pl_argmin(ls, c, N, C, K, None, uo, None, st),
        lib.ava_warpfit_pl_argmin(ls, None, N, C, K, b, uo, None, st),
        lib.ava_warpfit_pl_argmin(ls, c, 0, C, K, b, uo, None, st),
        lib.ava_warpfit_pl_argmin(ls, c, N, 0, K, b, uo, None, st),
        lib.ava_warpfit_pl_argmin(ls, c, N, 4097, K, b, uo, None, st),
        lib.ava_warpfit_pl_argmin(ls, c, N, C, 1, b, uo, None, st),
        lib.ava_warpfit_pl_argmin(ls, c, N, C, cap_k + 1, b, uo, None, st),
    ]
    assert bad == [EINVAL] * len(bad)
    torch.cuda.synchronize()
    for buf in (out, loss, cand_out, u_out):
        assert bool((buf == sentinel).all())
    assert best.tolist() == [-7] * N


# ---- the dataset with fit='device' and n_knots -------------------------------------------------------------------------

GAPS = [0, 3, 1, 5, 2]             # whole frame steps between the two halves of the motif


def _split_motif_files(tmp):
    """five files holding the same motif, its second half delayed by GAPS frame steps, in a little noise of their own"""
    p = dict(syn.FINCH_PARAMS)
    fs, step = p['fs'], p['nperseg'] - p['noverlap']
    ex, _, _ = syn.songs(n_exemplars=1, n_songs=0, fs=fs, motif_seconds=0.4, salt=8101)
    motif = ex[0].astype(np.float64)
    half = len(motif) // 2 // step * step
    n = len(motif) + (max(GAPS) + 3) * step
    fns = []
    for i, g in enumerate(GAPS):
        x = 30.0 * syn.gauss(n, 8300 + i)
        x[step:step + half] += motif[:half]
        start = step + half + g * step
        x[start:start + len(motif) - half] += motif[half:]
        fns.append(os.path.join(str(tmp), "motif_%02d.wav" % i))
        wavfile.write(fns[-1], fs, np.clip(np.rint(x), -32768, 32767).astype(np.int16))
    return fns, p, step


def _whole_msd(ds):
    whole = np.stack([ds.get_whole_warped_spectrogram(fn, time_bins=128) for fn in ds.audio_filenames])
    return float(((whole - whole.mean(axis=0)) ** 2).mean())


def test_dataset_fit_device_with_inner_knots(tmp_path):
    """fails on a fit that ignores ``n_knots`` (knots of shape [files, 2])"""
    from ava_amd import warped_window as ww
    fns, p, step = _split_motif_files(tmp_path)
    warp_fn = os.path.join(str(tmp_path), "warp.npy")
    with pytest.warns(UserWarning, match="experimental"):
        ds = ww.DeviceWarpedWindowDataset(fns, p, warp_fn=warp_fn, warp_type='spectrogram', fit='device',
                                          warp_params={'n_knots': 2})
    n = len(fns)
    T = int(round(ds.template_dur * p['fs'] / step))                 # time bins of the fit inputs
    assert ds.x_knots.shape == ds.y_knots.shape == (n, 4)
    assert np.array_equal(ds.y_knots, np.tile(PC.knot_columns(T, 4) / T, (n, 1)))
    assert (np.diff(ds.x_knots, axis=1) > 0).all()
    with pytest.warns(UserWarning, match="experimental"):
        line = ww.DeviceWarpedWindowDataset(fns, p, save_warp=False, warp_type='spectrogram', fit='device',
                                            warp_params={'n_knots': 0})
    assert line.x_knots.shape == (n, 2)
    msd_pl, msd_line = _whole_msd(ds), _whole_msd(line)
    print("mean squared difference between the files' whole warped spectrograms: 4 knots %.5g, 2 knots %.5g; x_knots * T - t:\n%s"
          % (msd_pl, msd_line, np.round(ds.x_knots * T - PC.knot_columns(T, 4), 2)))
    assert msd_pl < msd_line
    saved = np.load(warp_fn, allow_pickle=True).item()
    assert sorted(saved) == sorted(['x_knots', 'y_knots', 'template_dur', 'audio_filenames', 'amplitude_traces', 'warp_params'])
    assert saved['warp_params']['n_knots'] == 2 and saved['x_knots'].shape == (n, 4)
    again = ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=warp_fn)
    assert np.array_equal(again.x_knots, ds.x_knots) and np.array_equal(again.y_knots, ds.y_knots)
    assert again.template_dur == ds.template_dur
    assert torch.equal(again.__getitem__(list(range(8)), seed=3), ds.__getitem__(list(range(8)), seed=3))
