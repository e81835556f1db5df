"""GPU tests of the grouped warp fits and the warp parameter searches.

Every kernel comparison is against the plain entry points of csrc/warp_fit.hip on the gathered tensor
``specs[rows][:, bins]`` -- tests/test_gpu_warpfit.py and tests/test_gpu_warppl.py pin those to numpy -- and is an equality
of bits, compared through ``view(torch.int64)``: the grouped loss stages a group's bins in list order exactly as the plain
kernel stages rows 0 .. F-1, and the grouped template sums a group's rows in rising order as ``ava_warpfit_mean`` does.

Only the ``raw`` loss has no plain counterpart.  It is compared with numpy's sum of squared differences to the relative
bound 4 F T 2^-52 the project uses for an F T-term sum whose terms are the oracle's operation for operation, and with itself
bit for bit.  ``cross_validate``'s scores inherit that bound through SS_tot; the test derives theirs."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import warpfit_cases as FC
import warppl_cases as PC
import warpsearch_cases as SC
from ava_amd import synthetic as syn

pytestmark = pytest.mark.gpu

EINVAL = -1
U = 2.0 ** -52


@pytest.fixture(scope="module")
def wf():
    from ava_amd import warp_fit
    return warp_fit


@pytest.fixture(scope="module")
def ws():
    from ava_amd import warp_search
    return warp_search


def _lib_and_stream():
    from ava_amd import _lib
    return _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _plain_mean(x):
    """``ava_warpfit_mean`` of the device tensor ``x`` [N, F, T]: [F, T] float64"""
    lib, st = _lib_and_stream()
    N, F, T = x.shape
    out = torch.empty((F, T), dtype=torch.float64, device="cuda")
    assert lib.ava_warpfit_mean(x.data_ptr(), 0 if x.dtype == torch.float32 else 1, N, F, T, out.data_ptr(), st) == 0
    return out


def _plan(wf, shape, groups, dtype, salt):
    """hashed specs, their plan with hashed targets, and per group its gathered tensor and target on the device"""
    N, F, T = shape['N'], shape['F'], shape['T']
    specs = syn.u01(N * F * T, salt).reshape(N, F, T).astype(dtype)
    plan = wf.GroupPlan(_dev(specs), wf.check_groups(groups, N, F))
    sizes = SC.group_sizes(groups, N, F)
    assert plan.V == sum(r for r, _ in sizes) and plan.max_bins == max(b for _, b in sizes)
    targets = [syn.u01(b * T, salt + 10 + g).reshape(b, T) for g, (_, b) in enumerate(sizes)]
    plan.targets.copy_(_dev(np.concatenate([t.reshape(-1) for t in targets])))
    gathered = [_dev(SC.gather(specs, r, b)) for r, b in groups]
    return specs, plan, gathered, [_dev(t) for t in targets]


def _check_group_losses(wf, shape, groups, shift_λs, slope_λs, dtype, form, salt):
    T, C, K = shape['T'], shape['C'], shape['K']
    specs, plan, gathered, targets = _plan(wf, shape, groups, dtype, salt)
    if form == 'pl':
        cand = _dev(SC.hashed_knots(plan.V, C, T, K, salt + 1))
    else:
        cand = _dev(SC.hashed_params(plan.V, C, T, salt + 1))
    d_shift = _dev(np.array(shift_λs, dtype=np.float64))
    for fixed in (False, True):
        slopes = [np.inf] * len(groups) if fixed else slope_λs
        got = torch.full((plan.V, C), -123.0, dtype=torch.float64, device="cuda")
        (plan.pl_loss if form == 'pl' else plan.ss_loss)(cand, d_shift, _dev(np.array(slopes, dtype=np.float64)), fixed, got)
        for g in range(len(groups)):
            lo, hi = int(plan.row_off[g]), int(plan.row_off[g + 1])
            plain = wf.pl_warp_loss if form == 'pl' else wf.warp_loss
            want = plain(gathered[g], targets[g], cand[lo:hi], shift_λs[g], slopes[g])
            assert bool(torch.isfinite(want).all())
            assert _bits_equal(got[lo:hi], want), (form, dtype, fixed, g)


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("form", ['ss', 'pl'])
def test_grouped_loss_has_the_plain_kernels_bits(form, dtype, wf):
    """N = 5, F = 9, T = 130, C = 19, K = 4; one row and one bin, a bin list that straddles a staging pass, everything; every
    group its own λ; and once with slope_λ = inf.  Fails on a kernel that masks bins instead of compacting them."""
    _check_group_losses(wf, SC.KERNEL_SHAPE, SC.KERNEL_GROUPS, SC.KERNEL_SHIFT_LAMBDAS, SC.KERNEL_SLOPE_LAMBDAS, dtype, form, 5101)


@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_grouped_loss_at_the_caps(dtype, wf):
    """T = 512 (82 KB of LDS, over the 64 KB that need no attribute), K = 16, F = 2"""
    for form in ('pl', 'ss'):
        _check_group_losses(wf, SC.CAP_SHAPE, SC.CAP_GROUPS, [0.01, 0.2], [0.5, 0.0], dtype, form, 5201)


@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_raw_loss_is_the_sum_of_squared_raw_differences(dtype, wf):
    shape, groups = SC.KERNEL_SHAPE, SC.KERNEL_GROUPS
    specs, plan, gathered, targets = _plan(wf, shape, groups, dtype, 5301)
    got = plan.raw_loss(torch.full((plan.V,), -123.0, dtype=torch.float64, device="cuda"))
    again = plan.raw_loss(torch.full((plan.V,), -123.0, dtype=torch.float64, device="cuda"))
    assert _bits_equal(got, again)
    got = got.cpu().numpy()
    for g, (rows, bins) in enumerate(groups):
        lo, hi = int(plan.row_off[g]), int(plan.row_off[g + 1])
        sub = SC.gather(specs, rows, bins).astype(np.float64)
        want = ((sub - targets[g].cpu().numpy()[None]) ** 2).sum(axis=(1, 2))
        rel, bound = float(np.abs(got[lo:hi] / want - 1).max()), 4 * sub.shape[1] * sub.shape[2] * U
        print("%s group %d: raw loss max rel err %.3e (bound %.3e)" % (dtype, g, rel, bound))
        assert rel <= bound
    # the pl entry point's raw switch is the same sum
    lib, st = _lib_and_stream()
    pl = torch.full((plan.V,), -123.0, dtype=torch.float64, device="cuda")
    s = plan.specs
    assert lib.ava_warpfit_group_pl_loss(s.data_ptr(), 0 if s.dtype == torch.float32 else 1, plan.N, plan.F, plan.T,
                                         plan.row_src.data_ptr(), plan.row_group.data_ptr(), plan.d_bin_off.data_ptr(),
                                         plan.bins.data_ptr(), plan.V, plan.targets.data_ptr(), None, 1, shape['K'], None, None,
                                         0, 1, pl.data_ptr(), st) == 0
    assert _bits_equal(pl, again)


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("case", ['kernel', 'mean'])
def test_grouped_template_is_the_mean_of_the_apply_kernels_output(case, dtype, wf):
    """both forms and raw, against ``ava_warpfit_mean`` of ``ava_warpfit_apply`` / ``ava_warpfit_pl_apply`` on the gathered
    tensor.  'mean': 37 rows (row sets of 16), 131 bins (past one sweep of the bin lanes), 70 columns (tiles of 64)."""
    shape, groups = (SC.KERNEL_SHAPE, SC.KERNEL_GROUPS) if case == 'kernel' else (SC.MEAN_SHAPE, SC.MEAN_GROUPS)
    T, K = shape['T'], shape['K']
    specs, plan, gathered, _ = _plan(wf, shape, groups, dtype, 5401)
    x = SC.hashed_params(plan.V, 1, T, 5402)[:, 0, :]
    params = _dev(np.stack([x[:, 0] * 0.2, np.exp(x[:, 1])], axis=1))                        # (shift, slope)
    knots = _dev(SC.hashed_knots(plan.V, 1, T, K, 5403)[:, 0, :] * 1.0)
    for form in ('ss', 'pl', 'raw'):
        out = torch.full_like(plan.targets, -123.0)
        plan.mean(params=params if form == 'ss' else None, knots=knots if form == 'pl' else None, out=out)
        for g in range(len(groups)):
            lo, hi = int(plan.row_off[g]), int(plan.row_off[g + 1])
            if form == 'ss':
                warped = wf.apply_warp(gathered[g], {'shifts': params[lo:hi, 0], 'slopes': params[lo:hi, 1]})
            elif form == 'pl':
                warped = wf.apply_warp(gathered[g], {'knots': knots[lo:hi]})
            else:
                warped = gathered[g]
            assert warped.dtype == gathered[g].dtype
            want = _plain_mean(warped.contiguous())
            a, b = int(plan.bin_off[g]) * T, int(plan.bin_off[g + 1]) * T
            assert _bits_equal(out[a:b].reshape(-1, T), want), (case, form, dtype, g)
        assert not bool((out == -123.0).any())


def test_c_abi_argument_checks_launch_nothing(wf):
    lib, st = _lib_and_stream()
    shape = SC.KERNEL_SHAPE
    specs, plan, _, _ = _plan(wf, shape, SC.KERNEL_GROUPS, 'float64', 5501)
    N, F, T, C, K, V, G = plan.N, plan.F, plan.T, shape['C'], shape['K'], plan.V, plan.G
    sentinel = -123.0
    loss = torch.full((V, C), sentinel, dtype=torch.float64, device="cuda")
    out = torch.full_like(plan.targets, sentinel)
    cand = torch.zeros((V, C, 16), dtype=torch.float64, device="cuda")
    lam = torch.zeros(G, dtype=torch.float64, device="cuda")
    s, rs, rg, ro, bo, bi, tg = (t.data_ptr() for t in (plan.specs, plan.row_src, plan.row_group, plan.d_row_off,
                                                        plan.d_bin_off, plan.bins, plan.targets))
    c, la, ls, o = cand.data_ptr(), lam.data_ptr(), loss.data_ptr(), out.data_ptr()
    gl, gpl, gm, gpm = (lib.ava_warpfit_group_loss, lib.ava_warpfit_group_pl_loss, lib.ava_warpfit_group_mean,
                        lib.ava_warpfit_group_pl_mean)
    bad = [
        gl(None, 1, N, F, T, rs, rg, bo, bi, V, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 2, N, F, T, rs, rg, bo, bi, V, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, 0, F, T, rs, rg, bo, bi, V, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, 513, rs, rg, bo, bi, V, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, None, rg, bo, bi, V, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, None, bo, bi, V, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, None, bi, V, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, None, V, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, 0, tg, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, None, c, C, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, None, C, la, la, 0, 0, ls, st),              # candidates unless raw
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, 0, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, 4097, la, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, C, None, la, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, C, la, None, 0, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, C, la, la, 2, 0, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, C, la, la, 0, 2, ls, st),
        gl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, C, la, la, 0, 0, None, st),
        gpl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, C, 1, la, la, 0, 0, ls, st),
        gpl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, c, C, 17, la, la, 0, 0, ls, st),
        gpl(s, 1, N, F, 16, rs, rg, bo, bi, V, tg, c, C, 9, la, la, 0, 0, ls, st),             # T - 1 = 15 < 2 * 8
        gpl(s, 1, N, F, T, rs, rg, bo, bi, V, tg, None, C, K, la, la, 0, 0, ls, st),
        gm(None, 1, N, F, T, rs, ro, bo, bi, G, F, c, 0, o, st),
        gm(s, 1, N, F, T, None, ro, bo, bi, G, F, c, 0, o, st),
        gm(s, 1, N, F, T, rs, None, bo, bi, G, F, c, 0, o, st),
        gm(s, 1, N, F, T, rs, ro, None, bi, G, F, c, 0, o, st),
        gm(s, 1, N, F, T, rs, ro, bo, None, G, F, c, 0, o, st),
        gm(s, 1, N, F, T, rs, ro, bo, bi, 0, F, c, 0, o, st),
        gm(s, 1, N, F, T, rs, ro, bo, bi, G, 0, c, 0, o, st),
        gm(s, 1, N, F, T, rs, ro, bo, bi, G, F, None, 0, o, st),                               # parameters unless raw
        gm(s, 1, N, F, T, rs, ro, bo, bi, G, F, c, 2, o, st),
        gm(s, 1, N, F, T, rs, ro, bo, bi, G, F, c, 0, None, st),
        gm(s, 3, N, F, T, rs, ro, bo, bi, G, F, c, 0, o, st),
        gpm(s, 1, N, F, T, rs, ro, bo, bi, G, F, c, 1, 0, o, st),
        gpm(s, 1, N, F, T, rs, ro, bo, bi, G, F, c, 17, 0, o, st),
        gpm(s, 1, N, F, T, rs, ro, bo, bi, G, F, None, K, 0, o, st),
        gpm(s, 1, N, F, T, rs, ro, bo, bi, G, F, c, K, -1, o, st),
    ]
    assert bad == [EINVAL] * len(bad)
    torch.cuda.synchronize()
    assert bool((loss == sentinel).all()) and bool((out == sentinel).all())


# ---- align_specs_grouped -------------------------------------------------------------------------------------------------

def _schedules():
    shift = np.array([SC.scaled(PC.SHIFT_LAMBDAS, a) for a, _ in SC.ALIGN_SCALES]).T
    slope = np.array([SC.scaled(PC.SLOPE_LAMBDAS, b) for _, b in SC.ALIGN_SCALES]).T
    return shift, slope


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("n_knots", [0, 2])
def test_align_specs_grouped_is_align_specs_on_the_gathered_inputs(n_knots, dtype, wf):
    """the planted motifs (N = 6, F = 3, T = 97) under the 7-iteration schedule, three groups with their own rows, bins and
    λ scales; ``max_rows`` = 6 runs the groups one by one, 10 cuts after the first, and neither changes a bit"""
    specs = PC.planted_specs(dtype=dtype)
    shift, slope = _schedules()
    got = wf.align_specs_grouped(specs, SC.ALIGN_GROUPS, shift, slope, n_knots=n_knots)
    keys = ['knots', 'shifts', 'slopes'] if n_knots else ['shifts', 'slopes']
    assert len(got) == len(SC.ALIGN_GROUPS)
    for g, (rows, bins) in enumerate(SC.ALIGN_GROUPS):
        with pytest.warns(UserWarning, match="experimental"):
            _, want = wf.align_specs(SC.gather(specs, rows, bins), list(shift[:, g]), list(slope[:, g]), verbose=False,
                                     n_knots=n_knots)
        assert sorted(got[g]) == sorted(want) == keys
        for key in keys:
            assert isinstance(got[g][key], np.ndarray) and got[g][key].dtype == np.float64
            assert got[g][key].shape == want[key].shape
            assert np.array_equal(got[g][key].view(np.int64), want[key].view(np.int64)), (n_knots, dtype, g, key)
        assert not np.array_equal(got[g]['shifts'], np.zeros_like(got[g]['shifts']))          # something was fitted
    for max_rows in (6, 10, 1):
        split = wf.align_specs_grouped(specs, SC.ALIGN_GROUPS, shift, slope, n_knots=n_knots, max_rows=max_rows)
        for a, b in zip(split, got):
            assert all(np.array_equal(a[key].view(np.int64), b[key].view(np.int64)) for key in keys)
    dev = wf.align_specs_grouped(torch.from_numpy(specs).cuda(), SC.ALIGN_GROUPS, shift, slope, n_knots=n_knots)
    assert all(torch.is_tensor(d[key]) and d[key].is_cuda and np.array_equal(d[key].cpu().numpy(), w[key])
               for d, w in zip(dev, got) for key in keys)


def test_bad_groups_and_schedules_raise_before_any_launch(wf, monkeypatch):
    specs = PC.planted_specs()
    shift, slope = _schedules()

    def no_launch(*a, **k):
        raise AssertionError("a plan was built for a call that has to fail first")
    monkeypatch.setattr(wf, "GroupPlan", no_launch)
    for bad in [[([], [0]), (None, None), (None, None)], [(None, []), (None, None), (None, None)],
                [([2, 1], None), (None, None), (None, None)], [([1, 1], None), (None, None), (None, None)],
                [(None, [0, 0]), (None, None), (None, None)], [([6], None), (None, None), (None, None)],
                [(None, [3]), (None, None), (None, None)], [([-1], None), (None, None), (None, None)],
                [(None, None), (None, None)], []]:
        with pytest.raises(ValueError):
            wf.align_specs_grouped(specs, bad, shift, slope)
    mixed = slope.copy()
    mixed[0, 1] = 1.0                                                                          # inf for two groups of three
    with pytest.raises(ValueError, match="every group or for none"):
        wf.align_specs_grouped(specs, SC.ALIGN_GROUPS, shift, mixed)
    with pytest.raises(ValueError, match="knots"):
        wf.align_specs_grouped(specs, SC.ALIGN_GROUPS, shift, slope, n_knots=15)
    with pytest.raises(ValueError):
        wf.align_specs_grouped(specs, SC.ALIGN_GROUPS, shift, slope, max_rows=0)
    with pytest.raises(NotImplementedError):
        wf.align_specs_grouped(np.zeros((2, 1, 513)), [(None, None)], [[0.0]], [[0.0]])


# ---- the searches ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_cross_validate_against_the_plain_public_functions(dtype, wf, ws):
    """N = 6, F = 10, T = 97, one sample per knot count -1, 0, 1, two splits each: every score against the one assembled
    from ``align_specs``, ``apply_warp`` and ``warp_loss`` / ``pl_warp_loss`` on gathered tensors with the same splits.

    SS_res is made of the same kernels' sums on the same bits and is added in the same order, so it is equal; SS_tot comes
    from the raw loss, whose per-row sums are within 4 F T 2^-52 (relative) of numpy's, and adding N of them on either side
    costs at most N 2^-52 each.  With r = SS_res / SS_tot that bounds |R² - R²_ref| by r (4 F T + 2 N) 2^-52, first order,
    plus the roundings of the division and the subtraction, 2 (1 + r) 2^-52; 1% is allowed for the higher orders."""
    specs = PC.planted_specs(SC.CV_RECIPE, dtype=dtype)
    N, F, T = specs.shape
    res = ws.cross_validate(specs, SC.CV_PARAMS, seed=SC.CV_SEED)
    knots, a, b, schedules, splits = ws.search_plan(F, SC.CV_PARAMS, SC.CV_SEED)
    assert sorted(res) == sorted(['knots', 'shift_scale', 'slope_scale', 'train_rsq', 'valid_rsq', 'test_rsq', 'schedules'])
    assert res['knots'].tolist() == [-1, 0, 1] and np.array_equal(res['shift_scale'], a) and np.array_equal(res['slope_scale'], b)
    assert res['train_rsq'].shape == res['valid_rsq'].shape == (3, 2) and res['test_rsq'].shape == (3,)
    assert res['schedules'] == schedules
    want = np.zeros((3, 3, 2))
    bound = np.zeros((3, 3, 2))
    for s in range(3):
        for v in range(2):
            with pytest.warns(UserWarning, match="experimental"):
                _, wp = wf.align_specs(SC.gather(specs, None, splits[s][v][0]), schedules[s][0], schedules[s][1],
                                       verbose=False, n_knots=max(int(knots[s]), 0))
            for i, bins in enumerate(splits[s][v]):
                sub = SC.gather(specs, None, bins)
                template = wf.apply_warp(sub, wp).astype(np.float64).mean(axis=0)
                if 'knots' in wp:
                    ss_res = wf.pl_warp_loss(sub, template, wp['knots'][:, None, :], 0.0, 0.0)[:, 0]
                else:
                    x = np.stack([wp['shifts'], np.log(wp['slopes'])], axis=1)
                    ss_res = wf.warp_loss(sub, template, x[:, None, :], 0.0, 0.0)[:, 0]
                sub = sub.astype(np.float64)
                bin_mean = sub.mean(axis=0).mean(axis=1)
                ss_tot = ((sub - bin_mean[None, :, None]) ** 2).sum(axis=(1, 2))
                r = ss_res.sum() / ss_tot.sum()
                want[i, s, v] = 1.0 - r
                bound[i, s, v] = 1.01 * (r * (4 * len(bins) * T + 2 * N) + 2 * (1 + r)) * U
    got = np.stack([res['train_rsq'], res['valid_rsq']])
    err = np.abs(got - want[:2])
    print("%s R² train\n%s\nvalid\n%s\ntest %s\nmax |dev - ref| / bound = %.3f" % (dtype, got[0], got[1], res['test_rsq'],
                                                                                   float((err / bound[:2]).max())))
    assert (err <= bound[:2]).all()
    assert (np.abs(res['test_rsq'] - want[2].mean(axis=1)) <= bound[2].max(axis=1) + 2 * U).all()
    assert (got[0] > 0).all() and (got[0] < 1).all()                                           # the fit explains its own bins
    again = ws.cross_validate(specs, SC.CV_PARAMS, seed=SC.CV_SEED, max_rows=7)
    for key in res:
        if key == 'schedules':
            assert again[key] == res[key]
        else:
            assert np.array_equal(again[key], res[key]), key
    best = ws.best_warp_params(res)
    assert sorted(best) == ['n_knots', 'shift_lambdas', 'slope_lambdas'] and best['n_knots'] in (0, 1)


def test_cross_validate_refuses_amplitude_traces(ws):
    amps = FC.specs('amp_T37')                                                                 # [6, 1, 37]
    with pytest.raises(ValueError, match="anchor_point_warp_parameter_search"):
        ws.cross_validate(amps)


OFFSETS = [0, 3, 6]                 # whole frame steps by which the motif starts later in each file
ANCHORS = [0.08, 0.17, 0.29]        # seconds after the motif's start


def _anchor_files(tmp):
    """three files of one duration holding the same motif at different delays, in a little noise of their own, each with
    its annotation: one row per anchor, onset and offset"""
    p = dict(syn.FINCH_PARAMS)
    fs, step = p['fs'], p['nperseg'] - p['noverlap']
    ex, _, _ = syn.songs(n_exemplars=1, n_songs=0, fs=fs, motif_seconds=0.4, salt=8701)
    motif = ex[0].astype(np.float64)
    n = len(motif) + (max(OFFSETS) + 4) * step
    for i, off in enumerate(OFFSETS):
        x = 30.0 * syn.gauss(n, 8800 + i)
        x[(off + 2) * step:(off + 2) * step + len(motif)] += motif
        wavfile.write(os.path.join(str(tmp), "motif_%02d.wav" % i), fs, np.clip(np.rint(x), -32768, 32767).astype(np.int16))
        onsets = np.array(ANCHORS) + (off + 2) * step / fs
        np.savetxt(os.path.join(str(tmp), "motif_%02d.txt" % i), np.stack([onsets, onsets + 0.01], axis=1))
    return p


def test_anchor_point_search_on_three_files(tmp_path, wf, ws, capsys):
    from ava_amd import warped_window as ww
    p = _anchor_files(tmp_path)
    search = dict(knot_range=(-1, 2), shift_range=(0.5, 2.0), slope_range=(0.1, 10.0),
                  shift_lambdas=[1e-2, 1e-3, 0.0], slope_lambdas=[np.inf, 1.0, 0.0])
    num_iter, gridpoints = 4, 3
    img = os.path.join(str(tmp_path), "anchor.pdf")
    np.random.seed(12)
    history, losses, support = ws.anchor_point_warp_parameter_search([], str(tmp_path), p, search, num_iter=num_iter,
                                                                     gridpoints=gridpoints, img_fn=img)
    out = capsys.readouterr().out
    # the shapes and dtypes of the reference's return
    assert history.shape == (num_iter, 3) and history.dtype == np.zeros(1, dtype='int').dtype
    assert losses.shape == (num_iter,) and losses.dtype == np.float64 and np.isfinite(losses).all()
    assert isinstance(support, list) and len(support) == 3
    assert np.array_equal(support[0], np.arange(-1, 2)) and np.array_equal(support[1], np.geomspace(0.5, 2.0, num=gridpoints))
    assert np.array_equal(support[2], np.geomspace(0.1, 10.0, num=gridpoints))
    # the draws, call for call
    np.random.seed(12)
    ranges = [np.arange(3), np.arange(gridpoints), np.arange(gridpoints)]
    draws = np.array([[np.random.choice(ranges[j]) for j in range(3)] for _ in range(num_iter)])
    assert np.array_equal(history, draws)
    # every loss from knots fitted through align_specs
    fns = sorted(os.path.join(str(tmp_path), f) for f in os.listdir(str(tmp_path)) if f.endswith('.wav'))
    audio = [wavfile.read(fn)[1] for fn in fns]
    _, amps, template_dur = ww.get_specs_and_amplitude_traces(audio, p['fs'], p)
    to_warp = np.ascontiguousarray(amps.transpose(0, 2, 1))
    anchors = np.array([np.loadtxt(fn[:-4] + '.txt').reshape(-1, 2)[:, 0] for fn in fns])
    for i in range(num_iter):
        k = int(support[0][history[i, 0]])
        shift = SC.scaled(search['shift_lambdas'], support[1][history[i, 1]])
        slope = [np.inf] * 3 if k < 0 else SC.scaled(search['slope_lambdas'], support[2][history[i, 2]])
        with pytest.warns(UserWarning, match="experimental"):
            _, wp = wf.align_specs(to_warp, shift, slope, verbose=False, n_knots=max(k, 0))
        x_knots, y_knots = wf.knots_from_warp_params(wp, to_warp.shape[2])
        assert losses[i] == ws.anchor_errors(x_knots, y_knots, anchors, template_dur), i
    null = 1e3 * np.mean(np.abs(anchors.mean(axis=0, keepdims=True) - anchors))
    print("null warp %.3f ms, losses %s ms" % (null, np.array2string(losses, precision=3)))
    assert "Null warp MAE: %.3f ms" % null in out and out.count(" ms\n") == num_iter + 1
    assert losses.min() < 0.5 * null                                                           # the fits do align the anchors
    assert os.path.getsize(img) > 0
