"""GPU tests of the warp-fit row: the kernels of csrc/warp_fit.hip through ava_amd.warp_fit
against tests/golden/warpfit.npz, which tests/golden/make_golden_warpfit.py wrote from the reference's
ava/preprocessing/warping.py, and the dataset wiring ``fit='device'``.

Tolerances (u = 2^-52 for float64 inputs, 2^-23 for float32 inputs, whose outputs are float32):
  apply_warp      |dev - ref| <= 8 u max|spec|: three rounded operations on operands bounded by 2 max|spec|
  warp_loss       relative 4 F T 2^-52 (the order of an F T-term sum); two runs bit-identical
  minimize_warp   dev_loss <= ref_loss (1 + 1e-4), 1e-4 being Powell's own ftol; every motif of every case
  align_specs     spread_dev <= spread_ref (1 + m), m measured by the golden script (twice the relative difference
                  to a run with Powell's tolerances at 1e-8, at least 1e-3) and stored with the golden
"""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import warpfit_cases as FC
from ava_amd import synthetic as syn

pytestmark = pytest.mark.gpu

U = {'float64': 2.0 ** -52, 'float32': 2.0 ** -23}


@pytest.fixture(scope="module")
def G():
    return FC.load()


@pytest.fixture(scope="module")
def wf():
    from ava_amd import warp_fit
    return warp_fit


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_apply_warp_against_the_reference(name, dtype, G, wf):
    specs = FC.specs(name, dtype)
    shifts, slopes = FC.apply_params(specs.shape[2])
    want = G["%s.%s.apply" % (name, dtype)]
    got = wf.apply_warp(specs, {'shifts': shifts, 'slopes': slopes})
    assert isinstance(got, np.ndarray) and got.dtype == specs.dtype and got.shape == want.shape
    err, bound = float(np.abs(got.astype(np.float64) - want).max()), 8 * U[dtype] * float(np.abs(specs).max())
    print("%s %s: max abs err %.3e (bound %.3e)" % (name, dtype, err, bound))
    assert err <= bound
    # the same through device tensors, and the held ends: positions off the grid give the end columns exactly
    dev = wf.apply_warp(torch.from_numpy(specs).cuda(), {'shifts': torch.from_numpy(shifts).cuda(), 'slopes': slopes})
    assert torch.is_tensor(dev) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    assert np.array_equal(got[1, :, :3], np.repeat(specs[1, :, :1], 3, axis=1))          # -3.5 + 0.9 j < 0 for j < 4
    assert np.array_equal(got[2, :, -3:], np.repeat(specs[2, :, -1:], 3, axis=1))        # 5.25 + 1.1 j > T - 1 at the end


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_warp_loss_against_the_reference_objectives(name, G, wf):
    r = FC.RECIPES[name]
    specs, pts, target = FC.specs(name), FC.loss_points(name), G[name + '.float64.target']
    bound = 4 * r['F'] * r['T'] * 2.0 ** -52
    for shift_λ, slope_λ in FC.LOSS_LAMBDAS:
        want = G["%s.float64.loss.%s" % (name, FC.lam_key(shift_λ, slope_λ))]
        got = wf.warp_loss(specs, target, pts, shift_λ, slope_λ)
        again = wf.warp_loss(specs, target, pts, shift_λ, slope_λ)
        assert got.dtype == np.float64 and got.shape == want.shape
        rel = float(np.abs(got / want - 1).max())
        print("%s λ=(%g, %g): max rel err %.3e (bound %.3e)" % (name, shift_λ, slope_λ, rel, bound))
        assert rel <= bound
        assert np.array_equal(got.view(np.int64), again.view(np.int64))


@pytest.mark.parametrize("shape", [(3, 9, 200, 19), (2, 5, 512, 9), (70, 2, 64, 1)])
@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_warp_loss_at_shapes_with_several_row_passes_and_candidate_blocks(shape, dtype, wf):
    """F over the 4 staged rows, C over and off the 8 candidates of a workgroup, T at the cap: against the numpy
    objective of the cases module (pinned to the reference by tests/test_cpu_warpfit.py), same bound"""
    N, F, T, C = shape
    specs = syn.u01(N * F * T, 3301).reshape(N, F, T).astype(dtype)
    target = syn.u01(F * T, 3302).reshape(F, T)
    u = syn.u01(N * C * 2, 3303).reshape(N, C, 2)
    cands = np.stack([(2 * u[..., 0] - 1) * 0.6 * T, (2 * u[..., 1] - 1) * 0.3], axis=-1)
    bound = 4 * F * T * 2.0 ** -52
    for shift_λ, slope_λ in [(0.01, 0.5), (0.0, np.inf)]:
        want = np.stack([FC.objective(specs[n], target, cands[n], shift_λ, slope_λ) for n in range(N)])
        got = wf.warp_loss(torch.from_numpy(specs).cuda(), target, cands, shift_λ, slope_λ)
        assert torch.is_tensor(got) and got.dtype == torch.float64
        rel = float(np.abs(got.cpu().numpy() / want - 1).max())
        print("%s %s λ=(%g, %g): max rel err %.3e (bound %.3e)" % (shape, dtype, shift_λ, slope_λ, rel, bound))
        assert rel <= bound


def test_kernel_bits_are_the_recorded_ones():
    """The loss, apply and grouped-mean entry points against tests/golden/warpfit_bits.npz, recorded on the device before
    the loss bodies, kernels and launch paths of the two warp forms were folded into one of each: an equality of bit
    patterns.  The grouped-equals-plain tests compare two outputs of one body and would move together with it."""
    from conftest import load_golden
    want, got = load_golden("warpfit_bits.npz"), FC.bits_record()
    assert sorted(got) == sorted(want)
    inf = int(np.array([np.inf]).view(np.int64)[0])
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype == np.int64 and got[key].shape == want[key].shape, key
        differ = int((got[key] != want[key]).sum())
        assert differ == 0, "%s: %d of %d bit patterns differ" % (key, differ, want[key].size)
        if key.endswith("pl_loss.finite"):                                                # the crossed candidate
            assert want[key][0, 1] == inf and int((want[key] == inf).sum()) == 1, key
        elif "loss" in key:
            assert not (want[key] == inf).any(), key


def _lib_and_stream():
    from ava_amd import _lib
    return _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_candidates_layout_and_argmin_rules():
    lib, st = _lib_and_stream()
    N, T, ks, kl, hs, hl = 3, 41, 3, 2, 0.5, 0.125
    C = (2 * ks + 1) * (2 * kl + 1)
    x = torch.tensor([[0.0, 0.0], [1.5, -0.1], [-2.0, 0.2]], dtype=torch.float64, device="cuda")
    cand = torch.empty((N, C, 2), dtype=torch.float64, device="cuda")
    assert lib.ava_warpfit_candidates(x.data_ptr(), N, T, ks, kl, hs, hl, cand.data_ptr(), st) == 0
    got, xs = cand.cpu().numpy(), x.cpu().numpy()
    off = lambda i: -((i + 1) // 2) if i % 2 else i // 2                                  # noqa: E731
    for n in range(N):
        assert np.array_equal(got[n, 0], xs[n])                                           # the centre comes first
        for c in range(C):
            oa, ob = off(c // (2 * kl + 1)), off(c % (2 * kl + 1))
            ls = xs[n, 1] + ob * hl
            shift = xs[n, 0] + oa * hs - (np.exp(ls) - np.exp(xs[n, 1])) * 0.5 * (T - 1)
            assert abs(got[n, c, 1] - ls) <= 1e-15 and abs(got[n, c, 0] - shift) <= 1e-13, (n, c)
    # argmin: ties go to the lowest index, NaN never wins, all NaN gives candidate 0
    nan = float('nan')
    loss = torch.full((4, 70), 5.0, dtype=torch.float64, device="cuda")
    loss[0, 69] = 1.0
    loss[0, 3] = 1.0
    loss[1, :] = nan
    loss[1, 66] = 7.0
    loss[2, :] = nan
    loss[3, 0] = nan
    cand = torch.arange(4 * 70 * 2, dtype=torch.float64, device="cuda").reshape(4, 70, 2)
    best = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    xo = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    lo = torch.zeros(4, dtype=torch.float64, device="cuda")
    assert lib.ava_warpfit_argmin(loss.data_ptr(), cand.data_ptr(), 4, 70, best.data_ptr(), xo.data_ptr(), lo.data_ptr(), st) == 0
    assert best.tolist() == [3, 66, 0, 1]
    assert torch.equal(xo, cand[torch.arange(4), best.long()])
    assert lo[:2].tolist() == [1.0, 7.0] and bool(torch.isnan(lo[2])) and float(lo[3]) == 5.0


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_minimize_warp_against_powell(name, G, wf):
    r = FC.RECIPES[name]
    specs, target, x0 = FC.specs(name), G[name + '.float64.target'], FC.min_x0(name)
    for shift_λ, slope_λ in FC.MIN_LAMBDAS:
        ref = G["%s.float64.min_loss.%s" % (name, FC.lam_key(shift_λ, slope_λ))]
        x, loss = wf.minimize_warp(specs, target, x0, shift_λ, slope_λ)
        assert x.shape == (r['N'], 2) and loss.shape == ref.shape == (r['N'],)
        print("%s λ=(%g, %g): dev / ref - 1 = %s" % (name, shift_λ, slope_λ, np.array2string(loss / ref - 1, precision=2)))
        assert np.all(loss <= ref * (1 + 1e-4))                                           # no motif left out
        at_x = wf.warp_loss(specs, target, x[:, None, :], shift_λ, slope_λ)[:, 0]
        at_x0 = wf.warp_loss(specs, target, x0[:, None, :], shift_λ, slope_λ)[:, 0]
        assert np.array_equal(at_x, loss) and np.all(loss <= at_x0)
        if slope_λ == np.inf:
            assert np.array_equal(x[:, 1], x0[:, 1])


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_align_specs_end_to_end(name, dtype, G, wf, capsys):
    specs = FC.specs(name, dtype)
    before, ref, _ = G["%s.%s.align_spread" % (name, dtype)]
    m = float(G["%s.%s.align_margin" % (name, dtype)])
    with pytest.warns(UserWarning, match="experimental"):
        warped, wp = wf.align_specs(specs, FC.SHIFT_LAMBDAS, FC.SLOPE_LAMBDAS, verbose=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Iteration ")]
    assert len(lines) == len(FC.SHIFT_LAMBDAS) and lines[0].startswith("Iteration 0, loss=")
    assert isinstance(warped, np.ndarray) and warped.dtype == specs.dtype and warped.shape == specs.shape
    assert sorted(wp) == ['shifts', 'slopes'] and wp['shifts'].shape == wp['slopes'].shape == (len(specs),)
    got = FC.spread(warped)
    print("%s %s: spread %.6g -> device %.6g, reference %.6g (dev / ref - 1 = %.3e, m = %.1e)"
          % (name, dtype, before, got, ref, got / ref - 1, m))
    assert got <= ref * (1 + m)
    assert np.array_equal(wf.apply_warp(specs, wp), warped)          # the parameters reproduce the warped spectrograms
    # device tensors in, device tensors out, the same bits
    with pytest.warns(UserWarning):
        w2, wp2 = wf.align_specs(torch.from_numpy(specs).cuda(), FC.SHIFT_LAMBDAS, FC.SLOPE_LAMBDAS, verbose=False)
    assert torch.is_tensor(w2) and w2.dtype == torch.from_numpy(specs).dtype and np.array_equal(w2.cpu().numpy(), warped)
    assert np.array_equal(wp2['shifts'].cpu().numpy(), wp['shifts']) and np.array_equal(wp2['slopes'].cpu().numpy(), wp['slopes'])


def test_shape_and_dtype_errors(wf):
    with pytest.raises(NotImplementedError):
        wf.apply_warp(np.zeros((1, 1, 513)), {'shifts': [0.0], 'slopes': [1.0]})
    with pytest.raises(TypeError):
        wf.apply_warp(np.zeros((1, 1, 8), dtype=np.int16), {'shifts': [0.0], 'slopes': [1.0]})
    with pytest.raises(ValueError):
        wf.apply_warp(np.zeros((1, 8)), {'shifts': [0.0], 'slopes': [1.0]})
    with pytest.raises(ValueError):
        wf.apply_warp(np.zeros((2, 1, 8)), {'shifts': [0.0], 'slopes': [1.0]})
    with pytest.raises(ValueError):
        wf.warp_loss(np.zeros((2, 1, 8)), np.zeros((1, 8)), np.zeros((2, 3, 2)), np.inf, 1.0)


def test_c_abi_argument_checks_launch_nothing():
    lib, st = _lib_and_stream()
    EINVAL = -1
    N, F, T, C = 2, 3, 16, 5
    spec = torch.ones((N, F, T), dtype=torch.float64, device="cuda")
    target = torch.ones((F, T), dtype=torch.float64, device="cuda")
    cand = torch.zeros((N, C, 2), dtype=torch.float64, device="cuda")
    sentinel = -123.0
    out = torch.full((N, F, T), sentinel, dtype=torch.float64, device="cuda")
    loss = torch.full((N, C), sentinel, dtype=torch.float64, device="cuda")
    tgt_out = torch.full((F, T), sentinel, dtype=torch.float64, device="cuda")
    cand_out = torch.full((N, 15, 2), sentinel, dtype=torch.float64, device="cuda")
    best = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    x = torch.zeros((N, 2), dtype=torch.float64, device="cuda")
    s, t, c, o, ls, b = (v.data_ptr() for v in (spec, target, cand, out, loss, best))
    cap = lib.ava_warpfit_max_t()
    assert cap == 512
    bad = [
        lib.ava_warpfit_apply(None, 1, N, F, T, x.data_ptr(), o, st),
        lib.ava_warpfit_apply(s, 1, N, F, T, None, o, st),
        lib.ava_warpfit_apply(s, 1, N, F, T, x.data_ptr(), None, st),
        lib.ava_warpfit_apply(s, 2, N, F, T, x.data_ptr(), o, st),
        lib.ava_warpfit_apply(s, 1, 0, F, T, x.data_ptr(), o, st),
        lib.ava_warpfit_apply(s, 1, N, 0, T, x.data_ptr(), o, st),
        lib.ava_warpfit_apply(s, 1, N, F, 1, x.data_ptr(), o, st),
        lib.ava_warpfit_apply(s, 1, N, F, cap + 1, x.data_ptr(), o, st),
        lib.ava_warpfit_mean(None, 1, N, F, T, tgt_out.data_ptr(), st),
        lib.ava_warpfit_mean(s, 1, N, F, T, None, st),
        lib.ava_warpfit_mean(s, 1, 0, F, T, tgt_out.data_ptr(), st),
        lib.ava_warpfit_mean(s, 1, N, F, cap + 1, tgt_out.data_ptr(), st),
        lib.ava_warpfit_candidates(None, N, T, 7, 0, 1.0, 1.0, cand_out.data_ptr(), st),
        lib.ava_warpfit_candidates(x.data_ptr(), N, T, 7, 0, 1.0, 1.0, None, st),
        lib.ava_warpfit_candidates(x.data_ptr(), 0, T, 7, 0, 1.0, 1.0, cand_out.data_ptr(), st),
        lib.ava_warpfit_candidates(x.data_ptr(), N, T, -1, 0, 1.0, 1.0, cand_out.data_ptr(), st),
        lib.ava_warpfit_candidates(x.data_ptr(), N, T, 32, 0, 1.0, 1.0, cand_out.data_ptr(), st),
        lib.ava_warpfit_candidates(x.data_ptr(), N, T, 7, 0, float('nan'), 1.0, cand_out.data_ptr(), st),
        lib.ava_warpfit_candidates(x.data_ptr(), N, cap + 1, 7, 0, 1.0, 1.0, cand_out.data_ptr(), st),
        lib.ava_warpfit_loss(None, 1, N, F, T, t, c, C, 0.0, 0.0, ls, st),
        lib.ava_warpfit_loss(s, 1, N, F, T, None, c, C, 0.0, 0.0, ls, st),
        lib.ava_warpfit_loss(s, 1, N, F, T, t, None, C, 0.0, 0.0, ls, st),
        lib.ava_warpfit_loss(s, 1, N, F, T, t, c, C, 0.0, 0.0, None, st),
        lib.ava_warpfit_loss(s, 1, 0, F, T, t, c, C, 0.0, 0.0, ls, st),
        lib.ava_warpfit_loss(s, 1, N, F, T, t, c, 0, 0.0, 0.0, ls, st),
        lib.ava_warpfit_loss(s, 1, N, F, T, t, c, 4097, 0.0, 0.0, ls, st),
        lib.ava_warpfit_loss(s, 1, N, F, cap + 1, t, c, C, 0.0, 0.0, ls, st),
        lib.ava_warpfit_loss(s, 3, N, F, T, t, c, C, 0.0, 0.0, ls, st),
        lib.ava_warpfit_loss(s, 1, N, F, T, t, c, C, float('nan'), 0.0, ls, st),
        lib.ava_warpfit_argmin(None, c, N, C, b, x.data_ptr(), None, st),
        lib.ava_warpfit_argmin(ls, c, N, C, None, x.data_ptr(), None, st),
        lib.ava_warpfit_argmin(ls, None, N, C, b, x.data_ptr(), None, st),
        lib.ava_warpfit_argmin(ls, c, 0, C, b, x.data_ptr(), None, st),
        lib.ava_warpfit_argmin(ls, c, N, 0, b, x.data_ptr(), None, st),
    ]
    assert bad == [EINVAL] * len(bad)
    torch.cuda.synchronize()
    for buf in (out, loss, tgt_out, cand_out):
        assert bool((buf == sentinel).all())
    assert best.tolist() == [-7] * N and float(x.abs().sum()) == 0.0


# ---- the dataset with fit='device' -----------------------------------------------------------------------------------

DELAYS = [0, 3, 1, 5, 2]           # whole frame steps


def _delayed_motif_files(tmp):
    """five files holding the same motif, delayed by DELAYS frame steps, in a little noise of their own"""
    p = dict(syn.FINCH_PARAMS)
    fs, step = p['fs'], p['nperseg'] - p['noverlap']
    ex, _, _ = syn.songs(n_exemplars=1, n_songs=0, fs=fs, motif_seconds=0.4, salt=8101)
    motif = ex[0].astype(np.float64)
    n = len(motif) + (max(DELAYS) + 2) * step
    fns = []
    for i, d in enumerate(DELAYS):
        x = 30.0 * syn.gauss(n, 8200 + i)
        x[(d + 1) * step:(d + 1) * step + len(motif)] += motif
        fns.append(os.path.join(str(tmp), "motif_%02d.wav" % i))
        wavfile.write(fns[-1], fs, np.clip(np.rint(x), -32768, 32767).astype(np.int16))
    return fns, p, step


def _whole_msd(ds):
    whole = np.stack([ds.get_whole_warped_spectrogram(fn, time_bins=128) for fn in ds.audio_filenames])
    return float(((whole - whole.mean(axis=0)) ** 2).mean())


@pytest.mark.parametrize("warp_type", ["amplitude", "spectrogram"])
def test_dataset_fit_device(warp_type, tmp_path):
    from ava_amd import warped_window as ww
    fns, p, step = _delayed_motif_files(tmp_path)
    warp_fn = os.path.join(str(tmp_path), "warp.npy")
    with pytest.warns(UserWarning, match="experimental"):
        ds = ww.DeviceWarpedWindowDataset(fns, p, warp_fn=warp_fn, warp_type=warp_type, fit='device')
    n = len(fns)
    assert ds.x_knots.shape == ds.y_knots.shape == (n, 2)
    assert np.array_equal(ds.y_knots, np.tile([0.0, 1.0], (n, 1)))
    T = int(round(ds.template_dur * p['fs'] / step))                 # time bins of the fit inputs
    delays = np.array(DELAYS) * step / p['fs']
    got = ds.x_knots[:, 0] - ds.x_knots[0, 0]
    want = (delays - delays[0]) / ds.template_dur
    print("%s: x_knots[:, 0] differences %s, delays / template_dur %s, slopes %s"
          % (warp_type, np.round(got, 5), np.round(want, 5), np.round(ds.x_knots[:, 1] - ds.x_knots[:, 0], 5)))
    assert np.abs(got - want).max() <= 1.0 / T
    null = ww.DeviceWarpedWindowDataset(fns, p, warp_type='null', save_warp=False)
    msd_fit, msd_null = _whole_msd(ds), _whole_msd(null)
    print("%s: mean squared difference between the files' whole warped spectrograms: fit %.5g, null warp %.5g"
          % (warp_type, msd_fit, msd_null))
    assert msd_fit < msd_null
    saved = np.load(warp_fn, allow_pickle=True).item()
    assert sorted(saved) == sorted(['x_knots', 'y_knots', 'template_dur', 'audio_filenames', 'amplitude_traces', 'warp_params'])
    assert saved['amplitude_traces'].shape == (n, T, 1) and saved['audio_filenames'] == sorted(fns)
    again = ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=warp_fn)
    assert np.array_equal(again.x_knots, ds.x_knots) and again.template_dur == ds.template_dur
    assert torch.equal(again.__getitem__(list(range(8)), seed=3), ds.__getitem__(list(range(8)), seed=3))


def test_dataset_fit_device_schedule_from_warp_params(tmp_path):
    from ava_amd import warped_window as ww
    fns, p, _ = _delayed_motif_files(tmp_path)
    with pytest.raises(ValueError, match="one entry per iteration"):
        ww.DeviceWarpedWindowDataset(fns, p, save_warp=False, warp_type='amplitude', fit='device',
                                     warp_params={'shift_lambdas': [0.1, 0.1], 'slope_lambdas': [np.inf]})
    with pytest.warns(UserWarning, match="experimental"):
        ds = ww.DeviceWarpedWindowDataset(fns, p, save_warp=False, warp_type='amplitude', fit='device',
                                          warp_params={'shift_lambdas': [0.0, 0.0], 'slope_lambdas': [np.inf, np.inf]})
    assert np.abs(ds.x_knots[:, 1] - ds.x_knots[:, 0] - 1.0).max() <= 1e-12             # shift-only: every slope is 1
