"""The spectrogram kernels (csrc/spec.hip, csrc/spec_core.h) at their own edges: the cases of tests/spec_cases.py, which
tests/test_cpu_spec_cases.py shows to reach those edges, against the oracle's get_spec with the rule of
tests/test_gpu_spec.py -- the device's fp32 output within one fp32 ulp (6e-8 on [0, 1]) of the oracle's fp64 values
anywhere, and at most 1e-3 of the pixels different from the oracle's values rounded to fp32.  The share of differing
pixels only means something on a large array: it is asserted where a case has at least 4096 pixels, the ulp bound alone on
the smaller ones (``_hold``).  Every test prints the two figures of its case."""
import functools

import numpy as np
import pytest
import torch

import spec_cases as SC
from test_gpu_spec import ULP, _check

pytestmark = pytest.mark.gpu

AVA_EINVAL = -1
SHARE_PIXELS = 4096


@functools.lru_cache(maxsize=None)
def _device_audio(name):
    from ava_amd import spec as sp
    return sp.DeviceAudio(list(SC.case(name)['audio']))


def _run(name, order=None, **kw):
    """get_spec_batch of the case's windows (``order``: which of them, in which order)"""
    from ava_amd import spec as sp
    c = SC.case(name)
    tt, tf = SC.device_targets(c)
    idx = np.arange(len(c['t1'])) if order is None else np.asarray(order)
    return sp.get_spec_batch(_device_audio(name), c['fidx'][idx], c['t1'][idx], c['t2'][idx], c['p'], c['fs'], tt[idx],
                             target_freqs=tf, fill_value=c['fill_value'], remove_dc_offset=c['remove_dc_offset'], **kw)


def _hold(name, dev, want):
    """the comparison rule; the share of differing pixels is asserted from SHARE_PIXELS pixels on"""
    got = dev.cpu().numpy()
    assert not np.isnan(got).any(), name
    err = np.abs(got.astype(np.float64) - want).max()
    share = (got != want.astype(np.float32)).mean()
    print("%s: %d pixels, max err / 6e-8 = %.3f, share of pixels off the rounded oracle = %.2e"
          % (name, want.size, err / ULP, share))
    _check(dev, want, max_mismatch_frac=1e-3 if want.size >= SHARE_PIXELS else 1.0)


def _max_samples(c):
    return int((np.rint(c['t2'] * c['fs']) - np.rint(c['t1'] * c['fs'])).max())


def _abi(name, target_times, out, max_samples, ws=None):
    """ava_get_spec_batch called directly on a case's windows: the return code"""
    from ava_amd import _lib, spec as sp
    lib = _lib.load()
    c, audio = SC.case(name), _device_audio(name)
    p, dev = c['p'], audio.device
    n, T = target_times.shape
    F = len(c['target_freqs'])
    window, scale = sp._stft_constants(p['nperseg'], dev)
    d = [torch.from_numpy(np.array(a)).to(dev) for a in (c['fidx'], c['t1'], c['t2'], target_times, c['target_freqs'])]
    if ws is None:
        ws = torch.empty(max(1, lib.ava_spec_workspace_bytes(n, max_samples, p['nperseg'], p['noverlap'], F, T, 0)),
                         dtype=torch.uint8, device=dev)
    rc = lib.ava_get_spec_batch(audio.samples.data_ptr(), audio.code, audio.file_off.data_ptr(), audio.file_len.data_ptr(),
                                d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, max_samples,
                                float(c['fs']), p['nperseg'], p['noverlap'], window.data_ptr(), scale, d[4].data_ptr(), F, T,
                                float(p['spec_min_val']), float(p['spec_max_val']), float(c['fill_value']), 1, 0, 0, 0.0,
                                out.data_ptr(), None, ws.data_ptr(), ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    return rc


# ---- 1. table edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.TABLE_NAMES)
def test_column_table_strides_and_partial_row_groups(name):
    """F = 1, 15, 16, 17, 31, 33 rows (one group, a partial last group, whole groups) by T = 1, 255 .. 257 and 511, 512
    columns (the second stride of the 512-entry column table and its last entry).  table_1_1 has three pixels, all
    strictly inside (0, 1) by a clip floor of -20: ulp bound alone."""
    _hold(name, _run(name), SC.expected(name))


def test_more_than_512_target_times_are_refused():
    from ava_amd import spec as sp
    c = SC.case("table_31_512")
    on = c['target_times'][:, 0]
    tt = np.linspace(on, on + c['p']['window_length'], 513, axis=-1)
    with pytest.raises(NotImplementedError):
        sp.get_spec_batch(_device_audio("table_31_512"), c['fidx'], c['t1'], c['t2'], c['p'], c['fs'], tt)
    out = torch.full((len(on), 31, 513), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    assert _abi("table_31_512", tt, out, _max_samples(c), ws=ws) == AVA_EINVAL
    assert (out == 7.0).all().item()                               # nothing was launched


# ---- 2. knots ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.KNOT_NAMES)
def test_targets_on_beside_and_outside_the_knots(name):
    """target times / frequencies exactly on the first, second (an interior) and last knot, one fp64 step either side of
    each, before and after the grid; with the default fill (clips to 0), with the visible fill (4 - 2) / 4.5, and with
    NaN in place of the out-of-grid targets (the oracle keeps the out-of-grid value).  knots_freq* have 3840 pixels: ulp
    bound alone; knots_time* have 4464: both conditions."""
    want = SC.expected(name)
    dev = _run(name)
    _hold(name, dev, want)
    if SC.case(name)['fill_value'] == SC.KNOT_FILL:                # the fill constant is where the oracle has it, to the bit
        fillc = np.float32((SC.KNOT_FILL - 2.0) / 4.5)
        assert ((dev.cpu().numpy() == fillc) == (want == (SC.KNOT_FILL - 2.0) / 4.5)).all()


# ---- 3. slice mean -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.MEAN_NAMES)
def test_slice_mean_at_every_alignment_of_the_slice(name):
    """0 .. 500 Hz, clip floor at -12, recordings with a DC offset of 900: a mean that forgets one sample moves pixels
    by thousands of tolerances (tests/test_cpu_spec_cases.py).  The slices start at every offset mod 8 of the
    concatenated buffer and end at seven of them: the scalar head, vector body and scalar tail of the int16 sum, the
    plain loop of int32 and float64; the float64 recordings once more with the mean left in (4096 pixels each)."""
    want = SC.expected(name)
    assert want.min() > 0.0
    _hold(name, _run(name), want)


# ---- 4. pruning under a poisoned workspace -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.PRUNE_NAMES)
def test_pruned_frames_and_bins_are_never_read(name):
    """target grids that cover a thirtieth of the slice and a narrow band: all but a few frames and bins are left
    untransformed.  The cached workspace is filled with 0xFF bytes (every double a NaN) before the call: a pixel that
    read an unwritten frame or bin is NaN.  Afterwards most of the workspace still is NaN, so memory was left unwritten
    (4608 pixels a case: both conditions)."""
    from ava_amd import _lib, spec as sp
    c = SC.case(name)
    p, dev = c['p'], _device_audio(name).device
    n, T = c['target_times'].shape
    nbytes = _lib.load().ava_spec_workspace_bytes(n, _max_samples(c), p['nperseg'], p['noverlap'], len(c['target_freqs']), T, 0)
    assert nbytes > 0
    ws = sp._workspace(dev, nbytes)
    ws.fill_(0xFF)
    out = _run(name)
    assert sp._workspace(dev, nbytes) is ws                        # the call used the poisoned buffer
    assert not torch.isnan(out).any().item()
    _hold(name, out, SC.expected(name))
    left = torch.isnan(ws[:nbytes - nbytes % 8].view(torch.float64)).double().mean().item()
    print("%s: %.3f of the workspace's doubles still NaN" % (name, left))
    assert left > 0.5


# ---- 5. frame count ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.FRAME_NAMES)
def test_smallest_slices_and_whole_hops(name):
    """slices of nperseg samples, nperseg - 1 (zeros), ten hops and ten hops + 1 (one frame more), target times from the
    first to the last sample of the slice (4096 pixels: both conditions)"""
    dev = _run(name)
    _hold(name, dev, SC.expected(name))
    assert not dev[1].any().item() and dev[0].any().item()


# ---- 6. quantile select ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.QUANT_GRID_NAMES + SC.QUANT_ONES_NAMES)
def test_quantile_select_at_its_edges(name):
    """within_syll_normalize with F T = 1, 1023, 1025 and 17 x 257 values (none a multiple of the 1024 threads) and the
    order statistics 0, the median's, n - 2 and n - 1; the last window is silent (all 0 after the clip); in quant_ones_*
    every pixel clips to 1: zeros.  Cases under 4096 pixels (F T < 1024 a window): ulp bound alone."""
    want = SC.expected(name)
    dev, mx = _run(name, return_max=True)
    _hold(name, dev, want)
    n = want.shape[0]
    assert not dev[-1].any().item()
    assert np.allclose(mx.cpu().numpy(), want.reshape(n, -1).max(axis=1).astype(np.float32), atol=ULP)


# ---- 7. scratch too small ----------------------------------------------------------------------------------------------
def test_a_window_longer_than_max_samples_is_nan_and_the_others_are_right():
    """the documented marker of a window whose frames do not fit the caller's scratch (nframes = -1): all NaN, nothing
    transformed; every other window of the batch is the oracle's (2304 pixels: ulp bound alone)"""
    c, want = SC.case("scratch"), SC.expected("scratch")
    n = len(c['t1'])
    others = [i for i in range(n) if i != SC.SCRATCH_LONG]
    samples = [hi - lo for lo, hi in (SC.slice_of(c, i) for i in range(n))]
    max_samples = max(samples[i] for i in others)
    assert max_samples < samples[SC.SCRATCH_LONG]
    out = torch.full(want.shape, 7.0, dtype=torch.float32, device="cuda")
    assert _abi("scratch", c['target_times'], out, max_samples) == 0
    assert torch.isnan(out[SC.SCRATCH_LONG]).all().item()
    _hold("scratch", out[others], want[others])


# ---- 8. batch independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.KNOT_NAMES + SC.MEAN_NAMES)
def test_a_window_alone_and_in_a_batch_has_equal_bytes(name):
    n = len(SC.case(name)['t1'])
    for i in range(n):
        rest = [j for j in range(n) if j != i]
        alone = _run(name, [i])[0]
        first = _run(name, [i] + rest)[0]
        last = _run(name, rest + [i])[-1]
        assert torch.equal(alone.view(torch.int32), first.view(torch.int32)), (name, i)
        assert torch.equal(alone.view(torch.int32), last.view(torch.int32)), (name, i)
