"""GPU tests of the warped-window row: windows out of the motif cache (csrc/warp_spec.hip, via
ava_amd.warped_window) against the f4 path on the same draws (bit for bit), against oracle/spec_oracle.py on the
arguments the real WarpedWindowDataset handed to get_spec (tests/golden/warped.npz), and through the VAE.

Tolerances.  Cache path against f4 path: none, torch.equal -- both run the same device functions on the same fp64
inputs.  Against the oracle: f4's bound (tests/test_gpu_spec.py): at most one fp32 ulp anywhere,
bit-identical on >= 99.9 % of the pixels; float32 audio: 2e-3, what f4 states for it (the reference transforms float32
audio in single precision).  Fit inputs: 4x the noise floor stored with the golden."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import warped_cases as WC
from ava_amd import synthetic as syn
from oracle import spec_oracle as so

pytestmark = pytest.mark.gpu

ULP = 6e-8


@pytest.fixture(scope="module")
def G():
    return WC.load()


def _case_dataset(name, G, which='all', **kw):
    """the dataset of a golden case from arrays: null knots, or the knots the golden script saved"""
    from ava_amd import warped_window as ww
    recipe, p = WC.RECIPES[name], WC.params(name)
    audio = WC.motifs(recipe)
    td = float(G['%s.%s.template_dur' % (name, which)])
    if which == 'null':
        return ww.DeviceWarpedWindowDataset.from_arrays(audio, recipe['fs'], p, **kw), audio, p
    xk, yk = WC.knots(len(audio), G[name + '.n_knots.json'], recipe['salt'] + 1)
    if which == 'subset':
        keep = sorted(G[name + '.subset.json'])
        audio, xk, yk = [audio[k] for k in keep], xk[keep], yk[keep]
        kw = dict(dict(start_q=0.05, stop_q=0.9), **kw)
    return ww.DeviceWarpedWindowDataset.from_arrays(audio, recipe['fs'], p, x_knots=xk, y_knots=yk, template_dur=td, **kw), audio, p


def _f4(ds, file_idx, target_times):
    from ava_amd import spec as sp
    n = len(file_idx)
    return sp.get_spec_batch(ds.audio, file_idx, np.zeros(n), np.full(n, ds.template_dur), ds.p, ds.fs, target_times)


def _check_oracle(dev, want, max_mismatch_frac=1e-3):
    got = dev.cpu().numpy()
    w32 = want.astype(np.float32)
    assert got.shape == w32.shape and got.dtype == np.float32
    err, frac = np.abs(got.astype(np.float64) - want).max(), (got != w32).mean()
    print("max abs err %.3e, mismatching pixels %.3e" % (err, frac))
    assert err <= ULP
    assert frac <= max_mismatch_frac


def _generic(p, dtype, n_files=4, template_dur=None, **kw):
    """a dataset over synthetic motifs of ``dtype`` with 4-knot warps"""
    from ava_amd import warped_window as ww
    audio = WC.motifs(dict(n_files=n_files, fs=p['fs'], motif_seconds=0.3, salt=4411, dtype=np.dtype(dtype).name))
    if np.dtype(dtype).kind == 'f':
        p = dict(p, spec_min_val=p['spec_min_val'] - WC.LOG_INT16_SCALE, spec_max_val=p['spec_max_val'] - WC.LOG_INT16_SCALE)
    xk, yk = WC.knots(n_files, 4, 515)
    return ww.DeviceWarpedWindowDataset.from_arrays(audio, p['fs'], p, x_knots=xk, y_knots=yk, template_dur=template_dur, **kw)


MOUSE = dict(syn.MOUSE_PARAMS, spec_min_val=-2.0, spec_max_val=4.0)       # int16-scaled synthetic audio at 250 kHz
EQUAL_CASES = {
    "finch_int16": (syn.FINCH_PARAMS, np.int16, {}),
    "finch_float32": (syn.FINCH_PARAMS, np.float32, {}),
    "finch_float64": (syn.FINCH_PARAMS, np.float64, {}),
    "mouse_int16": (MOUSE, np.int16, {}),
    "nperseg_400": (dict(syn.FINCH_PARAMS, nperseg=400, noverlap=200), np.int16, {}),
    "linear_spacing": (dict(syn.FINCH_PARAMS, mel=False, num_freq_bins=96, num_time_bins=80), np.int16, {}),
    "within_syll_normalize": (dict(syn.FINCH_PARAMS, within_syll_normalize=True, normalize_quantile=0.5, spec_min_val=1.0),
                              np.int16, {}),
    "start_stop_q": (syn.FINCH_PARAMS, np.int16, dict(start_q=0.2, stop_q=0.8)),
    "short_template": (syn.FINCH_PARAMS, np.int16, dict(template_dur=0.2)),
}


@pytest.mark.parametrize("case", sorted(EQUAL_CASES))
def test_cache_path_equals_f4_path_bit_for_bit(case):
    """ds[list] against get_spec_batch(audio, file_idx, 0.0, template_dur, p, fs, target_times) on the same draws"""
    p, dtype, kw = EQUAL_CASES[case]
    ds = _generic(dict(p), dtype, **kw)
    for n, seed in ((64, 1), (7, 2)):
        file_idx, tt = ds._draw(n, seed)
        got = ds.__getitem__(list(range(n)), seed=seed)
        want = _f4(ds, file_idx, tt)
        assert got.dtype == torch.float32 and got.shape == (n, ds.p['num_freq_bins'], ds.p['num_time_bins']) and got.is_cuda
        assert torch.equal(got, want), "%s: %d pixels differ" % (case, int((got != want).sum()))
        assert float(want.max()) > 0.5 and float((want > 0).float().mean()) > 0.005     # not blank


def test_short_file_and_windows_outside_the_motif_equal_f4_and_are_zero():
    """a file shorter than nperseg yields zeros (utils.py:68-69); target times wholly outside [0, template_dur] take
    interp2d's fill value and clip to zero"""
    from ava_amd import warped_window as ww
    p = dict(syn.FINCH_PARAMS)
    audio = WC.motifs(dict(n_files=3, fs=p['fs'], motif_seconds=0.3, salt=4411, dtype='int16'))
    audio.insert(1, audio[0][:300].copy())                                           # 300 < nperseg = 512
    ds = ww.DeviceWarpedWindowDataset.from_arrays(audio, p['fs'], p, template_dur=0.3)
    T = p['num_time_bins']
    fidx = np.array([0, 1, 2, 3, 0, 2])
    tt = np.stack([np.linspace(0.05, 0.17, T), np.linspace(0.05, 0.17, T), np.linspace(-0.2, -0.08, T),
                   np.linspace(0.9, 1.02, T), np.linspace(-0.05, 0.07, T), np.linspace(0.25, 0.37, T)])
    got, want = ds.windows(fidx, tt), _f4(ds, fidx, tt)
    assert torch.equal(got, want)
    assert got[0].any().item() and got[4].any().item()
    assert not got[1].any().item() and not got[2].any().item() and not got[3].any().item()
    assert not got[4][:, :20].any().item()                                           # the part before the motif's first frame
    # seeded batches over the set with the short file still equal f4's
    file_idx, tt = ds._draw(32, 9)
    assert (file_idx == 1).any() and torch.equal(ds.__getitem__(list(range(32)), seed=9), _f4(ds, file_idx, tt))


@pytest.mark.parametrize("name,which", [("finch_int16", "null"), ("finch_int16", "all"), ("finch_int16", "subset")])
def test_golden_calls_match_the_oracle(name, which, G):
    """oracle/spec_oracle.get_spec on the arguments the real WarpedWindowDataset passed, against the cache path"""
    ds, audio, p = _case_dataset(name, G, which)
    key = "%s.%s" % (name, which)
    for call in ("list16_seed11", "single_seed13", "specific", "whole128", "whole200"):
        k = "%s.%s" % (key, call)
        fidx, tt = G[k + '.file_idx'], G[k + '.target_times']
        want = np.stack([so.get_spec(G[k + '.t1'][i], G[k + '.t2'][i], audio[fidx[i]], p, fs=int(G[k + '.fs'][i]),
                                     target_times=tt[i], max_dur=None)[0] for i in range(len(fidx))])
        _check_oracle(ds.windows(fidx, tt), want)
        assert want.max() > 0.5
    fns = ds.audio_filenames
    w = ds.get_whole_warped_spectrogram(fns[1], time_bins=200)
    assert isinstance(w, np.ndarray) and w.shape == (p['num_freq_bins'], 200)
    assert np.array_equal(w, ds.windows(G[key + '.whole200.file_idx'], G[key + '.whole200.target_times'])[0].cpu().numpy())
    s = ds.get_specific_item(fns[-1], 0.37)
    assert isinstance(s, np.ndarray) and np.array_equal(s, ds.windows(G[key + '.specific.file_idx'][1:2], G[key + '.specific.target_times'][1:2])[0].cpu().numpy())


def test_float32_audio_against_the_oracle(G):
    """what f4 states for float32 recordings (tests/test_gpu_spec.py::test_audio_dtypes): 2e-3"""
    ds, audio, p = _case_dataset("finch_float32", G, "all")
    k = "finch_float32.all.list16_seed11"
    fidx, tt = G[k + '.file_idx'], G[k + '.target_times']
    want = np.stack([so.get_spec(0.0, ds.template_dur, audio[fidx[i]], p, fs=ds.fs, target_times=tt[i], max_dur=None)[0]
                     for i in range(len(fidx))])
    err = np.abs(ds.windows(fidx, tt).cpu().numpy() - want).max()
    print("float32 audio: max abs err %.3e" % err)
    assert want.max() > 0.5 and err < 2e-3


@pytest.mark.parametrize("name", ["finch_int16", "finch_float32"])
def test_seeded_batch_is_the_reference_batch(name, G):
    for which in ("null", "all", "subset"):
        ds, audio, p = _case_dataset(name, G, which)
        key = "%s.%s" % (name, which)
        for seed in (11, 5):
            k = '%s.list16_seed%d' % (key, seed)
            got = ds.__getitem__(list(range(16)), seed=seed)
            assert torch.equal(got, ds.windows(G[k + '.file_idx'], G[k + '.target_times']))
        one = ds.__getitem__(0, seed=13)
        assert one.shape == (p['num_freq_bins'], p['num_time_bins']) and one.is_cuda and one.dtype == torch.float32
        k = key + '.single_seed13'
        assert torch.equal(one, ds.windows(G[k + '.file_idx'], G[k + '.target_times'])[0])


@pytest.mark.parametrize("fit", ["fit_int16", "fit_float32", "fit_band256"])
def test_fit_inputs_on_the_device_match_the_reference(fit, G):
    from ava_amd import warped_window as ww
    recipe, p = WC.RECIPES[G[fit + '.audio_case.json']], WC.params(G[fit + '.params.json'])
    specs, amps, template_dur = ww.get_specs_and_amplitude_traces(WC.motifs(recipe), recipe['fs'], p)
    assert template_dur == float(G[fit + '.template_dur'])
    assert specs.shape == tuple(G[fit + '.specs_shape']) and str(specs.dtype) == G[fit + '.specs_dtype.json']
    assert amps.shape == G[fit + '.amps'].shape and amps.dtype == G[fit + '.amps'].dtype
    idx = WC.spec_samples(specs.size, recipe['salt'])
    ds = np.abs(specs.reshape(-1)[idx].astype(np.float64) - G[fit + '.specs_sampled']).max()
    da = np.abs(amps.astype(np.float64) - G[fit + '.amps']).max()
    print("%s: specs %.3e (floor %.3e)  amps %.3e (floor %.3e)" % (fit, ds, float(G[fit + '.specs_floor']), da,
                                                                    float(G[fit + '.amps_floor'])))
    assert ds <= 4.0 * float(G[fit + '.specs_floor'])
    assert da <= 4.0 * float(G[fit + '.amps_floor'])
    assert specs.max() > 0.5
    with pytest.raises(NotImplementedError):
        ww.get_specs_and_amplitude_traces(WC.motifs(recipe), recipe['fs'], dict(p, nperseg=400, noverlap=200))


def test_determinism_and_independence_of_the_other_files(G):
    from ava_amd import warped_window as ww
    ds, audio, p = _case_dataset("finch_int16", G, "all")
    c1 = ds.build_cache().clone()
    c2 = ds.build_cache()
    assert torch.equal(c1, c2) and c1.numel() == ds.cache_bytes
    a, b = ds.__getitem__(list(range(64)), seed=4), ds.__getitem__(list(range(64)), seed=4)
    assert torch.equal(a, b)
    # file 2 alone and inside the set: the same windows, hence the same cache rows
    xk, yk = ds.x_knots, ds.y_knots
    alone = ww.DeviceWarpedWindowDataset.from_arrays([audio[2]], ds.fs, p, x_knots=xk[2:3], y_knots=yk[2:3],
                                                     template_dur=ds.template_dur)
    T = p['num_time_bins']
    tt = np.stack([np.linspace(-0.05, ds.template_dur + 0.05, T), np.linspace(0.1, 0.22, T)])
    assert torch.equal(alone.windows([0, 0], tt), ds.windows([2, 2], tt))
    ra, rs = alone.cache_rows(0), ds.cache_rows(2)
    assert ra.shape == rs.shape and ra.shape[0] > 100 and ra.shape[1] > 30 and torch.equal(ra, rs)
    assert torch.isfinite(ra).all() and float(ra.max()) > 5.0


def test_through_the_model_and_the_loaders(tmp_path, G):
    from ava_amd import warped_window as ww
    from ava_amd.vae import VAE
    recipe, p = WC.RECIPES["finch_int16"], WC.params("finch_int16")
    audio = WC.motifs(recipe)
    d = tmp_path / "motifs"
    d.mkdir()
    for k, a in enumerate(audio):
        wavfile.write(str(d / ("m_%02d.wav" % k)), recipe['fs'], a)
    (d / "notes.txt").write_text("not audio")
    warp_fn = str(tmp_path / "warp.npy")
    loaders = ww.get_warped_window_data_loaders([str(d)], p, batch_size=256, warp_fn=warp_fn, warp_type='null')
    assert loaders['train'] is loaders['test'] and loaders['train'].device_resident
    loader = loaders['train']
    ds = loader.dataset
    assert len(ds) == 2048 and len(loader) == 8 and len(ds.audio_filenames) == 5 and os.path.exists(warp_fn)
    batches = list(loader)
    assert len(batches) == len(loader)
    assert all(b.is_cuda and b.dtype == torch.float32 and tuple(b.shape) == (256, 128, 128) for b in batches)
    assert not torch.equal(batches[0], batches[1])
    torch.manual_seed(0)
    model = VAE(save_dir="", z_dim=32, device_name="cuda")
    losses = [model.train_epoch(loader) for _ in range(2)]
    assert all(np.isfinite(l) for l in losses)
    # the knots file is read back
    saved = np.load(warp_fn, allow_pickle=True).item()
    xk, yk = WC.knots(5, 3, 31)
    np.save(warp_fn, dict(saved, x_knots=xk, y_knots=yk))
    again = ww.get_warped_window_data_loaders([str(d)], p, batch_size=64, load_warp=True, warp_fn=warp_fn)
    assert np.array_equal(again['train'].dataset.x_knots, xk) and np.array_equal(again['train'].dataset.y_knots, yk)
    assert again['train'].dataset.template_dur == saved['template_dur'] and len(again['train']) == 32
    b = next(iter(again['train']))
    assert b.is_cuda and tuple(b.shape) == (64, 128, 128) and torch.isfinite(b).all()


def test_c_abi_argument_checks():
    from ava_amd import _lib
    lib = _lib.load()
    geo = (3, 0.25, 32000.0, 512, 256)
    band = (400.0, 10000.0)
    nbytes, wbytes = lib.ava_warp_cache_bytes(*geo, *band), lib.ava_warp_cache_workspace_bytes(*geo)
    assert nbytes > 3 * 100 * 33 * 8 and wbytes > 3 * 33 * 257 * 8
    assert lib.ava_warp_cache_bytes(0, 0.25, 32000.0, 512, 256, *band) == 0            # no files
    assert lib.ava_warp_cache_bytes(3, 0.25, 32000.0, 4096, 256, *band) == 0           # bad nperseg
    assert lib.ava_warp_cache_bytes(3, 0.25, 32000.0, 512, 512, *band) == 0
    assert lib.ava_warp_cache_bytes(3, 0.0, 32000.0, 512, 256, *band) == 0
    assert lib.ava_warp_cache_bytes(3, 0.25, 32000.0, 500, 250, *band) > 0             # any length in 64..2048
    assert lib.ava_warp_windows_workspace_bytes(4, 16, 16, 1) == 256 + 4 * 256 * 8
    lay = (ctypes.c_int64 * 6)()
    for bad in ((0, 0.25, 32000.0, 512, 256), (3, 0.25, 32000.0, 4096, 256), (3, 0.25, 32000.0, 512, 512),
                (3, 0.0, 32000.0, 512, 256)):                                           # where ava_warp_cache_bytes is 0
        assert lib.ava_warp_cache_layout(*bad, *band, lay) == -1
    assert lib.ava_warp_cache_layout(*geo, *band, lay) == 0
    maxframes, fstride, k0, nb, off_ftimes, off_logmag = lay
    assert nbytes == 256 + off_logmag + geo[0] * nb * fstride * 8
    assert maxframes == 33 and fstride == 48 and 0 <= k0 < 400 * 512 // 32000 and nb > 100
    assert off_ftimes == 256 and off_logmag == 256 + 1024                               # 3 int32, 3 x 33 doubles, each up to 256
    dev = torch.device("cuda")
    audio = torch.zeros(3 * 9000, dtype=torch.int16, device=dev)
    off = torch.tensor([0, 9000, 18000], dtype=torch.int64, device=dev)
    ln = torch.full((3,), 9000, dtype=torch.int64, device=dev)
    win = torch.ones(512, dtype=torch.float64, device=dev)
    cache = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(wbytes, dtype=torch.uint8, device=dev)

    def build(audio_ptr=audio.data_ptr(), g=geo, dtype=0, cb=nbytes, wb=wbytes):
        return lib.ava_warp_cache_build(audio_ptr, dtype, off.data_ptr(), ln.data_ptr(), *g, win.data_ptr(), 1.0 / 512, *band,
                                        1, cache.data_ptr(), cb, ws.data_ptr(), wb, _lib.stream())
    assert build(audio_ptr=None) == -1
    assert build(g=(0,) + geo[1:]) == -1
    assert build(g=geo[:3] + (48, 24)) == -1
    assert build(dtype=9) == -1
    assert build(cb=nbytes // 2) == -3
    assert build(wb=wbytes // 2) == -3
    assert build() == 0
    fidx = torch.zeros(4, dtype=torch.int32, device=dev)
    tt = torch.linspace(0.0, 0.2, 64, dtype=torch.float64, device=dev).reshape(4, 16).contiguous()
    tf = torch.linspace(400, 10000, 16, dtype=torch.float64, device=dev)
    out = torch.ones(4, 16, 16, device=dev)
    wws = torch.empty(256 + 4 * 256 * 8, dtype=torch.uint8, device=dev)

    def windows(cache_ptr=cache.data_ptr(), g=geo, n=4, T=16, smax=6.5, norm=0, q_lo=0, gamma=0.0, wb=wws.numel(), cb=nbytes):
        return lib.ava_warp_windows(cache_ptr, cb, *g, *band, fidx.data_ptr(), tt.data_ptr(), n, tf.data_ptr(), 16, T, 2.0,
                                    smax, -1e12, norm, q_lo, gamma, out.data_ptr(), wws.data_ptr(), wb, _lib.stream())
    assert windows(cache_ptr=None) == -1
    assert windows(g=(0,) + geo[1:]) == -1
    assert windows(g=geo[:3] + (5000, 256)) == -1
    assert windows(n=0) == -1
    assert windows(T=513) == -1
    assert windows(smax=2.0) == -1
    assert windows(norm=1, q_lo=256) == -1
    assert windows(norm=1, gamma=1.5) == -1
    assert windows(norm=1, wb=128) == -3
    assert windows(cb=nbytes // 2) == -3
    torch.cuda.synchronize()
    assert bool((out == 1).all())                      # nothing was launched by the refused calls
    assert windows() == 0
    torch.cuda.synchronize()
    assert not out.any().item()                        # silence: log(1e-12) is far below spec_min_val
    assert windows(norm=1, q_lo=10, gamma=0.5) == 0
    torch.cuda.synchronize()
    assert not out.any().item()
    # the Python surface refuses the same shapes before any launch
    from ava_amd import warped_window as ww
    p = dict(syn.FINCH_PARAMS)
    ds = ww.DeviceWarpedWindowDataset.from_arrays([np.zeros(9000, dtype=np.int16)], 32000, p)
    with pytest.raises(NotImplementedError):
        ds.windows([0], np.zeros((1, 600)))
    with pytest.raises(IndexError):
        ds.windows([1], np.zeros((1, 128)))
    with pytest.raises(ValueError):
        ds.windows([], np.zeros((0, 128)))
