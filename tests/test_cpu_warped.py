"""Host logic of the warped-window row, against tests/golden/warped.npz (the real
WarpedWindowDataset of the reference, tests/golden/make_golden_warped.py).  No library call: the draws, the inverse
warp and the knots file never touch the device."""
import os
import sys
import warnings

import numpy as np
import pytest
from scipy.io import wavfile

import warped_cases as WC
from ava_amd import warped_window as ww


@pytest.fixture(scope="module")
def G():
    return WC.load()


def _write_case(tmp, name):
    """the wav files of a case as the golden script wrote them: (names as given, sorted names, motifs, p)"""
    recipe = WC.RECIPES[name]
    audio = WC.motifs(recipe)
    fns = [os.path.join(str(tmp), n) for n in WC.names(len(audio))]
    for k, fn in enumerate(sorted(fns)):
        wavfile.write(fn, recipe['fs'], audio[k])
    return fns, sorted(fns), audio, WC.params(name)


def _knots_file(tmp, name, G, fns_sorted):
    recipe = WC.RECIPES[name]
    n_knots = G[name + '.n_knots.json']
    xk, yk = WC.knots(len(fns_sorted), n_knots, recipe['salt'] + 1)
    path = os.path.join(str(tmp), "knots.npy")
    wp = dict(ww.DEFAULT_WARP_PARAMS, n_knots=n_knots - 2)
    np.save(path, {'x_knots': xk, 'y_knots': yk, 'template_dur': float(G[name + '.null.template_dur']) * 0.96,
                   'audio_filenames': fns_sorted, 'warp_params': wp})
    return path, xk, yk, wp


def _datasets(tmp, name, G):
    """the three datasets the golden script drove: null (saved), all files loaded, a subset loaded"""
    fns, fns_sorted, audio, p = _write_case(tmp, name)
    null_fn = os.path.join(str(tmp), "null_warp.npy")
    out = {'null': (ww.DeviceWarpedWindowDataset(fns, p, warp_fn=null_fn, warp_type='null'), fns_sorted)}
    knots_fn, _, _, _ = _knots_file(tmp, name, G, fns_sorted)
    out['all'] = (ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=knots_fn), fns_sorted)
    sub = [fns_sorted[k] for k in G[name + '.subset.json']]
    out['subset'] = (ww.DeviceWarpedWindowDataset(sub, p, load_warp=True, save_warp=False, warp_fn=knots_fn,
                                                  start_q=0.05, stop_q=0.9), sorted(sub))
    return out, null_fn


def _same(key, G, file_idx, target_times, ds):
    assert np.array_equal(np.asarray(file_idx), G[key + '.file_idx']), key
    want = G[key + '.target_times']
    got = np.asarray(target_times)
    assert got.dtype == np.float64 and got.shape == want.shape, key
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), key           # bit-equal
    assert np.all(G[key + '.t1'] == 0.0) and np.all(G[key + '.t2'] == ds.template_dur) and np.all(G[key + '.fs'] == ds.fs)


@pytest.mark.parametrize("name", ["finch_int16", "finch_float32"])
def test_draws_and_target_times_are_the_reference_bits(name, G, tmp_path):
    """every recorded get_spec call of the real WarpedWindowDataset: which file, and the complete target_times"""
    dss, _ = _datasets(tmp_path, name, G)
    for which, (ds, fns) in dss.items():
        key = "%s.%s" % (name, which)
        assert ds.audio_filenames == fns and ds.fs == WC.RECIPES[name]['fs']
        assert ds.template_dur == float(G[key + '.template_dur'])
        assert ds.window_frac == float(G[key + '.window_frac'])
        assert np.array_equal(ds.x_knots, G[key + '.x_knots']) and np.array_equal(ds.y_knots, G[key + '.y_knots'])
        for seed in (11, 5):
            _same('%s.list16_seed%d' % (key, seed), G, *ds._draw(16, seed), ds)
        _same(key + '.single_seed13', G, *ds._draw(1, 13), ds)
        calls = [ds._specific_times(fn, q) for fn, q in zip((fns[0], fns[-1], fns[1]), (0.0, 0.37, 1.0))]
        _same(key + '.specific', G, [c[0] for c in calls], np.stack([c[1] for c in calls]), ds)
        for bins in (128, 200):
            fi, tt = ds._whole_times(fns[1], bins)
            _same('%s.whole%d' % (key, bins), G, [fi], tt[None, :], ds)
        assert len(ds) == 2048


def test_draw_reseeds_the_global_generator_like_the_reference(G, tmp_path):
    """np.random.seed(seed) ... np.random.seed(None): two seeded calls agree, and the global stream is not left seeded"""
    dss, _ = _datasets(tmp_path, "finch_int16", G)
    ds = dss['all'][0]
    a, b = ds._draw(8, 3), ds._draw(8, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    x, y = np.random.rand(), (ds._draw(8, 3), np.random.rand())[1]
    assert x != y


@pytest.mark.parametrize("name", ["finch_int16", "finch_float32"])
def test_null_warp_and_saved_dict(name, G, tmp_path):
    dss, null_fn = _datasets(tmp_path, name, G)
    ds, fns = dss['null']
    n = len(fns)
    assert np.array_equal(ds.x_knots, np.tile([0.0, 1.0], (n, 1))) and np.array_equal(ds.y_knots, ds.x_knots)
    assert ds.y_knots is not ds.x_knots
    saved = np.load(null_fn, allow_pickle=True).item()
    assert sorted(saved.keys()) == G[name + '.null.saved_keys.json']
    assert saved['warp_params'] == G[name + '.null.warp_params.json'] == ds.warp_params
    assert saved['audio_filenames'] == fns and saved['template_dur'] == ds.template_dur
    assert np.array_equal(saved['x_knots'], ds.x_knots) and np.array_equal(saved['y_knots'], ds.y_knots)
    assert ds.template_dur == ww.template_duration([len(a) for a in WC.motifs(WC.RECIPES[name])], ds.fs, ds.p)
    assert ds.window_frac == ds.p['window_length'] / ds.template_dur


def test_loaded_knots_subset_permutation_and_params(G, tmp_path):
    name = "finch_int16"
    fns, fns_sorted, audio, p = _write_case(tmp_path, name)
    knots_fn, xk, yk, wp = _knots_file(tmp_path, name, G, fns_sorted)
    subset = G[name + '.subset.json']                       # given unsorted: the dataset sorts its names
    ds = ww.DeviceWarpedWindowDataset([fns_sorted[k] for k in subset], p, load_warp=True, save_warp=False, warp_fn=knots_fn)
    assert np.array_equal(ds.x_knots, xk[sorted(subset)]) and np.array_equal(ds.y_knots, yk[sorted(subset)])
    assert ds.warp_params == wp and isinstance(ds.audio_filenames, list)
    assert ds.template_dur == float(G[name + '.null.template_dur']) * 0.96
    full = ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=knots_fn, warp_params={'n_knots': 9})
    assert np.array_equal(full.x_knots, xk) and full.warp_params == wp          # the file's parameters win (:552)


def test_load_path_asserts_and_warnings(G, tmp_path):
    name = "finch_int16"
    fns, fns_sorted, audio, p = _write_case(tmp_path, name)
    knots_fn, xk, yk, wp = _knots_file(tmp_path, name, G, fns_sorted)
    base = np.load(knots_fn, allow_pickle=True).item()

    def saved(**kw):
        path = os.path.join(str(tmp_path), "k_%d.npy" % len(os.listdir(str(tmp_path))))
        np.save(path, dict(base, **kw))
        return path

    with pytest.raises(AssertionError, match="must be specified to save warps"):
        ww.DeviceWarpedWindowDataset(fns, p, warp_type='null')
    with pytest.raises(AssertionError):
        ww.DeviceWarpedWindowDataset(fns, p, warp_type='dtw', save_warp=False)
    with pytest.raises(AssertionError):
        ww.DeviceWarpedWindowDataset(fns, [p], warp_type='null', save_warp=False)
    with pytest.raises(AssertionError, match="are not sorted"):
        ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=saved(audio_filenames=fns_sorted[::-1]))
    with pytest.raises(AssertionError):                                          # fewer saved names than files
        ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=saved(audio_filenames=fns_sorted[:3]))
    renamed = fns_sorted[:-1] + [fns_sorted[-1] + "x"]
    with pytest.raises(AssertionError, match="do not match saved filenames"):
        ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=saved(audio_filenames=renamed))
    with pytest.raises(AssertionError, match="Could not find filename"):
        ww.DeviceWarpedWindowDataset(fns[:2] if fns_sorted[-1] in fns[:2] else [fns_sorted[-1], fns_sorted[0]], p,
                                     load_warp=True, save_warp=False, warp_fn=saved(audio_filenames=renamed))
    with pytest.raises(AssertionError):                                          # duplicates in a subset
        ww.DeviceWarpedWindowDataset([fns_sorted[0], fns_sorted[0]], p, load_warp=True, save_warp=False, warp_fn=knots_fn)
    # nothing to load from: the two warnings, then the fit path, which needs affinewarp
    assert 'affinewarp' not in sys.modules or sys.modules['affinewarp'] is None
    with pytest.warns(UserWarning, match="``warp_fns`` is None"), pytest.raises(ImportError, match="load_warp"):
        ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False)
    missing = os.path.join(str(tmp_path), "nothing_here.npy")
    with pytest.warns(UserWarning, match="Can't load warps from"), pytest.raises(ImportError, match="warp_type='null'"):
        ww.DeviceWarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=missing)


@pytest.mark.parametrize("warp_type", ["amplitude", "spectrogram"])
def test_fit_without_affinewarp_is_an_import_error(warp_type, tmp_path):
    fns, fns_sorted, audio, p = _write_case(tmp_path, "finch_float32")
    with pytest.raises(ImportError, match="affinewarp") as e:
        ww.DeviceWarpedWindowDataset(fns, p, warp_type=warp_type, save_warp=False)
    assert "load_warp" in str(e.value) and "warp_type='null'" in str(e.value)


def test_from_arrays_and_knot_checks():
    name = "finch_int16"
    audio, p = WC.motifs(WC.RECIPES[name]), WC.params(name)
    ds = ww.DeviceWarpedWindowDataset.from_arrays(audio, 32000, p, dataset_length=96)
    assert len(ds) == 96 and ds.x_knots.shape == (5, 2) and ds.template_dur == ww.template_duration([len(a) for a in audio], 32000, p)
    xk, yk = WC.knots(5, 4, 77)
    ds = ww.DeviceWarpedWindowDataset.from_arrays(audio, 32000, p, x_knots=xk, y_knots=yk, template_dur=0.4)
    assert ds.window_frac == p['window_length'] / 0.4
    fi, tt = ds._draw(4, 2)
    assert fi.shape == (4,) and tt.shape == (4, p['num_time_bins']) and np.all(np.diff(tt, axis=1) > 0)
    bad = yk.copy()
    bad[2, 2] = bad[2, 1]
    with pytest.raises(ValueError, match="strictly increasing"):
        ww.DeviceWarpedWindowDataset.from_arrays(audio, 32000, p, x_knots=xk, y_knots=bad)
    with pytest.raises(ValueError):
        ww.DeviceWarpedWindowDataset.from_arrays(audio, 32000, p, x_knots=xk)
    with pytest.raises(ValueError):
        ww.DeviceWarpedWindowDataset.from_arrays(audio, 32000, p, x_knots=xk[:3], y_knots=yk[:3])
    with pytest.raises(NotImplementedError):
        ww.DeviceWarpedWindowDataset.from_arrays(audio, 32000, dict(p, nperseg=4096, noverlap=2048))
    with pytest.raises(NotImplementedError):
        ww.DeviceWarpedWindowDataset.from_arrays(audio, 32000, dict(p, num_time_bins=600))
    with pytest.raises(ValueError, match="fewer than nperseg"):
        ww.DeviceWarpedWindowDataset.from_arrays(audio + [audio[0][:100]], 32000, p)


@pytest.mark.parametrize("fit", ["fit_int16", "fit_float32", "fit_band256"])
def test_numpy_restatement_of_the_fit_inputs_is_within_the_reference_noise(fit, G):
    """tests/warped_cases.specs_and_amps against the real _get_specs_and_amplitude_traces, within 4x the distance the
    golden script measured between the reference and a second fp64 evaluation ('Oracle pin')"""
    recipe, p = WC.RECIPES[G[fit + '.audio_case.json']], WC.params(G[fit + '.params.json'])
    specs, amps, template_dur = WC.specs_and_amps(WC.motifs(recipe), recipe['fs'], p)
    assert template_dur == float(G[fit + '.template_dur'])
    assert specs.shape == tuple(G[fit + '.specs_shape']) and amps.shape == G[fit + '.amps'].shape
    idx = WC.spec_samples(specs.size, recipe['salt'])
    ds, da = np.abs(specs.reshape(-1)[idx] - G[fit + '.specs_sampled']).max(), np.abs(amps - G[fit + '.amps']).max()
    print("%s: specs %.3e (floor %.3e)  amps %.3e (floor %.3e)" % (fit, ds, float(G[fit + '.specs_floor']), da,
                                                                    float(G[fit + '.amps_floor'])))
    assert ds <= 4.0 * float(G[fit + '.specs_floor'])
    assert da <= 4.0 * float(G[fit + '.amps_floor'])


def test_install_points_the_reference_names_here():
    import types
    mod = types.ModuleType("window_vae_dataset")
    assert ww.install(mod) is mod
    assert mod.WarpedWindowDataset is ww.DeviceWarpedWindowDataset
    assert mod.get_warped_window_data_loaders is ww.get_warped_window_data_loaders
    assert not hasattr(ww.DeviceWarpedWindowDataset, "write_hdf5_files")
