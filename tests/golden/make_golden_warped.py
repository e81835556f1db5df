"""Writes tests/golden/warped.npz: the reference's ``WarpedWindowDataset`` (ava/models/window_vae_dataset.py:358-701)
and ``_get_specs_and_amplitude_traces`` (ava/models/utils.py:337-418) on synthetic song motifs.  Needs the reference
package and scipy; run from the repository root as ``python tests/golden/make_golden_warped.py /path/to/reference``.
The tests only read the npz.

The reference module imports affinewarp and h5py at load time; neither is used on the paths driven here (the null warp,
saved knots, the window draw), so they are stubbed as in make_golden.py.  The reference's own ``get_spec`` cannot run on
SciPy >= 1.14 (``interp2d`` was removed), so the class is driven through its ``p['get_spec']`` hook with a recorder that
keeps every argument: which file, ``t1``, ``t2``, ``fs``, ``max_dur`` and the complete ``target_times``.

Per case (tests/warped_cases.py regenerates its motif files from the recipe):
  ``null``     warp_type='null', save_warp=True: template_dur, the knots, the keys of the saved dict
  ``all``      load_warp=True from a knots file this script wrote for all files
  ``subset``   load_warp=True for some of the files of a knots file: pins the permutation
and for each of them seeded ``__getitem__`` calls (a list of 16, a single int), ``get_specific_item`` and
``get_whole_warped_spectrogram``.  Also the real ``_get_specs_and_amplitude_traces`` outputs (``specs`` at hashed
indices, ``amps``, ``template_dur``) with a noise floor: the largest absolute difference between the reference's values
and the same expressions evaluated in fp64 from a ``numpy.fft.rfft`` STFT whose window products are formed in
longdouble (tests/warped_cases.py) -- how far two honest evaluations of the formula lie apart.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
from scipy.io import wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AVA_REFERENCE", "../reference"))

for _m in ("h5py", "affinewarp", "affinewarp.crossval"):
    sys.modules[_m] = types.ModuleType(_m)
sys.modules["affinewarp"].PiecewiseWarping = object
sys.modules["affinewarp.crossval"].paramsearch = None

import warped_cases as WC                                       # noqa: E402
import ava.models.window_vae_dataset as W                       # noqa: E402
from ava.models.utils import _get_specs_and_amplitude_traces    # noqa: E402

OUT = {}


class Recorder:
    """``p['get_spec']``: keeps the arguments, answers with a blank spectrogram"""

    def __init__(self, ds_audio, shape):
        self.audio, self.shape, self.calls = ds_audio, shape, []

    def __call__(self, t1, t2, audio, p, fs=32000, max_dur='unset', target_times=None):
        file_index = [i for i, a in enumerate(self.audio()) if a is audio]
        assert len(file_index) == 1 and max_dur is None
        self.calls.append((file_index[0], t1, t2, fs, np.array(target_times, dtype=np.float64, copy=True)))
        return np.zeros((self.shape[0], len(target_times))), True

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def put(key, calls):
    OUT[key + '.file_idx'] = np.array([c[0] for c in calls], dtype=np.int64)
    OUT[key + '.t1'] = np.array([c[1] for c in calls], dtype=np.float64)
    OUT[key + '.t2'] = np.array([c[2] for c in calls], dtype=np.float64)
    OUT[key + '.fs'] = np.array([c[3] for c in calls], dtype=np.float64)
    OUT[key + '.target_times'] = np.stack([c[4] for c in calls])


def drive(key, ds, rec, fns):
    """the recorded calls of one dataset"""
    OUT[key + '.x_knots'], OUT[key + '.y_knots'] = np.array(ds.x_knots), np.array(ds.y_knots)
    OUT[key + '.template_dur'] = np.array(ds.template_dur)
    OUT[key + '.window_frac'] = np.array(ds.window_frac)
    for seed in (11, 5):
        out = ds.__getitem__(list(range(16)), seed=seed)
        assert isinstance(out, list) and len(out) == 16
        put('%s.list16_seed%d' % (key, seed), rec.take())
    out = ds.__getitem__(0, seed=13)
    assert out.shape == rec.shape
    put(key + '.single_seed13', rec.take())
    calls = []
    for fn, q in zip((fns[0], fns[-1], fns[1]), (0.0, 0.37, 1.0)):
        ds.get_specific_item(fn, q)
        calls += rec.take()
    put(key + '.specific', calls)
    for bins in (128, 200):
        ds.get_whole_warped_spectrogram(fns[1], time_bins=bins)
        put('%s.whole%d' % (key, bins), rec.take())


def case(name, n_knots, subset):
    recipe = WC.RECIPES[name]
    p = WC.params(name)
    audio = WC.motifs(recipe)
    wav_names = WC.names(len(audio))
    OUT[name + '.recipe.json'] = np.array(json.dumps(recipe))
    OUT[name + '.n_knots.json'] = np.array(json.dumps(n_knots))
    OUT[name + '.subset.json'] = np.array(json.dumps(subset))
    with tempfile.TemporaryDirectory() as tmp:
        # file k (in sorted-name order) holds motif k: the dataset sorts its file names
        fns = [os.path.join(tmp, n) for n in wav_names]
        for k, fn in enumerate(sorted(fns)):
            wavfile.write(fn, recipe['fs'], audio[k])
        holder = {}
        rec = Recorder(lambda: holder['ds'].audio, (p['num_freq_bins'], p['num_time_bins']))
        p['get_spec'] = rec
        # the null warp, saved
        warp_fn = os.path.join(tmp, "null_warp.npy")
        ds = holder['ds'] = W.WarpedWindowDataset(fns, p, warp_fn=warp_fn, warp_type='null')
        assert ds.audio_filenames == sorted(fns) and ds.fs == recipe['fs']
        saved = np.load(warp_fn, allow_pickle=True).item()
        OUT[name + '.null.saved_keys.json'] = np.array(json.dumps(sorted(saved.keys())))
        OUT[name + '.null.warp_params.json'] = np.array(json.dumps(saved['warp_params']))
        drive(name + '.null', ds, rec, sorted(fns))
        # knots written here for all files, loaded by all files and by a subset (given in unsorted order)
        xk, yk = WC.knots(len(audio), n_knots, recipe['salt'] + 1)
        knots_fn = os.path.join(tmp, "knots.npy")
        wp = dict(W.DEFAULT_WARP_PARAMS, n_knots=n_knots - 2)
        np.save(knots_fn, {'x_knots': xk, 'y_knots': yk, 'template_dur': ds.template_dur * 0.96,
                           'audio_filenames': sorted(fns), 'warp_params': wp})
        ds = holder['ds'] = W.WarpedWindowDataset(fns, p, load_warp=True, save_warp=False, warp_fn=knots_fn)
        assert ds.warp_params == wp
        drive(name + '.all', ds, rec, sorted(fns))
        sub = [sorted(fns)[k] for k in subset]
        ds = holder['ds'] = W.WarpedWindowDataset(sub, p, load_warp=True, save_warp=False, warp_fn=knots_fn,
                                                  start_q=0.05, stop_q=0.9)
        assert ds.audio_filenames == sorted(sub)
        drive(name + '.subset', ds, rec, sorted(sub))
    print("%-16s %d files, lengths %s, template_dur %.6f" % (name, len(audio), [len(a) for a in audio],
                                                              float(OUT[name + '.null.template_dur'])))


def fit_inputs(name, audio_case, pname):
    """the real _get_specs_and_amplitude_traces, with its distance from the fp64 restatement"""
    recipe, p = WC.RECIPES[audio_case], WC.params(pname)
    audio = WC.motifs(recipe)
    specs, amps, template_dur = _get_specs_and_amplitude_traces(audio, recipe['fs'], p)
    s2, a2, t2 = WC.specs_and_amps(audio, recipe['fs'], p, longdouble_products=True)
    assert specs.shape == s2.shape and amps.shape == a2.shape and template_dur == t2
    idx = WC.spec_samples(specs.size, recipe['salt'])
    OUT[name + '.audio_case.json'] = np.array(json.dumps(audio_case))
    OUT[name + '.params.json'] = np.array(json.dumps(pname))
    OUT[name + '.specs_shape'] = np.array(specs.shape)
    OUT[name + '.specs_dtype.json'] = np.array(json.dumps(str(specs.dtype)))
    OUT[name + '.specs_sampled'] = specs.reshape(-1)[idx]
    OUT[name + '.amps'] = amps
    OUT[name + '.template_dur'] = np.array(template_dur)
    OUT[name + '.specs_floor'] = np.array(float(np.abs(specs.astype(np.float64) - s2).max()))
    OUT[name + '.amps_floor'] = np.array(float(np.abs(amps.astype(np.float64) - a2).max()))
    assert specs.max() > 0.5 and (specs > 0).mean() > 0.05, "blank fixture"
    print("%-16s specs %s %s  floor specs %.3e amps %.3e" % (name, specs.shape, specs.dtype,
                                                             float(OUT[name + '.specs_floor']),
                                                             float(OUT[name + '.amps_floor'])))


def main():
    case('finch_int16', n_knots=4, subset=[3, 0, 2])
    case('finch_float32', n_knots=5, subset=[2, 1])
    fit_inputs('fit_int16', 'finch_int16', 'finch_int16')
    fit_inputs('fit_float32', 'finch_float32', 'finch_float32')
    fit_inputs('fit_band256', 'finch_int16', 'band_256')
    OUT['case_names.json'] = np.array(json.dumps(['finch_int16', 'finch_float32']))
    OUT['fit_names.json'] = np.array(json.dumps(['fit_int16', 'fit_float32', 'fit_band256']))
    path = os.path.join(HERE, "warped.npz")
    np.savez_compressed(path, **OUT)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
