"""Cases of tests/golden/warped.npz (written by tests/golden/make_golden_warped.py): the motif files of every case are
regenerated from ``ava_amd.synthetic.songs`` exemplars by the recipe stored with it, so that the fixture holds only
results.  Also the knots the golden script saved and loaded, and a numpy restatement of the reference's
``_get_specs_and_amplitude_traces`` (ava/models/utils.py:337-418) in fp64."""
import json

import numpy as np

from ava_amd import synthetic as syn

LOG_INT16_SCALE = float(np.log(32768.0))   # float audio is the samples / 32768: spectra are that much lower
EPSILON = 1e-9                             # ava/models/utils.py
SAMPLES = 4000                             # hashed entries of ``specs`` kept per case


def params(name):
    """the numeric parameter sets of the cases ('get_spec' is added by the caller)"""
    finch = dict(syn.FINCH_PARAMS)
    if name == 'finch_int16':
        return finch
    if name == 'finch_float32':
        return dict(finch, spec_min_val=finch['spec_min_val'] - LOG_INT16_SCALE,
                    spec_max_val=finch['spec_max_val'] - LOG_INT16_SCALE)
    if name == 'band_256':                 # second parameter set of the fit inputs
        return dict(finch, nperseg=256, noverlap=128, min_freq=1000, max_freq=8e3, spec_min_val=1.5, spec_max_val=6.0)
    raise KeyError(name)


RECIPES = {
    'finch_int16': dict(n_files=5, fs=32000, motif_seconds=0.5, salt=9009, dtype='int16'),
    'finch_float32': dict(n_files=4, fs=32000, motif_seconds=0.4, salt=9109, dtype='float32'),
}


def motifs(recipe):
    """the motif files of a case: one rendition each, of unequal lengths"""
    ex, _, _ = syn.songs(n_exemplars=recipe['n_files'], n_songs=0, fs=recipe['fs'], seconds=1.0,
                         motif_seconds=recipe['motif_seconds'], salt=recipe['salt'], dtype=np.dtype(recipe['dtype']))
    return [a[:len(a) - 37 * i].copy() for i, a in enumerate(ex)]


def names(n):
    """file names of a case; written in an order that is not the sorted one"""
    return ["motif_%02d.wav" % ((7 * i + 3) % n) for i in range(n)]


def knots(n_files, n_knots, salt):
    """monotone piecewise-linear warps: ``(x_knots, y_knots)`` [n_files, n_knots], both running from 0 to 1"""
    u = syn.u01(2 * n_files * n_knots, salt).reshape(2, n_files, n_knots)
    out = []
    for k in range(2):
        steps = 0.25 + u[k]                                     # strictly positive increments
        c = np.cumsum(steps, axis=1)
        out.append((c - c[:, :1]) / (c[:, -1:] - c[:, :1]))
    return out[0], out[1]


def stft_fp64(x, nperseg, noverlap, longdouble_products=False):
    """scipy.signal.stft(x, nperseg=, noverlap=)'s frames (hann, zero boundary, padded, 'spectrum' scaling, no detrend)
    in fp64: [frames, nperseg // 2 + 1] complex"""
    from scipy.signal import get_window
    nstep = nperseg - noverlap
    win = get_window('hann', nperseg)
    x = np.concatenate([np.zeros(nperseg // 2), np.asarray(x, dtype=np.float64), np.zeros(nperseg // 2)])
    nadd = (-(len(x) - nperseg) % nstep) % nperseg
    x = np.concatenate([x, np.zeros(nadd)])
    n_frames = (len(x) - nperseg) // nstep + 1
    idx = np.arange(nperseg)[None, :] + nstep * np.arange(n_frames)[:, None]
    if longdouble_products:
        frames = (x.astype(np.longdouble)[idx] * win.astype(np.longdouble)[None, :]).astype(np.float64)
    else:
        frames = x[idx] * win[None, :]
    return np.fft.rfft(frames, axis=-1) * np.sqrt(1.0 / win.sum() ** 2)


def specs_and_amps(all_audio, fs, p, longdouble_products=False):
    """``_get_specs_and_amplitude_traces`` (ava/models/utils.py:371-418) restated in fp64 numpy"""
    nperseg, noverlap = p['nperseg'], p['noverlap']
    f = np.fft.rfftfreq(nperseg, 1 / fs)
    i1, i2 = np.searchsorted(f, p['min_freq']), np.searchsorted(f, p['max_freq'])
    specs = []
    for a in all_audio:
        spec = stft_fp64(a, nperseg, noverlap, longdouble_products)[:, i1:i2]
        spec = np.log(np.abs(spec) + EPSILON)
        spec -= p['spec_min_val']
        spec /= p['spec_max_val'] - p['spec_min_val'] + EPSILON
        specs.append(np.clip(spec, 0.0, 1.0))
    min_time_bins = min(s.shape[0] for s in specs)
    specs = [s[:min_time_bins] for s in specs]
    time = np.array([nperseg / 2, nperseg / 2 + (nperseg - noverlap)]) / float(fs)
    time -= (nperseg / 2) / fs
    template_dur = min_time_bins * (time[1] - time[0])
    amps = []
    for s in specs:
        amp_trace = np.sum(s, axis=-1, keepdims=True)
        amp_trace -= np.min(amp_trace)
        amp_trace /= np.max(amp_trace) + EPSILON
        amps.append(amp_trace)
    return np.stack(specs), np.stack(amps), template_dur


def spec_samples(numel, salt):
    """the hashed flat indices of ``specs`` the golden keeps"""
    return np.minimum((syn.u01(SAMPLES, 7700 + salt) * numel).astype(np.int64), numel - 1)


def load():
    """the golden as a dict, JSON entries decoded"""
    from conftest import load_golden
    g = load_golden("warped.npz")
    return {k: (json.loads(str(v)) if k.endswith('.json') else v) for k, v in g.items()}
