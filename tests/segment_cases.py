"""Cases of tests/golden/segment.npz (written by tests/golden/make_golden_segment.py): the audio of every case is
regenerated from ``ava_amd.synthetic`` by the recipe stored with it, so that the fixture holds only results."""
import json

import numpy as np

from conftest import load_golden

LOG_INT16_SCALE = float(np.log(32768.0))   # syn.recordings divides float audio by 32768: spectra are that much lower
BASE = dict(min_dur=0.03, max_dur=0.3, smoothing_timescale=0.007, temperature=0.5)
MOUSE = dict(BASE, fs=250000, nperseg=1024, noverlap=512, min_freq=30e3, max_freq=110e3, spec_min_val=2.0,
             spec_max_val=6.0)
FINCH = dict(BASE, fs=32000, nperseg=512, noverlap=256, min_freq=400, max_freq=10e3, spec_min_val=2.0, spec_max_val=6.0)


def audio_of(recipe):
    """the recordings a case segments"""
    from ava_amd import synthetic as syn
    dtype = np.dtype(recipe['dtype'])
    if recipe['kind'] == 'rec':
        audio, _ = syn.recordings(n_files=recipe['n_files'], fs=recipe['fs'], seconds=recipe['seconds'], dtype=dtype)
        return audio
    src, _ = syn.recordings(n_files=1, fs=recipe['fs'], seconds=1.0, dtype=dtype)
    out = []
    for n in recipe['lengths']:
        out.append(np.zeros(-n, dtype=dtype) if n < 0 else src[0][:n].copy())   # negative length: that many zeros
    return out


def load():
    """(cases, hand): dicts name -> entry, parameters and recipes decoded"""
    g = load_golden("segment.npz")
    cases, hand = {}, {}
    for name in json.loads(str(g['case_names'])):
        c = {k.split('/', 1)[1]: v for k, v in g.items() if k.startswith(name + '/')}
        c['p'] = json.loads(str(c['p']))
        c['recipe'] = json.loads(str(c['recipe']))
        cases[name] = c
    for name in json.loads(str(g['hand_names'])):
        c = {k.split('/', 1)[1]: v for k, v in g.items() if k.startswith(name + '/')}
        c['p'] = json.loads(str(c['p']))
        hand[name] = c
    return cases, hand
