"""Cases of tests/golden/template.npz (written by tests/golden/make_golden_template.py): the audio of every case is
regenerated from ``ava_amd.synthetic.songs`` by the recipe stored with it, so that the fixture holds only results."""
import json

import numpy as np

from conftest import load_golden

LOG_INT16_SCALE = float(np.log(32768.0))   # float audio is the samples / 32768: spectra are that much lower
FINCH = dict(fs=32000, nperseg=512, noverlap=256, min_freq=400, max_freq=10e3, spec_min_val=2.0, spec_max_val=6.5)


def audio_of(recipe):
    """(exemplars, files) of a case"""
    from ava_amd import synthetic as syn
    dtype = np.dtype(recipe['dtype'])
    ex, songs, _ = syn.songs(n_exemplars=recipe['n_exemplars'], n_songs=recipe['n_songs'], fs=recipe['fs'],
                             seconds=recipe['seconds'], motif_seconds=recipe['motif_seconds'], salt=recipe['salt'],
                             dtype=dtype)
    if recipe['kind'] == 'songs':
        return ex, songs
    files = []
    for n in recipe['lengths']:
        if n == 'loud':                                        # noise loud enough that every bin clips to 1
            x = 20000.0 * syn.gauss(int(recipe['fs'] * recipe['seconds']), recipe['salt'] + 99)
            files.append(np.clip(np.rint(x), -32768, 32767).astype(dtype))
        elif n < 0:                                            # negative length: that many zeros
            files.append(np.zeros(-n, dtype=dtype))
        else:
            files.append(songs[0][:n].copy())
    return ex, files


def _entries(g, name):
    c = {k.split('/', 1)[1]: v for k, v in g.items() if k.startswith(name + '/')}
    for key in ('p', 'tp', 'recipe', 'opts'):
        if key in c:
            c[key] = json.loads(str(c[key]))
    return c


def load():
    """(cases, hand): dicts name -> entry, parameters and recipes decoded"""
    g = load_golden("template.npz")
    cases = {n: _entries(g, n) for n in json.loads(str(g['case_names']))}
    hand = {n: _entries(g, n) for n in json.loads(str(g['hand_names']))}
    return cases, hand
