"""Recordings, segment files and parameter sets for the syllable path (ava_amd.preprocess, ava_amd.syllable_dataset).

The recordings come from ava_amd.synthetic's hash streams, so tests/golden/sylls.npz (written by
tests/golden/make_golden_sylls.py) holds results only.  Two directories of three recordings each:

  directory 0  int16.  ``s0_a``: a segment shorter than ``nperseg`` (all-zero spectrogram) and one that runs past the
               end of the file; ``s0_b``: a segment longer than ``max_dur`` (warning); ``s0_c``: two segments.
               5 + 4 + 2 = 11 syllables: two groups of four, three dropped.  With ``max_num_syllables = 8`` the loop stops
               after ``s0_b`` and never reads ``s0_c``.
  directory 1  float32 (the int16 scale, so one ``spec_min_val`` serves both).  ``s1_a`` has no segment file (dropped),
               ``s1_c`` an empty one; the seed-42 order of the two remaining pairs is ``s1_c``, ``s1_b``.
               6 syllables: one group of four, two dropped.
"""
import os

import numpy as np

from ava_amd import synthetic as syn

FS = 32000
SECONDS = 1.2

# per directory: (name, (onset, offset) lines of its segment file or None for no file)
SYLL_DIRS = [
    [("s0_a", [(0.290, 0.450), (0.560, 0.570), (0.600, 0.800), (0.900, 1.100), (1.100, 1.300)]),
     ("s0_b", [(0.200, 0.620), (0.470, 0.600), (0.810, 0.950), (1.000, 1.100)]),
     ("s0_c", [(0.150, 0.300), (0.520, 0.700)])],
    [("s1_a", None),
     ("s1_b", [(0.050, 0.200), (0.240, 0.400), (0.460, 0.610), (0.800, 0.990), (1.000, 1.150), (1.200, 1.350)]),
     ("s1_c", [])],
]
SYLL_DTYPES = [np.int16, np.float32]

_BASE = dict(fs=FS, nperseg=512, noverlap=256, min_freq=400, max_freq=10e3, spec_min_val=2.0, spec_max_val=6.5,
             max_dur=0.3, sylls_per_file=4, max_num_syllables=None, within_syll_normalize=False,
             normalize_quantile=0.5, num_freq_bins=32, num_time_bins=24, mel=False, time_stretch=False)

# name -> (overrides of _BASE, directories the set runs on)
SYLL_SETS = {
    "train128": (dict(num_freq_bins=128, num_time_bins=128, mel=True, time_stretch=True), [1]),
    "lin": (dict(), [0, 1]),
    "mel_ts": (dict(mel=True, time_stretch=True), [0, 1]),
    "norm": (dict(time_stretch=True, within_syll_normalize=True), [0, 1]),
    "stop": (dict(max_num_syllables=8), [0, 1]),
}


def params(name):
    return dict(_BASE, **SYLL_SETS[name][0])


def audio_of(d):
    """the three recordings of directory ``d``"""
    _, songs, _ = syn.songs(n_exemplars=1, n_songs=3, fs=FS, seconds=SECONDS, motif_seconds=0.25, renditions=3,
                            salt=6111 + 50 * d, dtype=SYLL_DTYPES[d])
    if SYLL_DTYPES[d] == np.float32:
        songs = [s * np.float32(32768.0) for s in songs]          # exact: a power of two
    return songs


def write_dirs(root):
    """writes the recordings and segment files under ``root``: (audio_dirs, seg_dirs), relative to ``root`` (the
    stored ``audio_filenames`` hold the paths as given, so callers work from inside ``root``)"""
    from scipy.io import wavfile
    audio_dirs, seg_dirs = [], []
    for d, files in enumerate(SYLL_DIRS):
        ad, sd = os.path.join(root, "audio_%d" % d), os.path.join(root, "segs_%d" % d)
        os.makedirs(ad)
        os.makedirs(sd)
        for (name, segs), audio in zip(files, audio_of(d)):
            wavfile.write(os.path.join(ad, name + ".wav"), FS, audio)
            if segs is not None:
                np.savetxt(os.path.join(sd, name + ".txt"), np.array(segs).reshape(-1, 2), fmt='%.5f',
                           header="Onsets/offsets for " + name + ".wav")
        audio_dirs.append("audio_%d" % d)
        seg_dirs.append("segs_%d" % d)
    return audio_dirs, seg_dirs
