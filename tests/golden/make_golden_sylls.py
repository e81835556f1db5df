"""Writes tests/golden/sylls.npz: the reference's ``process_sylls`` and ``get_syll_specs``
(ava/preprocessing/preprocess.py) and ``get_syllable_partition`` (ava/models/vae_dataset.py) on the synthetic recordings
and segment files of tests/sylls_cases.py.  Needs the reference package, scipy, torch and matplotlib; run from the repository
root as ``python tests/golden/make_golden_sylls.py /path/to/reference``.  The tests only read the npz.

The reference's own ``get_spec`` cannot run on a SciPy without ``interp2d``; ``p['get_spec']`` is a caller-supplied
parameter of the reference, and ``oracle.spec_oracle.get_spec`` (the statement-by-statement restatement the other
goldens live with) is handed in, wrapped in a recorder.  h5py is not needed: a stub module stands in whose
``File(...).create_dataset`` keeps what the reference writes.

Recorded per parameter set and directory (keys ``<set>.<dir>.``), all from the reference's own functions:
  ``pairs.json``                what ``get_audio_seg_filenames`` returns
  ``written.json``              the names of the files ``process_sylls`` wrote, in order
  ``specs`` / ``onsets`` / ``offsets`` / ``audio_filenames``   their four datasets, concatenated in that order
                                (``stop`` stores no ``specs``: the generator asserts they are those of ``lin``)
  ``calls_t1`` / ``calls_t2`` / ``calls_fn.json``   every ``get_spec`` call in order, and the file it was made for
  ``warnings.json``             the ``max_dur`` warnings, in order
and once: ``gss.*`` (``get_syll_specs`` called directly), ``partition.json`` (``get_syllable_partition`` on a directory
tree of empty files for ``split`` in 1.0, 0.8, 0.5 with and without ``max_num_files``), ``spec_tol`` =
max(4 |spec - spec of the float64-cast audio|_max, 4 fp32 ulp of 1), the rule of make_golden_refine.py.
The spectrograms are float64 and stored as float64: those of float32 audio are no float32 values.
"""
import json
import os
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AVA_REFERENCE", "../reference"))

WRITTEN = []                       # (file name, {dataset: array}) in the order the reference wrote them


class _File:
    def __init__(self, name, mode):
        assert mode == "w"
        self.data = {}
        WRITTEN.append((name, self.data))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def create_dataset(self, key, data):
        self.data[key] = np.array(data)


h5py = types.ModuleType("h5py")
h5py.File = _File
sys.modules["h5py"] = h5py
# ava.models.utils imports affinewarp at load time; nothing driven here calls it (as in make_golden_warped.py)
for _m in ("affinewarp", "affinewarp.crossval"):
    sys.modules[_m] = types.ModuleType(_m)
sys.modules["affinewarp"].PiecewiseWarping = object
sys.modules["affinewarp.crossval"].paramsearch = None

import sylls_cases as SC                                    # noqa: E402
from oracle import spec_oracle as SO                        # noqa: E402
import ava.preprocessing.preprocess as P                    # noqa: E402
import ava.models.vae_dataset as VD                         # noqa: E402

OUT = {}
CALLS = []                          # (audio file, t1, t2)
CURRENT = [None]
GAP = [0.0]


def recording_get_spec(t1, t2, audio, p, fs=32000, target_freqs=None, **kwargs):
    CALLS.append((CURRENT[0], float(t1), float(t2)))
    spec, flag = SO.get_spec(t1, t2, audio, p, fs, target_freqs=target_freqs, **kwargs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        other, _ = SO.get_spec(t1, t2, audio.astype(np.float64), p, fs, target_freqs=target_freqs, **kwargs)
    GAP[0] = max(GAP[0], float(np.abs(spec - other).max()))
    return spec, flag


_real_get_syll_specs = P.get_syll_specs


def noting_get_syll_specs(onsets, offsets, audio_filename, p):
    CURRENT[0] = str(audio_filename)
    return _real_get_syll_specs(onsets, offsets, audio_filename, p)


P.get_syll_specs = noting_get_syll_specs


def run(name, d, audio_dir, seg_dir):
    p = SC.params(name)
    p['get_spec'] = recording_get_spec
    del WRITTEN[:], CALLS[:]
    key = "%s.%d." % (name, d)
    OUT[key + "pairs.json"] = np.array(json.dumps(P.get_audio_seg_filenames(audio_dir, seg_dir, p)))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        P.process_sylls(audio_dir, seg_dir, "save_%s_%d" % (name, d), p, shuffle=True, verbose=False)
    msgs = [str(w.message) for w in caught if str(w.message).startswith("Found segment longer")]
    OUT[key + "warnings.json"] = np.array(json.dumps(msgs))
    OUT[key + "written.json"] = np.array(json.dumps([os.path.basename(fn) for fn, _ in WRITTEN]))
    OUT[key + "calls_t1"] = np.array([c[1] for c in CALLS], dtype=np.float64)
    OUT[key + "calls_t2"] = np.array([c[2] for c in CALLS], dtype=np.float64)
    OUT[key + "calls_fn.json"] = np.array(json.dumps([c[0] for c in CALLS]))
    F, T = p['num_freq_bins'], p['num_time_bins']
    specs = np.concatenate([w['specs'] for _, w in WRITTEN] + [np.zeros((0, F, T))])
    assert specs.dtype == np.float64 and all(len(w['specs']) == p['sylls_per_file'] for _, w in WRITTEN)
    if name == "stop":
        assert np.array_equal(specs, OUT["lin.%d.specs" % d][:len(specs)])
    else:
        OUT[key + "specs"] = specs
    OUT[key + "onsets"] = np.concatenate([w['onsets'] for _, w in WRITTEN] + [np.zeros(0)])
    OUT[key + "offsets"] = np.concatenate([w['offsets'] for _, w in WRITTEN] + [np.zeros(0)])
    OUT[key + "audio_filenames"] = np.concatenate([w['audio_filenames'] for _, w in WRITTEN] + [np.zeros(0, 'S1')])
    print("%-9s dir %d: %d get_spec calls, %d files written, %d warnings, zero specs %d" % (
        name, d, len(CALLS), len(WRITTEN), len(msgs), int((specs.reshape(len(specs), -1).max(1) == 0).sum())))
    return specs


def partitions():
    """get_syllable_partition on empty files; the names are recorded with the suffix the reference looks for"""
    os.makedirs("part_0")
    os.makedirs("part_1")
    for k in range(4):
        open(os.path.join("part_0", "syllables_%04d.hdf5" % k), "w").close()
    for k in range(3):
        open(os.path.join("part_1", "syllables_%04d.hdf5" % k), "w").close()
    open(os.path.join("part_1", "notes.txt"), "w").close()
    out = {}
    for split in (1.0, 0.8, 0.5):
        for max_num_files in (None, 5):
            part = VD.get_syllable_partition(["part_0", "part_1"], split, max_num_files=max_num_files)
            out["%s|%s" % (split, max_num_files)] = part
    out["0.5|None|noshuffle"] = VD.get_syllable_partition(["part_0", "part_1"], 0.5, shuffle=False)
    OUT["partition.json"] = np.array(json.dumps(out))


def main():
    root = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(root)
    try:
        audio_dirs, seg_dirs = SC.write_dirs(root)
        for name, (_, dirs) in SC.SYLL_SETS.items():
            for d in dirs:
                specs = run(name, d, audio_dirs[d], seg_dirs[d])
                if name == "lin" and d == 0:
                    assert (specs.reshape(len(specs), -1).max(1) == 0).sum() == 1 and specs.max() > 0.5
        # the stopped run: s0_c is never asked for
        fns = json.loads(str(OUT["stop.0.calls_fn.json"]))
        assert len(fns) == 9 and not any("s0_c" in f for f in fns) and len(json.loads(str(OUT["stop.0.written.json"]))) == 2
        assert len(json.loads(str(OUT["lin.0.calls_fn.json"]))) == 11
        # get_syll_specs, called directly
        p = SC.params("mel_ts")
        p['get_spec'] = recording_get_spec
        segs = np.array(SC.SYLL_DIRS[0][0][1])
        specs, valid = _real_get_syll_specs(segs[:, 0], segs[:, 1], os.path.join(audio_dirs[0], "s0_a.wav"), p)
        OUT["gss.specs"] = np.stack(specs)
        OUT["gss.valid"] = np.array(valid, dtype=np.int64)
        partitions()
    finally:
        os.chdir(cwd)
        shutil.rmtree(root)
    OUT["spec_tol"] = np.array(max(4.0 * GAP[0], 4.0 * float(np.spacing(np.float32(1.0)))))
    path = os.path.join(HERE, "sylls.npz")
    np.savez_compressed(path, **OUT)
    print("wrote", path, os.path.getsize(path), "bytes; gap %.3g spec_tol %.3g" % (GAP[0], float(OUT["spec_tol"])))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
