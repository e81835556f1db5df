"""Syllable spectrograms made on the device.

Mirror of the reference's ``ava/preprocessing/preprocess.py`` without its interactive tuners:

  ``get_audio_seg_filenames``, ``get_audio_filenames``, ``read_onsets_offsets_from_file``, ``is_audio_file``
                           :313-367, the reference's rules restated
  ``get_syll_specs``       :108-150, one ``spec.get_spec_batch`` over the file's syllables instead of one
                           ``p['get_spec']`` call per syllable
  ``process_sylls``        :23-105, same files visited, same groups written, same prints
  ``syllables_to_device``  the same rows as ``process_sylls`` writes, kept in HBM as a ``SyllableStore``

The audio of a directory is uploaded once (``spec.DeviceAudio``); its syllables go through ``get_spec_batch`` in chunks
whose workspace (``ava_spec_workspace_bytes`` of the chunk's own longest segment) stays below ``max_workspace_bytes``,
straight into the fp32 ``[N, F, T]`` tensor ``syllable_dataset.DeviceSyllableDataset`` serves batches from.  The result
does not depend on the chunking.

DEVIATION: ``process_sylls`` writes ``syllables_0000.npz`` (``numpy.savez``) where the reference writes
``syllables_0000.hdf5``; this package does not depend on h5py.  The four datasets (``specs``, ``onsets``, ``offsets``,
``audio_filenames``) have the reference's names, dtypes and shapes.  ``p['get_spec']`` is not consulted: the
spectrograms are ``spec.get_spec``'s.

There is no CPU fallback.
"""
import os
import warnings

import numpy as np
import torch

from . import _lib
from .spec import DeviceAudio, _check_stft_shape, _quantile_index, _read_wav, get_spec_batch, target_freqs_of

__all__ = ["SyllableStore", "get_audio_seg_filenames", "get_audio_filenames", "read_onsets_offsets_from_file",
           "is_audio_file", "get_syll_specs", "process_sylls", "syllables_to_device", "plan_groups", "plan_directory",
           "iter_groups", "group_filename", "install"]

DEFAULT_WORKSPACE_BYTES = 1 << 28        # get_spec_batch scratch per chunk of syllables


# ---- file names and segment files (the reference's rules) ------------------------------------------------------------
def is_audio_file(fn):
    """preprocess.py:365-367 (a file named ``.wav`` is one)"""
    return len(fn) >= 4 and fn[-4:] == '.wav'


def get_audio_filenames(audio_dir):
    """preprocess.py:329-333: the sorted audio files of a directory"""
    return [os.path.join(audio_dir, i) for i in sorted(os.listdir(audio_dir)) if is_audio_file(i)]


def get_audio_seg_filenames(audio_dir, segment_dir, p):
    """preprocess.py:313-326: sorted (audio, segment) file names; a pair whose segment file is missing is dropped"""
    temp_filenames = [i for i in sorted(os.listdir(audio_dir)) if is_audio_file(i)]
    audio_filenames = [os.path.join(audio_dir, i) for i in temp_filenames]
    seg_filenames = [os.path.join(segment_dir, i[:-4] + '.txt') for i in temp_filenames]
    for i in range(len(seg_filenames) - 1, -1, -1):
        if not os.path.exists(seg_filenames[i]):
            del seg_filenames[i]
            del audio_filenames[i]
    return audio_filenames, seg_filenames


def read_onsets_offsets_from_file(txt_filename, p):
    """preprocess.py:336-348: two whitespace-separated columns, ``#`` before header and footer lines"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)              # numpy's "input contained no data"
        segs = np.loadtxt(txt_filename)
    assert segs.size % 2 == 0, "Incorrect formatting: " + txt_filename
    segs = segs.reshape(-1, 2)
    return segs[:, 0], segs[:, 1]


# ---- grouping (host arithmetic only) ---------------------------------------------------------------------------------
def group_filename(num):
    return "syllables_" + str(num).zfill(4) + '.npz'


def plan_groups(counts, sylls_per_file, max_num_syllables=None):
    """The write loop of ``process_sylls`` (preprocess.py:64-103) on syllable counts alone.  ``counts[i]`` syllables come
    from the i-th visited file; after every file full groups of ``sylls_per_file`` are written, and the function returns
    as soon as ``groups * sylls_per_file >= max_num_syllables``.  Returns ``(files_visited, groups, stopped)``: the rows
    written are the first ``groups * sylls_per_file`` syllables of the first ``files_visited`` files; the rest of those
    files' syllables, the final partial group, is dropped."""
    have, groups = 0, 0
    for k, c in enumerate(counts):
        have += int(c)
        while have >= sylls_per_file:
            groups += 1
            have -= sylls_per_file
            if max_num_syllables is not None and groups * sylls_per_file >= max_num_syllables:
                return k + 1, groups, True
    return len(counts), groups, False


def plan_directory(audio_dir, segment_dir, p, shuffle=True):
    """The host half of ``process_sylls`` for one directory: which files it visits in which order and what it asks of
    ``get_spec``.  Returns a dict: ``audio_filenames`` / ``seg_filenames`` (the visited pairs, in the seed-42 order
    with ``shuffle``), ``onsets`` / ``offsets`` (one array per visited file: the ``t1``, ``t2`` of every ``get_spec``
    call, in order), ``groups`` and ``stopped`` (``plan_groups``).  Files behind the ``max_num_syllables`` stop are not
    read, as in the reference."""
    audio_filenames, seg_filenames = get_audio_seg_filenames(audio_dir, segment_dir, p)
    if shuffle:
        np.random.seed(42)
        perm = np.random.permutation(len(audio_filenames))
        np.random.seed(None)
        audio_filenames = np.array(audio_filenames)[perm]
        seg_filenames = np.array(seg_filenames)[perm]
    sylls_per_file, max_num = p['sylls_per_file'], p['max_num_syllables']
    plan = dict(audio_filenames=[], seg_filenames=[], onsets=[], offsets=[], groups=0, stopped=False)
    counts = []
    for audio_filename, seg_filename in zip(audio_filenames, seg_filenames):
        onsets, offsets = read_onsets_offsets_from_file(seg_filename, p)
        plan['audio_filenames'].append(str(audio_filename))
        plan['seg_filenames'].append(str(seg_filename))
        plan['onsets'].append(onsets)
        plan['offsets'].append(offsets)
        counts.append(len(onsets))
        _, plan['groups'], plan['stopped'] = plan_groups(counts, sylls_per_file, max_num)
        if plan['stopped']:
            break
    return plan


def iter_groups(specs, onsets, offsets, audio_filenames, sylls_per_file):
    """Cut accumulated syllables into the datasets of the files ``process_sylls`` writes (preprocess.py:78-96): yields
    one dict per full group of ``sylls_per_file`` rows with ``specs`` float64 ``[n, F, T]``, ``onsets``, ``offsets`` and
    ``audio_filenames`` (bytes); a final partial group is dropped.  ``specs`` may be any ``[N, F, T]`` array."""
    for g in range(len(onsets) // sylls_per_file):
        rows = slice(g * sylls_per_file, (g + 1) * sylls_per_file)
        yield dict(specs=np.asarray(specs[rows], dtype=np.float64), onsets=np.array(onsets[rows]),
                   offsets=np.array(offsets[rows]), audio_filenames=np.array(audio_filenames[rows]).astype('S'))


# ---- spectrograms ---------------------------------------------------------------------------------------------------------
def _target_times(t1, t2, p):
    """the default ``target_times`` of ``get_spec`` (utils.py:89-95) for every syllable: ``[n, T]``"""
    max_dur = p['max_dur']
    duration = t2 - t1
    if p['time_stretch']:
        duration = np.sqrt(duration * max_dur)
    shoulder = 0.5 * (max_dur - duration)
    lo, hi = t1 - shoulder, t2 + shoulder
    if (lo == hi).any():                      # numpy takes another path for a zero step, and takes it for all rows
        return np.stack([np.linspace(a, b, p['num_time_bins']) for a, b in zip(lo, hi)])
    return np.linspace(lo, hi, p['num_time_bins'], axis=-1)


def _check_syllables(t1, t2, fs, p):
    """the per-syllable warning and assertion of ``get_spec`` (utils.py:54-61), in its order"""
    max_dur = p['max_dur']
    for a, b in zip(t1, t2):
        if b - a > max_dur + 1e-4:
            warnings.warn("Found segment longer than max_dur: " + str(b - a) + "s, max_dur = " + str(max_dur) + "s")
        s1, s2 = int(round(a * fs)), int(round(b * fs))
        assert s1 < s2, "s1: " + str(s1) + " s2: " + str(s2) + " t1: " + str(a) + " t2: " + str(b)


def _chunk_bounds(n_samples, p, max_workspace_bytes):
    """``[(lo, hi), ...]``: consecutive syllables whose ``get_spec_batch`` workspace, sized by the chunk's own longest
    segment, stays within ``max_workspace_bytes`` (a syllable that needs more is a chunk of its own)"""
    nperseg, noverlap = _check_stft_shape(p, p['num_time_bins'])
    F, T = p['num_freq_bins'], p['num_time_bins']
    normalize = _quantile_index(p, F, T)[0]
    need = _lib.load().ava_spec_workspace_bytes
    bounds, lo, longest = [], 0, 0
    for i, m in enumerate(n_samples):
        m = int(m)
        if i > lo and need(i - lo + 1, max(longest, m), nperseg, noverlap, F, T, normalize) > max_workspace_bytes:
            bounds.append((lo, i))
            lo, longest = i, 0
        longest = max(longest, m)
    if len(n_samples) > lo:
        bounds.append((lo, len(n_samples)))
    return bounds


def _specs_into(out, audio, file_idx, t1, t2, fs, p, target_freqs, max_workspace_bytes):
    """``out[i] = get_spec(t1[i], t2[i], recording file_idx[i])`` for all i, chunk by chunk on the current stream"""
    n_samples = np.rint(t2 * fs) - np.rint(t1 * fs)
    tt = _target_times(t1, t2, p)
    for lo, hi in _chunk_bounds(n_samples, p, max_workspace_bytes):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)          # the batch's one warning: given per syllable above
            out[lo:hi] = get_spec_batch(audio, file_idx[lo:hi], t1[lo:hi], t2[lo:hi], p, fs, tt[lo:hi],
                                        target_freqs=target_freqs)


def get_syll_specs(onsets, offsets, audio_filename, p, device="cuda", max_workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """Mirror of preprocess.py:108-150: ``(specs, valid_syllables)``, a list of ``[F, T]`` float64 arrays (holding the
    fp32 values the device produced) and the indices of the syllables they belong to (all of them: ``get_spec`` calls
    every segment valid).  The file's syllables go through ``get_spec_batch`` together, in several batches when their
    workspace would exceed ``max_workspace_bytes``."""
    fs, audio = _read_wav(audio_filename)
    assert p['nperseg'] % 2 == 0 and p['nperseg'] > 2
    t1 = np.asarray(onsets, dtype=np.float64).reshape(-1)
    t2 = np.asarray(offsets, dtype=np.float64).reshape(-1)
    _check_syllables(t1, t2, fs, p)
    if len(t1) == 0:
        return [], []
    dev_audio = DeviceAudio([audio], device)
    out = torch.empty((len(t1), p['num_freq_bins'], p['num_time_bins']), dtype=torch.float32, device=dev_audio.device)
    _specs_into(out, dev_audio, np.zeros(len(t1), dtype=np.int32), t1, t2, fs, p, target_freqs_of(p),
                max_workspace_bytes)
    return list(out.cpu().numpy().astype(np.float64)), list(range(len(t1)))


class SyllableStore:
    """The syllables of one or more directories in HBM: ``specs`` fp32 device tensor ``[N, F, T]``; host arrays
    ``onsets``, ``offsets`` (float64 ``[N]``), ``audio_filenames`` (bytes ``[N]``: ``join(audio_dir, basename)``, what
    the reference stores) and ``group_of`` (int64 ``[N]``: which of the store's groups, i.e. which ``.npz`` file of
    ``process_sylls``, the row belongs to; groups are numbered through all directories in order).  Per group:
    ``group_dir`` (index of its directory) and ``group_num`` (its file number within that directory).  ``stopped``
    holds per directory whether the ``max_num_syllables`` rule ended it."""

    def __init__(self, specs, onsets, offsets, audio_filenames, group_of, group_dir, group_num, stopped):
        self.specs = specs
        self.onsets = onsets
        self.offsets = offsets
        self.audio_filenames = audio_filenames
        self.group_of = group_of
        self.group_dir = group_dir
        self.group_num = group_num
        self.stopped = stopped

    def __len__(self):
        return int(self.specs.shape[0])

    @property
    def num_groups(self):
        return len(self.group_dir)

    def group_names(self, save_dirs=None):
        """the ``.npz`` name of every group: under ``save_dirs[d]`` for directory d, by default under ``'%04d' % d``"""
        return [os.path.join(save_dirs[d] if save_dirs is not None else "%04d" % d, group_filename(g))
                for d, g in zip(self.group_dir, self.group_num)]


def syllables_to_device(audio_dirs, segment_dirs, p, shuffle=True, device="cuda",
                        max_workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """The rows ``process_sylls`` would write for ``audio_dirs`` / ``segment_dirs`` (one directory after the other, each
    with its own ``max_num_syllables`` stop and its own dropped remainder), as a ``SyllableStore``.  Nothing goes through
    the host or the disk: every directory's visited recordings are uploaded once, their syllables are computed in chunks
    bounded by ``max_workspace_bytes`` of scratch, and only the rows of full groups are kept."""
    assert len(audio_dirs) == len(segment_dirs), f"{len(audio_dirs)} != {len(segment_dirs)}"
    assert p['nperseg'] % 2 == 0 and p['nperseg'] > 2
    dev = torch.device(device)
    F, T = p['num_freq_bins'], p['num_time_bins']
    target_freqs = target_freqs_of(p)
    spf = p['sylls_per_file']
    parts, onsets, offsets, fns, group_of, group_dir, group_num, stopped = [], [], [], [], [], [], [], []
    for d, (audio_dir, segment_dir) in enumerate(zip(audio_dirs, segment_dirs)):
        plan = plan_directory(audio_dir, segment_dir, p, shuffle)
        stopped.append(plan['stopped'])
        wavs = [_read_wav(fn) for fn in plan['audio_filenames']]
        t1 = np.concatenate(plan['onsets'] + [np.zeros(0)])
        t2 = np.concatenate(plan['offsets'] + [np.zeros(0)])
        file_idx = np.concatenate([np.full(len(o), k, dtype=np.int32) for k, o in enumerate(plan['onsets'])] +
                                  [np.zeros(0, dtype=np.int32)])
        rates = np.array([wavs[k][0] for k in file_idx], dtype=np.float64)
        for k, (fs, _) in enumerate(wavs):                            # get_spec's checks, file by file as it is called
            _check_syllables(plan['onsets'][k], plan['offsets'][k], fs, p)
        keep = plan['groups'] * spf
        if keep == 0:
            continue
        # rows behind the last full group are dropped by the reference after it has computed them; here they are not made
        t1, t2, file_idx, rates = t1[:keep], t2[:keep], file_idx[:keep], rates[:keep]
        audio = DeviceAudio([a for _, a in wavs], dev)
        out = torch.empty((keep, F, T), dtype=torch.float32, device=dev)
        cuts = [0] + [i for i in range(1, keep) if rates[i] != rates[i - 1]] + [keep]     # one sampling rate per batch
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            _specs_into(out[lo:hi], audio, file_idx[lo:hi], t1[lo:hi], t2[lo:hi], rates[lo], p, target_freqs,
                        max_workspace_bytes)
        parts.append(out)
        onsets.append(t1)
        offsets.append(t2)
        fns += [os.path.join(audio_dir, os.path.split(plan['audio_filenames'][k])[-1]) for k in file_idx]
        first = len(group_dir)
        group_of.append(first + np.arange(keep, dtype=np.int64) // spf)
        group_dir += [d] * plan['groups']
        group_num += list(range(plan['groups']))
    if parts:
        specs = parts[0] if len(parts) == 1 else torch.cat(parts)
    else:
        specs = torch.empty((0, F, T), dtype=torch.float32, device=dev)
    return SyllableStore(specs, np.concatenate(onsets + [np.zeros(0)]), np.concatenate(offsets + [np.zeros(0)]),
                         np.array(fns).astype('S'), np.concatenate(group_of + [np.zeros(0, dtype=np.int64)]),
                         np.array(group_dir, dtype=np.int64), np.array(group_num, dtype=np.int64), stopped)


def process_sylls(audio_dir, segment_dir, save_dir, p, shuffle=True, verbose=True, device="cuda"):
    """Mirror of preprocess.py:23-105 (same arguments): extract the syllables of ``audio_dir`` and save them to
    ``save_dir`` in files of ``p['sylls_per_file']``.  Same seed-42 file order, same accumulation across files, same
    dropped final partial group, same ``max_num_syllables`` stop, same prints.  It is ``syllables_to_device`` of the one
    directory followed by the writes.  DEVIATION: the files are ``syllables_0000.npz`` written by ``numpy.savez``, not
    ``.hdf5``; the datasets ``specs`` (float64), ``onsets``, ``offsets`` and ``audio_filenames`` (bytes) are the
    reference's."""
    if verbose:
        print("Processing audio files in", audio_dir)
    if not os.path.exists(save_dir):
        os.makedirs(save_dir)
    store = syllables_to_device([audio_dir], [segment_dir], p, shuffle=shuffle, device=device)
    groups = iter_groups(store.specs.cpu().numpy(), store.onsets, store.offsets, store.audio_filenames,
                         p['sylls_per_file'])
    for num, data in enumerate(groups):
        np.savez(os.path.join(save_dir, group_filename(num)), **data)
    if store.stopped[0]:
        if verbose:
            print("\tSaved max_num_syllables (" + str(p['max_num_syllables']) + "). Returning.")
        return
    if verbose:
        print("\tDone.")


def install(module=None):
    """Point ``process_sylls``, ``get_syll_specs`` and the file-name helpers of ``module`` (by default
    ``ava.preprocessing.preprocess``; the reference module imports h5py at import time, so a module object may be
    passed instead) at this module.  ``process_sylls`` then writes ``.npz`` files."""
    if module is None:
        import ava.preprocessing.preprocess as module
    for name in ("process_sylls", "get_syll_specs", "get_audio_seg_filenames", "get_audio_filenames",
                 "read_onsets_offsets_from_file", "is_audio_file"):
        setattr(module, name, globals()[name])
    return module
