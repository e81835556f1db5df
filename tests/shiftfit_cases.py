"""The integer-shift fit restated in numpy: the oracle of tests/test_gpu_shiftfit.py, pinned
by tests/test_cpu_shiftfit.py.  The model is this project's own (the docstring of ``ava_amd.shift_fit`` states it), so
it is written out here from its definition: ``lag_order``, the template through ``scipy.linalg.solveh_banded``, the
loss, the argmin and the whole loop.  Also here: the planted recipe of the tests, and a plain numpy statement of what
the two ``segment_sylls_*`` functions of the reference's ``ava/segmenting/template_segmentation.py`` (lines 455-627 and
630-755) do on the host, given shifts, quantiles and a dataset: the oracle of the device module's host halves.

The planted recipe: ``x_k(t) = base(t - sh_k)`` with ``base`` a sum of three Gaussian bumps at ``[0.2, 0.45, 0.75] T``
of widths ``[0.05, 0.07, 0.04] T``, per-row gains ``0.5 + u01(3 F, salt + 1)``, integer ``sh = round((2 u01(K, salt) -
1) max_shift)`` and noise ``0.02 u01(K F T, salt + 2)``; traces (``F = 1``) are z-scored, minus the mean, divided by
``std + 1e-12``.  ``max_shift`` stays at or below ``0.8 L``: closer to ``L`` the clipping of the search bites and the
planted shifts are not recovered."""
import os

import numpy as np
from scipy.linalg import solveh_banded

from ava_amd import synthetic as syn

L2 = 1e-7
MAXLAG, SMOOTHNESS, ITERATIONS = 0.2, 10.0, 12
# (K, F, T, max_shift, salt)
CASES = [(40, 1, 130, 20, 5101), (24, 3, 67, 10, 5102), (7, 5, 37, 6, 5103)]
DTYPES = ['float32', 'float64']


def lag_order(L):
    """0, -1, +1, -2, +2, ..., -L, +L"""
    out = [0]
    for i in range(1, L + 1):
        out += [-i, i]
    return np.array(out, dtype=np.int64)


def second_differences(T):
    """D2: the (T - 2) x T matrix of rows (1, -2, 1), dense"""
    D = np.zeros((T - 2, T))
    for i in range(T - 2):
        D[i, i:i + 3] = [1.0, -2.0, 1.0]
    return D


def banded_A(T, K, lam, l2=L2):
    """A = (1 + l2 / K) I + lam D2^T D2 in the upper banded form of ``solveh_banded``: [3, T]"""
    t = np.arange(T)
    diag = (t <= T - 3) + 4.0 * ((t >= 1) & (t <= T - 2)) + (t >= 2)
    off1 = -2.0 * ((t <= T - 3).astype(float) + ((t >= 1) & (t <= T - 2)))       # A[t, t + 1]
    off2 = (t <= T - 3).astype(float)                                            # A[t, t + 2]
    ab = np.zeros((3, T))
    ab[2] = (1.0 + l2 / K) + lam * diag
    ab[1, 1:] = lam * off1[:-1]
    ab[0, 2:] = lam * off2[:-2]
    return ab


def dense_A(T, K, lam, l2=L2):
    D = second_differences(T)
    return (1.0 + l2 / K) * np.eye(T) + lam * D.T @ D


def aligned(x, shifts):
    """x [K, F, T] read at the columns clip(t + s_k, 0, T - 1)"""
    K, F, T = x.shape
    idx = np.clip(np.arange(T)[None, :] + np.asarray(shifts)[:, None], 0, T - 1)
    return np.take_along_axis(x, np.broadcast_to(idx[:, None, :], x.shape), axis=2)


def template(x, shifts, lam, l2=L2):
    """(m, mbar) [F, T] float64"""
    x = np.asarray(x, dtype=np.float64)
    K, F, T = x.shape
    mbar = aligned(x, shifts).sum(axis=0) / K
    m = solveh_banded(banded_A(T, K, lam, l2), mbar.T).T
    return m, mbar


def loss(x, m, L):
    """[K, 2 L + 1] float64"""
    x = np.asarray(x, dtype=np.float64)
    K, F, T = x.shape
    out = np.empty((K, 2 * L + 1))
    for c, lag in enumerate(lag_order(L)):
        idx = np.clip(np.arange(T) + lag, 0, T - 1)
        d = x[:, :, idx] - m[None]
        out[:, c] = (d * d).sum(axis=(1, 2)) / (F * T)
    return out


def argmin(losses):
    """per row the lowest index of the least value; NaN never wins (all NaN: 0)"""
    return np.where(np.isnan(losses), np.inf, losses).argmin(axis=1)


def objective(x, shifts, m, lam, l2=L2):
    """J = sum_k sum (aligned_k - m)^2 + K lam |D2 m|^2 + l2 |m|^2"""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    d2 = m[:, 2:] - 2.0 * m[:, 1:-1] + m[:, :-2]
    return ((aligned(x, shifts) - m[None]) ** 2).sum() + K * lam * (d2 * d2).sum() + l2 * (m * m).sum()


def fit(x, maxlag, lam, iterations, l2=L2):
    """The whole loop: a dict with ``shifts`` [K] (the last), ``template`` [F, T] (the last), ``J`` (after every
    iteration), ``J_template`` (after every template step, before the shifts move), ``history`` (the shifts after every
    iteration) and ``gap``: the smallest relative gap between the best and the second-best loss of any rendition in any
    iteration (inf when there is a single lag)."""
    x = np.asarray(x, dtype=np.float64)
    K, F, T = x.shape
    L = int(maxlag * T)
    lags = lag_order(L)
    shifts = np.zeros(K, dtype=np.int64)
    out = dict(J=[], J_template=[], history=[], gap=np.inf)
    for _ in range(iterations):
        m, _ = template(x, shifts, lam, l2)
        out['J_template'].append(objective(x, shifts, m, lam, l2))
        ls = loss(x, m, L)
        if ls.shape[1] > 1:
            two = np.sort(ls, axis=1)[:, :2]
            with np.errstate(invalid='ignore', divide='ignore'):
                gaps = (two[:, 1] - two[:, 0]) / np.abs(two[:, 1])
            gaps = gaps[ls.max(axis=1) > ls.min(axis=1)]   # a constant trace ties at every lag: no gap to speak of
            if len(gaps):
                out['gap'] = min(out['gap'], float(gaps.min()))
        shifts = lags[argmin(ls)]
        out['J'].append(objective(x, shifts, m, lam, l2))
        out['history'].append(shifts.copy())
    out.update(shifts=shifts, template=m)
    return out


def planted(K, F, T, max_shift, salt):
    """(x [K, F, T] float64, planted shifts [K])"""
    centres, widths = np.array([0.2, 0.45, 0.75]) * T, np.array([0.05, 0.07, 0.04]) * T
    gains = 0.5 + syn.u01(3 * F, salt + 1).reshape(F, 3)
    sh = np.round((2 * syn.u01(K, salt) - 1) * max_shift).astype(np.int64)
    t = np.arange(T)[None, None, :] - sh[:, None, None]                          # [K, 1, T]
    x = np.zeros((K, F, T))
    for b in range(3):
        x += gains[None, :, b, None] * np.exp(-0.5 * ((t - centres[b]) / widths[b]) ** 2)
    x += 0.02 * syn.u01(K * F * T, salt + 2).reshape(K, F, T)
    if F == 1:
        x -= x.mean(axis=2, keepdims=True)
        x /= x.std(axis=2, keepdims=True) + 1e-12
    return x, sh


# ---- the host halves of the two segmenters, stated plainly --------------------------------------------------------------

def song_slices(song_segs, audio_of, shoulder):
    """What lines 489-512 of the reference ask of the audio: per song segment ``(filename, widened onset, i1, i2, reaches
    outside the file)`` with ``i = int(fs * t)`` (Python's ``int()``); the samples are ``audio[max(i1, 0):i2]``.  And the
    recordings without song.  ``audio_of[filename]`` is ``(fs, samples)``."""
    rows, empty = [], []
    for fn in song_segs:
        fs, audio = audio_of[fn]
        for seg in np.asarray(song_segs[fn]).reshape(-1, 2):
            onset, offset = seg[0] - shoulder, seg[1] + shoulder
            i1, i2 = int(fs * onset), int(fs * offset)
            rows.append((fn, onset, i1, i2, i1 < 0 or i2 > len(audio)))
        if len(song_segs[fn]) == 0:
            empty.append(fn)
    return rows, empty


def edge_bins(i1, i2, n_samples, fs, dt):
    """(pre_bins, post_bins) of lines 500-501"""
    return max(0, int(np.round(-i1 / fs / dt))), max(0, int(np.round((i2 - n_samples) / fs / dt)))


def write_syllable_segments(fns, song_onsets, shifts, quantiles, num_time_bins, dt, audio_dirs, syll_seg_dirs, empty):
    """What lines 593-627 write"""
    duration = num_time_bins * dt
    q = np.sort(np.array(quantiles))
    seen = set()
    for i, (fn, song_onset) in enumerate(zip(fns, song_onsets)):
        onsets = song_onset + duration * q[:-1]
        offsets = song_onset + duration * q[1:]
        onsets += shifts[i] * dt
        offsets += shifts[i] * dt
        out_dir = syll_seg_dirs[audio_dirs.index(os.path.split(fn)[0])]
        os.makedirs(out_dir, exist_ok=True)
        write_fn = os.path.join(out_dir, os.path.split(fn)[-1])[:-4] + '.txt'
        header = "Song onset: " + str(song_onset)
        if fn not in seen:
            seen.add(fn)
            header = "Syllables from song: " + fn + "\n" + header
            mode = 'wb'
        else:
            mode = 'ab'
        with open(write_fn, mode) as f:
            np.savetxt(f, np.stack([onsets, offsets]).reshape(2, -1).T, fmt='%.5f', header=header)
    for fn in empty:
        out_dir = syll_seg_dirs[audio_dirs.index(os.path.split(fn)[0])]
        os.makedirs(out_dir, exist_ok=True)
        np.savetxt(os.path.join(out_dir, os.path.split(fn)[-1])[:-4] + '.txt', np.array([]),
                   header="Syllables from song: " + fn)


def warped_syllables(dset, quantiles):
    """What lines 712-739 collect per recording: ``{filename: (specs [n, F, T], onsets, offsets, filenames)}``, every
    spectrogram one ``windows`` call of its own"""
    q = sorted(quantiles)
    out = {}
    for index, fn in enumerate(dset.audio_filenames):
        specs, onsets, offsets = [], [], []
        for q1, q2 in zip(q[:-1], q[1:]):
            target_ts = dset._target_times(index, q1, q2, dset.p['num_time_bins'])
            spec = dset.windows([index], target_ts[None, :])[0]
            specs.append(np.asarray(spec.cpu().numpy() if hasattr(spec, 'cpu') else spec))
            onsets.append(q1)
            offsets.append(q2)
        out[fn] = (np.stack(specs), np.array(onsets), np.array(offsets), np.array([fn] * len(specs)).astype('S'))
    return out
