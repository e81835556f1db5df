"""Cases of the amplitude segmentation's tests (ava_amd.segment, csrc/segment.hip, the band stage of csrc/stft.h).

Two kinds.  The cases of tests/golden/segment.npz (written by tests/golden/make_golden_segment.py): the audio of every
case is regenerated from ``ava_amd.synthetic`` by the recipe stored with it, so that the fixture holds only results
(``audio_of``, ``load``).  And seeded cases at the kernels' own edges with a plain numpy restatement of what the kernels
compute, ``np.longdouble`` (64-bit significand on x86) wherever a sum is formed: ``candidates`` for the decision kernels,
``band_values`` for band_stft_kernel, ``smoothed`` for amp_smooth_kernel.  Nothing of ava_amd is used but ``synthetic``
and the host helpers of ava_amd.segment that tests/test_cpu_segment.py holds against scipy.  tests/test_cpu_segment.py
asserts the properties the cases are built for, holds the restatement against scipy and shows that wrong variants of it
break the bounds.

Bounds (``U`` = 2^-53, N = nperseg, F kept bins).  They are fixed from the reference side: scipy's own fp64 stft, the
arithmetic of the reference, stays within 0.06 of the spectrum bound, of the ``v`` bound and of the per-frame bounds
against the longdouble DFT on every row below (N = 64..2048, hops 1, N/3, N/2, N); the CPU test asserts scipy within
half of every bound, the GPU tests hold the device to the whole bound.

  spectrum   A radix-2 transform of N real samples through an N/2-point complex FFT and the split step applies at most
             about 4 log2 N roundings to every term w_n x_n of every bin, each relative to a partial sum that is at most
             S1 = scale sum_n |w_n x_n|.  |dX| <= C_FFT log2(N) U S1 with C_FFT = 8: twice the count, which covers the
             window product, the split step and the magnitude.                                       (``spectrum_bound``)
  v          lg = log(|X| + 1e-9) moves by |dX| / (|X| + 1e-9) (log is 1 / x-Lipschitz) and by 2 U |lg| for the
             logarithm's and the sum's roundings, 2 U for the scale's; (lg - spec_min) / range adds the subtraction's and
             the division's roundings: |dv| <= (C_FFT log2(N) U S1 / (|X| + 1e-9) + 4 U (1 + |lg| + |spec_min|)) / |range|
             + 2 U.  The clip is 1-Lipschitz, so this also holds at the clips.                              (``v_bound``)
  sum        F additions of non-negative terms: the sum of the elements' bounds plus (F + 2) U sum v.     (``sum_bound``)
  softmax    f = sum v e / (sum e + 1e-9), e = exp(v / t): df / dv_k = p_k (1 + (v_k - f) / t) with p_k = e_k / (sum e +
             1e-9), sum p_k <= 1 and |v_k - f| <= v_max - v_min, so the elements' errors move f by at most
             max_k |dv_k| (1 + (v_max - v_min) / |t|).  Rounding: relative errors d_k of the weights move a weighted mean
             by at most max |d_k| (v_max - v_min) <= max |d_k|, and d_k <= (2 + |v / t|) U (exp to two ulp, the rounded
             quotient v / t); the two sums of F positive terms are within (F + 1) U relative each, the final quotient U,
             and f <= 1.  Together (2 F + 2) U + (2 + 1 / |t|) U + U <= (2 F + 8) U while 1 / |t| <= 3; every case here
             has t = 0.5 and ``softmax_bound`` refuses a smaller |t|.
  smoothing  2 radius + 1 fused multiply-adds in fp64: (2 radius + 2) U sum_k |w_k| |raw|; a float32 trace adds its one
             rounding, 2^-24 |want|.                                                                    (``smooth_bound``)
"""
import functools
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


# ---- the decisions: restatement --------------------------------------------------------------------------------------
U = 2.0 ** -53
C_FFT = 8.0
EPS = 1e-9                                 # segmenting/utils.py:19
LD = np.longdouble


def _thresholds(th, dtype):
    from ava_amd import segment as S
    return S.decide_thresholds(th, dtype)


def candidates(trace, th, dtype):
    """(maxima, left, right) of one file's trace with numpy and the reference's own predicates: the maxima above th_3,
    and the nearest stop on either side of each (-1: none), for the host chain.  ``th`` holds th_1, th_2 and th_3; they
    are compared as numpy compares them with a trace of ``dtype``."""
    th1, th2, th3 = _thresholds(th, dtype)
    a = trace.astype(np.float64)
    T = len(a)
    mx = [i for i in range(1, T - 1) if a[i] > th3 and a[i] == a[i - 1:i + 2].max()]

    def stop(j):
        return a[j] < th1 or (a[j] < th2 and a[j] == a[j - 1:j + 2].min())
    left = [next((j for j in range(m - 1, 0, -1) if stop(j)), -1) for m in mx]
    right = [next((j for j in range(m + 1, T) if stop(j)), -1) for m in mx]
    return mx, left, right


def candidates_per_file(trace, frame_off, th, dtype):
    """``candidates`` of every file of a batch trace (indices inside the file)"""
    return [candidates(trace[frame_off[f]:frame_off[f + 1]], th, dtype) for f in range(len(frame_off) - 1)]


def while_loop_candidates(trace, th, dtype):
    """The same triples by the reference's two searches as it writes them (amplitude_segmentation.py:72-100), without
    its chain: the trace in its own dtype against the Python thresholds, one index walked down while it is above 0 and
    one walked up while it is below the length."""
    amps = np.asarray(trace, dtype=dtype)
    th_1, th_2, th_3 = th['th_1'], th['th_2'], th['th_3']
    mx, left, right = [], [], []
    for i in range(1, len(amps) - 1, 1):
        if amps[i] > th_3 and amps[i] == np.max(amps[i - 1:i + 2]):
            mx.append(i)
    for m in mx:
        found = -1
        i = m - 1
        while i > 0:
            if amps[i] < th_1:
                found = i
                break
            elif amps[i] < th_2 and amps[i] == np.min(amps[i - 1:i + 2]):
                found = i
                break
            i -= 1
        left.append(found)
        found = -1
        i = m + 1
        while i < len(amps):
            if amps[i] < th_1:
                found = i
                break
            elif amps[i] < th_2 and amps[i] == np.min(amps[i - 1:i + 2]):
                found = i
                break
            i += 1
        right.append(found)
    return mx, left, right


def wrong_candidates(trace, frame_off, th, dtype, wrong):
    """Per file, what a wrong kernel would give (tests/test_cpu_segment.py shows that the cases tell each from
    ``candidates``): ``'span64'`` looks at 64 frames on either side only, ``'stop0'`` lets the left search accept frame
    0, ``'across'`` takes no notice of where a file ends: the neighbours of a frame are those of the whole trace, the
    first and last frame of a file may be maxima, and the searches are still those of the file."""
    th1, th2, th3 = _thresholds(th, dtype)
    a = np.asarray(trace).astype(np.float64)
    out = []
    for f in range(len(frame_off) - 1):
        b, e = int(frame_off[f]), int(frame_off[f + 1])
        T = e - b
        lo, hi = (0, len(a)) if wrong == 'across' else (b, e)

        def near(g):
            return a[max(g - 1, lo):min(g + 2, hi)]

        def stop(j):
            return a[b + j] < th1 or (a[b + j] < th2 and a[b + j] == near(b + j).min())
        if wrong == 'across':
            cand = [i for i in range(T) if 0 < b + i < len(a) - 1]
        else:
            cand = range(1, T - 1)
        mx = [i for i in cand if a[b + i] > th3 and a[b + i] == near(b + i).max()]
        first = 0 if wrong == 'stop0' else 1
        span = 64 if wrong == 'span64' else T
        left = [next((j for j in range(m - 1, max(first, m - span) - 1, -1) if stop(j)), -1) for m in mx]
        right = [next((j for j in range(m + 1, min(T, m + span + 1)) if stop(j)), -1) for m in mx]
        out.append((mx, left, right))
    return out


# ---- the decisions: cases ----------------------------------------------------------------------------------------------
# Every trace value is a multiple of 1 / 1024 below 1: the float32 and the float64 copy of a case hold the same numbers,
# none near a threshold.
TH = dict(th_1=0.1, th_2=0.2, th_3=0.3)
_LOW, _MID, _FLAT, _PEAK = 50, 150, 250, 900     # below th_1; in [th_1, th_2); in [th_2, th_3); a maximum
DISTANCES = (1, 2, 63, 64, 65, 127, 128, 129, 300)
NAN = float('nan')


def _one_file(values):
    a = np.asarray(values, dtype=np.float64) / 1024.0
    return a, np.array([0, len(a)], dtype=np.int64)


def _far_stops():
    """peaks whose nearest stop lies exactly D frames away, every D of DISTANCES on either side, once as a frame below
    th_1 and once as a local minimum below th_2; the frames between fall by 2 / 1024 a frame and stay above th_3"""
    def slope(D):
        return [_PEAK - 2 * d for d in range(1, D)]
    a = [_FLAT]
    for rule in (1, 2):
        for i, d_left in enumerate(DISTANCES):
            d_right = DISTANCES[(i + 4) % len(DISTANCES)]
            s_left, s_right = (_LOW, _MID) if rule == 1 else (_MID, _LOW)
            a += [s_left] + slope(d_left)[::-1] + [_PEAK] + slope(d_right) + [s_right, _FLAT]
    return _one_file(a)


def _many_maxima():
    """T = 20001: every odd frame is a maximum (10000 of them: more than the 8192 waves of amp_stops_kernel's capped
    grid), the even frames between are stops or not by a hash stream, so the distances vary"""
    from ava_amd import synthetic as syn
    T = 20001
    u = syn.u01(T, 5150)
    a = np.where(u < 0.4, _LOW, np.where(u < 0.6, _MID, _FLAT)).astype(np.float64)
    a[1::2] = 400 + np.floor(500 * syn.u01(T // 2, 5151))
    return _one_file(a)


BOUNDARY_FILES = (
    [], [],                                  # 0, 1   no frames, at the start
    [900],                                   # 2      one frame
    [900, 50],                               # 3      two frames
    [50, 700, 50],                           # 4      three frames: the maximum at 1 = T - 2 has no left stop
    [50, 40, 500, 800, 400],                 # 5      maximum at T - 2 without a right stop; the next file starts below th_1
    [30, 700, 350, 45],                      # 6      maximum at 1 without a left stop, frame 0 below th_1; ends below th_1
    [35, 750, 40, 600, 20],                  # 7      the mirror: the file before ends below th_1, the maximum at 1 has -1
    [],                                      # 8      no frames, in the middle
    [300, 40, 800, 400, 150],                # 9      the last frame is a th_2 stop only because the slice is clipped
    [120, 600, 30],                          # 10     ... the next file's first frame is lower
    [990, 40, 700, 45, 995],                 # 11     first and last frame exceed all neighbours, in the files around too
    [60, 650],                               # 12
    [10],                                    # 13
    [], [],                                  # 14, 15 no frames, at the end
)


def _boundaries():
    T = [len(f) for f in BOUNDARY_FILES]
    a = np.array([v for f in BOUNDARY_FILES for v in f], dtype=np.float64) / 1024.0
    return a, np.concatenate([[0], np.cumsum(T)]).astype(np.int64)


def _plateaus_nan():
    return _one_file([50, 700, 700, 50, 290, 150, 150, 290, 800, 50,        # tied maxima at 1, 2; tied minima at 5, 6
                      600, NAN, 600, 50,                                    # NaN between two would-be maxima: none
                      900, 400, 150, NAN, 40, 290,                          # 16 would stop but for the NaN beside it
                      850, 400, NAN, 150, 290, 30, 290])                    # NaN on the way, and beside the minimum at 23


WAVE_MAXIMA = tuple(range(1, 64, 2)) + (128, 255, 256) + tuple(range(512, 576, 2)) + (700, 1023, 1024, 1098)


def _waves():
    """T = 1100 (five workgroups of amp_maxima_kernel): waves with 32 maxima, with one and with none inside one
    workgroup, maxima at lanes 0 and 63 and on either side of a workgroup's edge (255 | 256, 1023 | 1024, tied)"""
    a = np.full(1100, _FLAT, dtype=np.float64)
    a[list(WAVE_MAXIMA)] = 700
    a[[10, 40, 100, 300, 600, 900, 1099]] = _LOW
    a[[200, 531, 1000]] = _MID
    return _one_file(a)


DECISION_CASES = {"far_stops": _far_stops, "many_maxima": _many_maxima, "boundaries": _boundaries,
                  "plateaus_nan": _plateaus_nan, "waves": _waves}


@functools.lru_cache(maxsize=None)
def decision_case(name):
    """(trace float64 [frames], frame_off int64 [files + 1]); shared among the tests: never written to"""
    a, fo = DECISION_CASES[name]()
    a.setflags(write=False)
    fo.setflags(write=False)
    return a, fo


@functools.lru_cache(maxsize=None)
def decision_want(name, dtype):
    """``candidates_per_file`` of a case in ``dtype`` ('float32' or 'float64')"""
    a, fo = decision_case(name)
    return candidates_per_file(a.astype(dtype), fo, TH, np.dtype(dtype))


# ---- the band stage: restatement --------------------------------------------------------------------------------------
def frames_of(x, nperseg, hop, wrong=None):
    """scipy.signal.stft's frames [T, nperseg] of one file (any float type): zero boundary of nperseg / 2 on either side,
    zero padded to whole hops.  ``wrong='left'`` puts the whole boundary in front."""
    half = nperseg // 2
    lead, tail = (nperseg, 0) if wrong == 'left' else (half, half)
    ext = np.concatenate([np.zeros(lead, dtype=x.dtype), x, np.zeros(tail, dtype=x.dtype)])
    nadd = (-(len(ext) - nperseg) % hop) % nperseg
    ext = np.concatenate([ext, np.zeros(nadd, dtype=x.dtype)])
    T = (len(ext) - nperseg) // hop + 1
    return ext[np.arange(T)[:, None] * hop + np.arange(nperseg)[None, :]]


@functools.lru_cache(maxsize=None)
def _twiddles(nperseg, k0, k1):
    """cos and sin of 2 pi n k / N for 0 <= n < N, k0 <= k < k1, longdouble, the argument reduced mod N as an integer"""
    pi = 4 * np.arctan(LD(1))
    ang = 2 * pi * np.arange(nperseg).astype(LD) / LD(nperseg)
    m = (np.arange(nperseg, dtype=np.int64)[:, None] * np.arange(k0, k1, dtype=np.int64)[None, :]) % nperseg
    return np.cos(ang)[m], np.sin(ang)[m]


def hann(nperseg):
    from scipy.signal import get_window
    return get_window('hann', nperseg)                                    # periodic


def band_spectrum(audio, p, wrong=None):
    """Per file of ``audio`` (a list of 1-D arrays; files below nperseg samples have no frames), joined along the frames:
    dict of the scaled one-sided spectrum of the kept bins ``re``, ``im`` [F, frames] by a direct longdouble DFT of
    scipy's frames, ``X`` = |X|, ``lg`` = log(|X| + 1e-9), ``S1`` = scale sum_n |w_n x_n| [frames], and ``frame_off``.
    ``wrong``: 'hann' (window shifted by one sample), 'nyquist' (sign of W^k O_k flipped in the bin N / 2), 'eps' (1e-9
    left out), 'left' (boundary zeros in front only)."""
    from ava_amd import segment as S
    N, hop = int(p['nperseg']), int(p['nperseg']) - int(p['noverlap'])
    k0, k1, _ = S.band_indices(p)
    w = hann(N).astype(LD)
    scale = 1 / w.sum(dtype=LD)
    if wrong == 'hann':
        w = np.roll(w, 1)
    cs, sn = _twiddles(N, k0, k1)
    re, im, s1, T = [], [], [], []
    for x in audio:
        if len(x) < N:
            T.append(0)
            continue
        wx = frames_of(np.asarray(x).astype(np.float64).astype(LD), N, hop, wrong) * w[None, :]
        r, i = wx @ cs, -(wx @ sn)
        if wrong == 'nyquist' and k1 == N // 2 + 1:
            r[:, -1] = wx.sum(axis=1, dtype=LD)                           # E + O where the bin is E - O
        re.append(r.T * scale)
        im.append(i.T * scale)
        s1.append(np.abs(wx).sum(axis=1, dtype=LD) * scale)
        T.append(len(wx))
    out = dict(re=np.concatenate(re, axis=1), im=np.concatenate(im, axis=1), S1=np.concatenate(s1),
               frame_off=np.concatenate([[0], np.cumsum(T)]).astype(np.int64))
    out['X'] = np.sqrt(out['re'] * out['re'] + out['im'] * out['im'])
    with np.errstate(divide='ignore'):
        out['lg'] = np.log(out['X'] + (0 if wrong == 'eps' else LD(EPS)))
    return out


def band_values(audio, p, wrong=None, spectrum=None):
    """``band_spectrum`` and what band_stft_kernel makes of it, longdouble: ``u`` = (lg - spec_min) / range, ``v`` =
    clip(u, 0, 1) [F, frames], ``value`` [frames] = sum v, or sum v e / (sum e + 1e-9), e = exp(v / temperature), with
    ``p['softmax']``.  ``wrong='lastbin'`` drops the last kept bin from ``value``."""
    out = dict(band_spectrum(audio, p, wrong) if spectrum is None else spectrum)
    spec_min = LD(float(p['spec_min_val']))
    rng = LD(float(p['spec_max_val']) - float(p['spec_min_val']))         # the reference's fp64 difference
    out['u'] = (out['lg'] - spec_min) / rng
    v = out['v'] = np.clip(out['u'], 0, 1)
    if wrong == 'lastbin':
        v = v[:-1]
    if p.get('softmax', False):
        e = np.exp(v / LD(float(p['temperature'])))
        out['value'] = (v * e).sum(axis=0, dtype=LD) / (e.sum(axis=0, dtype=LD) + LD(EPS))
    else:
        out['value'] = v.sum(axis=0, dtype=LD)
    return out


def smoothed(raw, frame_off, w, radius):
    """scipy.ndimage.gaussian_filter's correlation with the weights ``w`` inside every file, longdouble: mode 'reflect'
    (d c b a | a b c d | d c b a) has the period 2 T, m = (i + k) mod 2 T mirrored when m >= T"""
    return _reflect_sum(np.asarray(raw).astype(LD), frame_off, np.asarray(w).astype(LD), radius, 0)


def _reflect_sum(raw, frame_off, w, radius, shorter):
    out = np.zeros(len(raw), dtype=raw.dtype)
    for f in range(len(frame_off) - 1):
        b, T = int(frame_off[f]), int(frame_off[f + 1] - frame_off[f])
        if T == 0:
            continue
        P = 2 * T - shorter                                               # shorter = 2: scipy's 'mirror', for T >= 2
        m = (np.arange(T)[:, None] + np.arange(-radius, radius + 1)[None, :]) % P
        m = np.where(m >= T, P - 1 + shorter // 2 - m, m)
        out[b:b + T] = (raw[b + m] * w[None, :]).sum(axis=1, dtype=raw.dtype)
    return out


def wrong_smoothed(raw, frame_off, w, radius):
    """the reflect period taken as 2 T - 2 (d c b | a b c d | c b a: scipy's 'mirror')"""
    return _reflect_sum(np.asarray(raw).astype(LD), frame_off, np.asarray(w).astype(LD), radius, 2)


# ---- the band stage: bounds ------------------------------------------------------------------------------------------
def spectrum_bound(b, p):
    """[frames] bound of |dX| of every bin of a frame"""
    return C_FFT * np.log2(int(p['nperseg'])) * U * b['S1']


def v_bound(b, p):
    """[F, frames] bound of |dv|, element by element"""
    spec_min = abs(float(p['spec_min_val']))
    rng = abs(float(p['spec_max_val']) - float(p['spec_min_val']))
    return (spectrum_bound(b, p)[None, :] / (b['X'] + LD(EPS)) + 4 * U * (1 + np.abs(b['lg']) + spec_min)) / rng + 2 * U


def sum_bound(b, p):
    F = b['v'].shape[0]
    return v_bound(b, p).sum(axis=0, dtype=LD) + (F + 2) * U * b['v'].sum(axis=0, dtype=LD)


def softmax_bound(b, p):
    t = abs(float(p['temperature']))
    assert 1 / t <= 3, "the rounding term (2 F + 8) U is derived for 1 / |temperature| <= 3"
    F, v = b['v'].shape[0], b['v']
    return v_bound(b, p).max(axis=0) * (1 + (v.max(axis=0) - v.min(axis=0)) / t) + (2 * F + 8) * U


def value_bound(b, p):
    """[frames] bound of the per-frame value in fp64"""
    return softmax_bound(b, p) if p.get('softmax', False) else sum_bound(b, p)


def smooth_bound(raw, frame_off, w, radius, want=None, float32=False):
    """[frames] bound of the smoothed trace; ``float32`` adds the one rounding of ``want`` to the trace's dtype"""
    out = (2 * radius + 2) * U * _reflect_sum(np.abs(np.asarray(raw)).astype(LD), frame_off,
                                              np.abs(np.asarray(w)).astype(LD), radius, 0)
    return out + 2.0 ** -24 * np.abs(want) if float32 else out


# ---- the band stage: cases -------------------------------------------------------------------------------------------
# fs = nperseg puts bin k at the frequency k: min_freq = k0 and max_freq = k1 keep the bins k0 <= k < k1.
def _row(nperseg, hop, k0, k1, n0, modes):
    return dict(nperseg=nperseg, hop=hop, k0=k0, k1=k1, n0=n0, modes=modes)


# n0: samples of the first file, never a whole number of hops
BAND_ROWS = {
    "n64_hop64_full": _row(64, 64, 0, 33, 64 * 37 + 13, ("sum", "softmax")),     # H = 32, odd final pass, DC, Nyquist
    "n64_hop1_b3_20": _row(64, 1, 3, 21, 601, ("softmax",)),                     # hop 1, F < 64; (601 = 600 hops + 1)
    "n64_hop64_4200": _row(64, 64, 1, 33, 64 * 4200 + 31, ("sum",)),             # 4202 frames: the frame grid stride
    "n128_hop43_full": _row(128, 43, 0, 65, 43 * 90 + 20, ("softmax",)),         # H = 64
    "n256_hop128_b10_100": _row(256, 128, 10, 101, 128 * 50 + 77, ("sum", "softmax")),
    "n512_hop171_full": _row(512, 171, 0, 257, 171 * 40 + 100, ("softmax",)),    # F = 257: the bin stride
    "n1024_hop512_full": _row(1024, 512, 0, 513, 512 * 20 + 300, ("softmax",)),
    "n2048_hop1365_full": _row(2048, 1365, 0, 1025, 1365 * 18 + 700, ("sum", "softmax")),   # 20 + 3 frames
}
BAND_MODES = [(r, m) for r, c in BAND_ROWS.items() for m in c['modes']]
DTYPE_ROWS = {"n256_hop128_b10_100": "sum", "n1024_hop512_full": "softmax"}
DTYPES = ("int16", "int32", "float32")
QUANTILES = (0.15, 0.9)                   # of lg over the kept band: spec_min_val and spec_max_val of a case


def _base_audio(n, nperseg, hop, salt, zeros=True):
    """a gated tone over noise and a DC offset, in int16 units, with a stretch of nperseg + hop + 17 exact zeros"""
    from ava_amd import synthetic as syn
    t = np.arange(n, dtype=np.float64)
    phase = 2.0 * np.pi * (0.11 * t + 3.0 * np.sin(2.0 * np.pi * t / (7.0 * nperseg)))
    gate = (np.sin(2.0 * np.pi * t / (5.3 * nperseg) + 1.0) > -0.3).astype(np.float64)
    x = 3000.0 * gate * (np.sin(phase) + 0.4 * np.sin(2.1 * phase)) + 60.0 * syn.gauss(n, salt) + 30.0
    if zeros:
        z = nperseg + hop + 17
        assert n > 2 * z
        start = (n - z) // 3
        x[start:start + z] = 0.0
    return x


def _to_dtype(x, dtype):
    if dtype == 'int16':
        return np.rint(x).astype(np.int16)
    if dtype == 'int32':
        return np.rint(x * 65536.0).astype(np.int32)
    return (x / 32768.0).astype(dtype)


@functools.lru_cache(maxsize=None)
def band_audio(row, dtype='float64'):
    """the three files of a row: n0 samples (no whole number of hops), exactly nperseg, and nperseg - 1 (no frames)"""
    c = BAND_ROWS[row]
    salt = 5200 + 10 * sorted(BAND_ROWS).index(row)
    lengths = (c['n0'], c['nperseg'], c['nperseg'] - 1)
    assert c['n0'] % c['hop'] != 0 or c['hop'] == 1
    audio = tuple(_to_dtype(_base_audio(n, c['nperseg'], c['hop'], salt + k, zeros=k == 0), dtype)
                  for k, n in enumerate(lengths))
    for a in audio:
        a.setflags(write=False)
    return audio


def _band_p(row):
    c = BAND_ROWS[row]
    return dict(fs=c['nperseg'], nperseg=c['nperseg'], noverlap=c['nperseg'] - c['hop'], min_freq=c['k0'],
                max_freq=c['k1'], temperature=0.5)


@functools.lru_cache(maxsize=None)
def _band_spectrum_of(row, dtype):
    return band_spectrum(band_audio(row, dtype), _band_p(row))


@functools.lru_cache(maxsize=None)
def band_params(row, mode, dtype='float64'):
    """the parameter dict of a case: spec_min_val and spec_max_val are the QUANTILES of the restatement's lg"""
    lg = _band_spectrum_of(row, dtype)['lg'].astype(np.float64)
    lo, hi = (float(q) for q in np.quantile(lg, QUANTILES))
    return dict(_band_p(row), spec_min_val=lo, spec_max_val=hi, softmax=mode == 'softmax')


@functools.lru_cache(maxsize=None)
def band_want(row, mode, dtype='float64'):
    """``band_values`` of a case (longdouble arrays, shared: never written to)"""
    out = band_values(None, band_params(row, mode, dtype), spectrum=_band_spectrum_of(row, dtype))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the smoothing: cases --------------------------------------------------------------------------------------------
SMOOTH_P = dict(fs=64, nperseg=64, noverlap=0, min_freq=2, max_freq=30, spec_min_val=2.0, spec_max_val=6.0,
                softmax=False)
SMOOTH_FRAMES = (2, 3, 4, 5, 40)
SMOOTH_RADII = (1, 2, 5, 9, 11, 35)       # below T, T, 2 T and 2 T + 1 of the short files, and several periods


@functools.lru_cache(maxsize=None)
def smooth_audio(dtype='float64'):
    """files of SMOOTH_FRAMES frames at nperseg = hop = 64, in int16 units whatever the dtype: the float64 copy of the
    int16 files means the same samples"""
    lengths = [64 * (T - 1) for T in SMOOTH_FRAMES]
    audio = tuple(_base_audio(n, 64, 64, 5400 + k, zeros=False) for k, n in enumerate(lengths))
    if dtype == 'int16':
        audio = tuple(_to_dtype(a, dtype) for a in audio)
    for a in audio:
        a.setflags(write=False)
    return audio


def smooth_timescale(radius):
    """a smoothing_timescale for which gaussian_weights gives this radius at SMOOTH_P's frame step of 1 s"""
    return radius / 4.0
