"""Writes tests/golden/segment.npz: the reference's amplitude segmentation
(ava/segmenting/amplitude_segmentation.py:get_onsets_offsets, ava/segmenting/utils.py:get_spec) on synthetic
recordings and on hand-made traces.  Needs the reference package and scipy; run from the repository root as
``python tests/golden/make_golden_segment.py /path/to/reference``.  The GPU tests only read the npz.

Per recording case: the recipe of its audio (tests/segment_cases.py regenerates it), the parameters, per file the
reference's trace / onsets / offsets on the audio as given and on the float64-cast audio, dt, a seeded sample of the
band spectrogram of file 0 with its own tolerance (the same rule per bin), and the trace's tolerance max(4 |trace - trace64|_max, 4 fp32 ulp of the peak).  A case is
refused when a trace value lies within 10x that tolerance of a threshold that decides something, or when a
neighbour comparison the decisions use is that close.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AVA_REFERENCE", "../reference"))

import segment_cases as SC                                  # noqa: E402
import ava.segmenting.amplitude_segmentation as A           # noqa: E402
import ava.segmenting.utils as U                            # noqa: E402

OUT = {}
SPEC_SAMPLES = 256


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def check_margins(name, tr, p, tol):
    a = tr.astype(np.float64)
    m = 10.0 * tol
    for key in ('th_1', 'th_2', 'th_3'):
        d = np.abs(a - p[key])
        if d.min() < m:
            raise SystemExit("%s: trace value %.9g within %.3g of %s = %s" % (name, a[d.argmin()], m, key, p[key]))
    T = len(a)
    for i in range(1, T):
        hi_side = a[i] > p['th_3'] or a[i - 1] > p['th_3']                       # maxima tests
        lo_side = p['th_1'] <= a[i] < p['th_2'] or p['th_1'] <= a[i - 1] < p['th_2']   # minima tests
        if (hi_side or lo_side) and a[i] != a[i - 1] and abs(a[i] - a[i - 1]) < m:
            raise SystemExit("%s: neighbours %d, %d differ by %.3g < %.3g" % (name, i - 1, i, abs(a[i] - a[i - 1]), m))


def rec_case(name, params, recipe):
    p = dict(params)
    audio = SC.audio_of(recipe)
    entry = {'p': np.array(json.dumps(p)), 'recipe': np.array(json.dumps(recipe))}
    gap, peak = 0.0, 0.0
    results = []
    for k, a in enumerate(audio):
        r = A.get_onsets_offsets(a, p, return_traces=True)
        r64 = A.get_onsets_offsets(a.astype(np.float64), p, return_traces=True)
        results.append((r, r64))
        if r[2] is not None:
            gap = max(gap, float(np.abs(r[2][0].astype(np.float64) - r64[2][0]).max()))
            peak = max(peak, float(np.abs(r[2][0]).max()))
    tol = max(4.0 * gap, 4.0 * ulp32(peak))
    for k, (r, r64) in enumerate(results):
        entry['on_%d' % k] = np.array(r[0], dtype=np.float64)
        entry['off_%d' % k] = np.array(r[1], dtype=np.float64)
        entry['on64_%d' % k] = np.array(r64[0], dtype=np.float64)
        entry['off64_%d' % k] = np.array(r64[1], dtype=np.float64)
        if r[2] is None:
            entry['nframes_%d' % k] = np.array(0)
            continue
        tr = r[2][0]
        check_margins("%s file %d" % (name, k), tr, p, tol)
        assert r[0] == r64[0] and r[1] == r64[1], name + ": float32 and float64 decisions differ"
        entry['nframes_%d' % k] = np.array(len(tr))
        entry['trace_%d' % k] = tr
        entry['trace64_%d' % k] = r64[2][0]
    spec, dt, f = U.get_spec(audio[0], p) if len(audio[0]) >= p['nperseg'] else (None, None, None)
    if spec is not None:
        rs = np.random.RandomState(7)
        idx = np.sort(rs.choice(spec.size, size=min(SPEC_SAMPLES, spec.size), replace=False))
        entry['spec_shape'] = np.array(spec.shape)
        entry['spec_idx'] = idx.astype(np.int64)
        entry['spec_val'] = spec.reshape(-1)[idx]
        spec64 = U.get_spec(audio[0].astype(np.float64), p)[0]
        gap_spec = float(np.abs(spec.astype(np.float64) - spec64).max())
        entry['spec_tol'] = np.array(max(4.0 * gap_spec, 4.0 * ulp32(1.0)))
        entry['dt'] = np.array(dt, dtype=np.float64)
        entry['f'] = f
    entry['tol'] = np.array(tol)
    entry['n_files'] = np.array(len(audio))
    for key, v in entry.items():
        OUT[name + '/' + key] = v
    counts = [len(r[0]) for r, _ in results]
    print("%-28s tol %.2e  syllables per file %s" % (name, tol, counts))
    return entry


def hand_case(name, values, dtype, th, min_dur=0.0, max_dur=1e9, dt=0.01):
    trace = np.array(values, dtype=dtype)
    p = dict(nperseg=1, th_1=th[0], th_2=th[1], th_3=th[2], min_dur=min_dur, max_dur=max_dur, softmax=False,
             smoothing_timescale=0.0)
    dt = np.float64(dt)
    saved = A.get_spec, A.gaussian_filter
    A.get_spec = lambda audio, q: (trace[None, :], dt, None)
    A.gaussian_filter = lambda x, s: x
    try:
        on, off, tr = A.get_onsets_offsets(np.zeros(1), p, return_traces=True)
    finally:
        A.get_spec, A.gaussian_filter = saved
    assert tr[0].dtype == trace.dtype
    OUT[name + '/p'] = np.array(json.dumps(p))
    OUT[name + '/trace'] = trace
    OUT[name + '/dt'] = np.array(dt)
    OUT[name + '/on'] = np.array(on, dtype=np.float64)
    OUT[name + '/off'] = np.array(off, dtype=np.float64)
    print("%-28s T %4d  syllables %d" % (name, len(trace), len(on)))


def main():
    names = []
    for animal, P, secs in (('mouse', SC.MOUSE, 2.0), ('finch', SC.FINCH, 2.0)):
        for softmax in (False, True):
            for dt in ('int16', 'int32', 'float32', 'float64'):
                p = dict(P, softmax=softmax)
                if animal == 'mouse':
                    p.update(th_1=2.0, th_2=5.0, th_3=10.0) if not softmax else p.update(th_1=0.03, th_2=0.06, th_3=0.1)
                else:
                    p.update(th_1=5.0, th_2=10.0, th_3=20.0) if not softmax else p.update(th_1=0.1, th_2=0.2, th_3=0.3)
                if dt.startswith('float'):
                    p['spec_min_val'] -= SC.LOG_INT16_SCALE
                    p['spec_max_val'] -= SC.LOG_INT16_SCALE
                name = "%s_%s_%s" % (animal, dt, 'softmax' if softmax else 'sum')
                rec_case(name, p, dict(kind='rec', dtype=dt, fs=P['fs'], seconds=secs, n_files=2))
                names.append(name)
    # durations: one syllable too short, two too long
    p = dict(SC.MOUSE, softmax=False, th_1=2.0, th_2=5.0, th_3=10.0, min_dur=0.08, max_dur=0.2)
    rec_case('mouse_int16_durations', p, dict(kind='rec', dtype='int16', fs=p['fs'], seconds=2.0, n_files=2))
    names.append('mouse_int16_durations')
    # edge files: shorter than nperseg, exactly nperseg (T = 3), T = 4, all zeros, radius > T
    p = dict(SC.MOUSE, softmax=False, th_1=2.0, th_2=5.0, th_3=10.0)
    rec_case('mouse_int16_edges', p, dict(kind='edge', dtype='int16', fs=p['fs'], lengths=[500, 1024, 1025, 1536, -20000,
                                                                                            60000]))
    names.append('mouse_int16_edges')
    p = dict(SC.FINCH, noverlap=0, softmax=False, th_1=5.0, th_2=10.0, th_3=20.0)    # hop = nperseg: T = 2 at nperseg
    rec_case('finch_float32_hop0_edges', dict(p, spec_min_val=p['spec_min_val'] - SC.LOG_INT16_SCALE,
                                              spec_max_val=p['spec_max_val'] - SC.LOG_INT16_SCALE),
             dict(kind='edge', dtype='float32', fs=p['fs'], lengths=[511, 512, 513, 1024, -4096, 16000]))
    names.append('finch_float32_hop0_edges')
    OUT['case_names'] = np.array(json.dumps(names))

    hand = []
    rs = np.random.RandomState(11)
    smooth = np.convolve(rs.standard_normal(260), np.ones(8) / 8, mode='valid')[:200] * 3 + 2
    for dtype in ('float32', 'float64'):
        cases = [
            ('plateau', [0, 0.5, 3, 3, 3, 0.5, 0, 0.5, 4, 4, 0.2, 0], (1.0, 2.0, 2.5)),
            ('exact_dyadic', [0, 0.25, 1.0, 0.5, 0.5, 2.0, 1.0, 0.5, 0.75, 2.0, 0.25, 0], (0.25, 0.5, 1.0)),
            ('exact_decimal', [0, 0.1, 0.3, 0.2, 0.25, 0.4, 0.2, 0.3, 0.1, 0.35, 0.1, 0], (0.1, 0.2, 0.3)),
            ('no_left_stop', [5, 5, 6, 9, 6, 0.5, 0, 0], (1.0, 2.0, 3.0)),
            ('no_right_stop', [0, 0.5, 6, 9, 6, 5, 5], (1.0, 2.0, 3.0)),
            ('inside_previous', [0, 1, 5, 4.5, 6, 1, 0, 0.5, 7, 0.2, 0], (1.5, 4.0, 4.2)),
            ('edge_maxima', [0, 9, 0, 0.5, 0, 0, 9, 0], (1.0, 2.0, 3.0)),
            ('tied_minima', [0, 0.5, 5, 3, 3, 5, 0.5, 0, 3, 3, 3, 6, 3, 3, 0], (1.0, 4.0, 4.5)),
            ('len1', [9], (1.0, 2.0, 3.0)),
            ('len2', [0, 9], (1.0, 2.0, 3.0)),
            ('len3', [0, 9, 0], (1.0, 2.0, 3.0)),
            ('noise', smooth.tolist(), (1.0, 2.0, 3.5)),
        ]
        for nm, vals, th in cases:
            name = "hand_%s_%s" % (nm, dtype)
            hand_case(name, vals, dtype, th)
            hand.append(name)
        name = "hand_noise_durations_%s" % dtype
        hand_case(name, smooth.tolist(), dtype, (1.0, 2.0, 3.5), min_dur=0.05, max_dur=0.3)
        hand.append(name)
    OUT['hand_names'] = np.array(json.dumps(hand))
    path = os.path.join(HERE, "segment.npz")
    np.savez_compressed(path, **OUT)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
