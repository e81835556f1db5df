"""Writes tests/golden/template.npz: the reference's template segmentation
(ava/segmenting/template_segmentation.py: get_template, _segment_file, _clean_max_indices) on synthetic song and on
hand-made maxima.  Needs the reference package and scipy; run from the repository root as
``python tests/golden/make_golden_template.py /path/to/reference``.  The GPU tests only read the npz.

The reference module imports affinewarp, umap, h5py and ava.plotting.tooltip_plot at load time; none of them is used
by the functions above, so they are stubbed here.  _segment_file returns only segments: its trace is captured through a
numpy proxy handed to the module for the call, whose ``median`` records its first argument (``np.median(result)``).

Per case: the recipe of its audio (tests/template_cases.py regenerates it), the parameters, the reference's template
on the exemplars as given and on the float64-cast exemplars, and per file the reference's trace and segments on the
audio as given (with the template as given) and on the float64-cast audio (with the float64 template).  The trace
tolerance is max(4 |trace - trace64|_max, 4 fp32 ulp of the peak), the template's the same rule.  A case is refused
when a decision could flip within 10x that tolerance: a trace value near the threshold (allowing for the threshold's
own shift through the median and the MAD), a neighbour comparison of a candidate maximum, or a near-tie in the value
order _clean_max_indices sorts by.
"""
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np
from scipy.io import wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AVA_REFERENCE", "../reference"))

for _name in ("affinewarp", "umap", "h5py", "ava.plotting.tooltip_plot"):
    _stub = types.ModuleType(_name)
    _stub.ShiftWarping = _stub.tooltip_plot = None
    sys.modules[_name] = _stub

import template_cases as TC                                 # noqa: E402
import ava.segmenting.template_segmentation as TS           # noqa: E402

OUT = {}


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


class _MedianRecorder:
    """numpy for the reference module, except that the first np.median call keeps its argument"""

    def __init__(self):
        self.first = None

    def __getattr__(self, name):
        return getattr(np, name)

    def median(self, a, *args, **kwargs):
        if self.first is None:
            self.first = np.array(a, copy=True)
        return np.median(a, *args, **kwargs)


def ref_segment(path, template, p, num_mad, min_dt):
    """(segments, trace or None) of the reference's _segment_file"""
    rec = TS.np = _MedianRecorder()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, _, segs = TS._segment_file("unused", path, template, p, num_mad=num_mad, min_dt=min_dt)
    finally:
        TS.np = np
    return segs, rec.first


def ref_template(tmp, tag, exemplars, p, smoothing):
    d = os.path.join(tmp, tag)
    os.makedirs(d)
    for i, a in enumerate(exemplars):
        wavfile.write(os.path.join(d, "ex_%d.wav" % i), p['fs'], a)
    return TS.get_template(d, p, smoothing_kernel=smoothing, verbose=False)


def check_margins(name, r, tol, num_mad):
    m = 10.0 * tol
    med = np.median(r)
    thr = med + num_mad * (np.median(np.abs(r - med)) + TS.EPSILON)
    shift = (1.0 + 2.0 * num_mad) * m                     # the median moves by <= m, the MAD by <= 2 m
    d = np.abs(r - thr)
    if d.min() < m + shift:
        raise SystemExit("%s: trace value %.9g within %.3g of the threshold %.9g" % (name, r[d.argmin()], m + shift, thr))
    idx = np.argwhere(r > thr).flatten()[1:-1]
    cand = idx[2:len(idx) - 1]
    gap = np.abs(np.maximum(r[cand - 1], r[cand + 1]) - r[cand])
    if len(cand) and gap.min() < 2 * m:
        raise SystemExit("%s: a candidate maximum is within %.3g of its neighbour" % (name, gap.min()))
    mx = np.sort(r[cand[np.maximum(r[cand - 1], r[cand + 1]) < r[cand]]])
    if len(mx) > 1 and np.diff(mx).min() < 2 * m:
        raise SystemExit("%s: two maxima within %.3g of each other" % (name, np.diff(mx).min()))


def case(name, recipe, p, smoothing=(0.5, 0.5), num_mad=2.0, min_dt=0.05, tp=None, template_from=None):
    tp = dict(p) if tp is None else tp
    exemplars, files = TC.audio_of(recipe)
    entry = {'p': json.dumps(p), 'tp': json.dumps(tp), 'recipe': json.dumps(recipe),
             'opts': json.dumps(dict(smoothing=list(smoothing), num_mad=num_mad, min_dt=min_dt,
                                     template_from=template_from))}
    with tempfile.TemporaryDirectory() as tmp:
        tpl = ref_template(tmp, "ex", exemplars, tp, tuple(smoothing))
        tpl64 = ref_template(tmp, "ex64", [a.astype(np.float64) for a in exemplars], tp, tuple(smoothing))
        if template_from is None:
            entry['template'], entry['template64'] = tpl, tpl64
            gap = float(np.abs(tpl.astype(np.float64) - tpl64).max())
            entry['template_tol'] = max(4.0 * gap, 4.0 * ulp32(np.abs(tpl).max()))
        else:                                             # the same exemplars and template parameters as that case
            np.testing.assert_array_equal(OUT[template_from + '/template'], tpl)
        results = []
        for k, a in enumerate(files):
            path, path64 = os.path.join(tmp, "f%d.wav" % k), os.path.join(tmp, "f%d_64.wav" % k)
            wavfile.write(path, p['fs'], a)
            wavfile.write(path64, p['fs'], a.astype(np.float64))
            results.append((ref_segment(path, tpl, p, num_mad, min_dt), ref_segment(path64, tpl64, p, num_mad, min_dt)))
    gap, peak = 0.0, 0.0
    for (s, r), (s64, r64) in results:
        if r is not None:
            gap = max(gap, float(np.abs(r - r64).max()))
            peak = max(peak, float(np.abs(r).max()))
    tol = max(4.0 * gap, 4.0 * ulp32(peak))
    for k, ((s, r), (s64, r64)) in enumerate(results):
        entry['seg_%d' % k] = s
        np.testing.assert_array_equal(s, s64, err_msg="%s file %d: as given and float64 segments differ" % (name, k))
        if r is None:
            entry['nlags_%d' % k] = 0
            continue
        entry['nlags_%d' % k] = len(r)
        entry['trace_%d' % k] = r
        entry['trace64_%d' % k] = r64
        if np.all(r == 0.0) and np.all(r64 == 0.0):       # silent / saturated: exactly 0, on the device as well
            assert len(s) == 0
            continue
        check_margins("%s file %d" % (name, k), r, tol, num_mad)
    entry['tol'] = tol
    entry['n_files'] = len(files)
    for key, v in entry.items():
        OUT[name + '/' + key] = np.array(v) if not isinstance(v, np.ndarray) else v
    t = entry.get('template', OUT.get(str(template_from) + '/template'))
    print("%-26s F x L %3d x %3d  tol %.2e  segments per file %s" % (name, t.shape[0], t.shape[1], tol,
                                                                      [len(s) for (s, _), _ in results]))


def clean_hand_cases():
    rs = np.random.RandomState(5)
    names = []
    dt = np.float64(0.008)
    times = dt * np.arange(400)
    specs = [
        ('empty', np.array([], dtype='int'), None, 0.05),
        ('one', np.array([7]), None, 0.05),
        ('ties_small', np.array([3, 9, 12, 20, 26, 27, 40]), [0.5, 0.7, 0.7, 0.2, 0.7, 0.5, 0.1], 0.05),
        ('all_tied', np.arange(2, 60, 3), 'tied', 0.03),
        ('close_pairs', np.array([10, 11, 30, 32, 33, 70]), [1.0, 0.9, 0.3, 0.8, 0.8, 0.4], 0.02),
        ('many_ties', np.sort(rs.choice(np.arange(1, 399), size=120, replace=False)), 'levels', 0.05),
        ('random', np.sort(rs.choice(np.arange(1, 399), size=90, replace=False)), 'random', 0.1),
    ]
    for nm, idx, vals, min_dt in specs:
        values = np.zeros(400)
        if isinstance(vals, list):
            values[idx] = vals
        elif vals == 'tied':
            values[idx] = 0.25
        elif vals == 'levels':
            values[idx] = rs.randint(0, 4, size=len(idx)) * 0.125
        elif vals == 'random':
            values[idx] = rs.standard_normal(len(idx))
        out = TS._clean_max_indices(idx, times, values, min_dt=min_dt)
        name = "clean_" + nm
        for key, v in (('indices', idx), ('times', times), ('values', values), ('min_dt', np.array(min_dt)),
                       ('out', np.asarray(out))):
            OUT[name + '/' + key] = v
        names.append(name)
        print("%-26s %3d maxima -> %3d" % (name, len(idx), len(out)))
    return names


def main():
    F = TC.FINCH
    shift = dict(spec_min_val=F['spec_min_val'] - TC.LOG_INT16_SCALE, spec_max_val=F['spec_max_val'] - TC.LOG_INT16_SCALE)
    base = dict(kind='songs', fs=F['fs'], n_exemplars=3, n_songs=2, seconds=3.0, motif_seconds=0.3, salt=6006)
    names = []

    def add(name, **kw):
        case(name, **kw)
        names.append(name)

    add('songs_int16_512', recipe=dict(base, dtype='int16'), p=dict(F))
    add('songs_int32_256', recipe=dict(base, dtype='int32', salt=6106), p=dict(F, nperseg=256, noverlap=128),
        smoothing=(1.0, 2.0), num_mad=3.0, min_dt=0.2)
    add('songs_float32_1024', recipe=dict(base, dtype='float32', salt=6206), p=dict(F, nperseg=1024, noverlap=512, **shift),
        min_dt=0.2)
    add('songs_float64_512', recipe=dict(base, dtype='float64', salt=6306), p=dict(F, **shift), smoothing=(1.0, 2.0),
        num_mad=3.0)
    # edge files: shorter than nperseg, frames - L = 4 and 5, silent, and a whole song (template L is 41 frames)
    L, nstep = OUT['songs_int16_512/template'].shape[1], F['nperseg'] - F['noverlap']
    add('edges_int16_512', recipe=dict(base, kind='edge', dtype='int16', lengths=[511, (L + 3) * nstep, (L + 4) * nstep,
                                                                                  -64000, 96000]),
        p=dict(F), template_from='songs_int16_512')
    # loud noise with spec_min_val = -10, spec_max_val = -9: every bin clips to 1, the trace is exactly 0
    add('saturated_int16_512', recipe=dict(base, kind='edge', dtype='int16', lengths=['loud']),
        p=dict(F, spec_min_val=-10.0, spec_max_val=-9.0), tp=dict(F), template_from='songs_int16_512')
    OUT['case_names'] = np.array(json.dumps(names))
    OUT['hand_names'] = np.array(json.dumps(clean_hand_cases()))
    path = os.path.join(HERE, "template.npz")
    np.savez_compressed(path, **OUT)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
