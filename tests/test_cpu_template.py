"""CPU tests of the template segmentation's host side (ava_amd.template_segmentation): the
golden's integrity and margins, the decision stage on the reference's stored traces, the _clean_max_indices mirror,
the writer of segment_files, install() and the argument checks that need no device."""
import os
import sys
import types

import numpy as np
import pytest

import template_cases as TC
from ava_amd import segment as S
from ava_amd import template_segmentation as TS


@pytest.fixture(scope="module")
def golden():
    return TC.load()


def _template(cases, c):
    src = c['opts']['template_from']
    return cases[src]['template'] if src else c['template']


def test_module_imports_without_the_reference_extras():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys\nfor n in ('affinewarp', 'umap', 'h5py', 'bokeh'): sys.modules[n] = None\n"
            "import ava_amd.template_segmentation as T\nprint(T.get_template.__module__)")
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable] + flags + ["-c", code], cwd=root, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "ava_amd.template_segmentation"


def test_golden_integrity_and_margins(golden):
    cases, hand = golden
    assert len(cases) >= 6 and len(hand) >= 7
    dtypes, npersegs, kernels, mads, dts = set(), set(), set(), set(), set()
    zero_files, lag_counts = 0, []
    for name, c in cases.items():
        p, o, tol = c['p'], c['opts'], float(c['tol'])
        dtypes.add(c['recipe']['dtype'])
        npersegs.add(p['nperseg'])
        kernels.add(tuple(o['smoothing']))
        mads.add(o['num_mad'])
        dts.add(o['min_dt'])
        tpl = _template(cases, c)
        assert tpl.dtype == S.trace_dtype(np.dtype(c['recipe']['dtype']))
        if o['template_from'] is None:
            gap = np.abs(tpl.astype(np.float64) - c['template64']).max()
            assert 4 * gap <= float(c['template_tol']) and float(c['template_tol']) > 0
        for k in range(int(c['n_files'])):
            n = int(c['nlags_%d' % k])
            lag_counts.append(n)
            if n == 0:
                assert c['seg_%d' % k].shape == (0, 2)
                continue
            r, r64 = c['trace_%d' % k], c['trace64_%d' % k]
            assert r.dtype == np.float64 and r.shape == (n,) and r64.shape == (n,)
            assert 4 * np.abs(r - r64).max() <= tol
            if not r.any():
                zero_files += 1
                continue
            m = 10 * tol
            med = np.median(r)
            thr = med + o['num_mad'] * (np.median(np.abs(r - med)) + TS.EPSILON)
            assert np.abs(r - thr).min() >= m * (2 + 2 * o['num_mad']), (name, k)
    assert dtypes == {'int16', 'int32', 'float32', 'float64'}
    assert npersegs == {256, 512, 1024}
    assert len(kernels) == 2 and len(mads) == 2 and len(dts) == 2
    assert zero_files >= 2 and 5 in lag_counts and 0 in lag_counts
    assert sum(len(c['seg_%d' % k]) for c in cases.values() for k in range(int(c['n_files']))) >= 60


def test_edge_lengths_are_what_the_recipe_says(golden):
    cases, _ = golden
    c = cases['edges_int16_512']
    p = c['p']
    L = _template(cases, c).shape[1]
    _, files = TC.audio_of(c['recipe'])
    T = S.frame_count([len(a) for a in files], p['nperseg'], p['noverlap'])
    assert len(files[0]) < p['nperseg'] and T[1] - L == 4 and T[2] - L == 5
    assert not files[3].any()
    assert [int(c['nlags_%d' % k]) for k in range(5)] == [0, 0, 5, T[3] - L, T[4] - L]


def test_decisions_on_reference_traces(golden):
    cases, _ = golden
    checked = 0
    for name, c in cases.items():
        p, o = c['p'], c['opts']
        dt = S.frame_step(p['fs'], p['nperseg'], p['noverlap'])
        L = _template(cases, c).shape[1]
        for k in range(int(c['n_files'])):
            if int(c['nlags_%d' % k]) == 0:
                continue
            for key in ('trace_%d', 'trace64_%d'):
                seg = TS.segments_from_trace(c[key % k], dt, L, o['num_mad'], o['min_dt'])
                assert seg.dtype == np.float64 and seg.shape[1] == 2
                np.testing.assert_array_equal(seg, c['seg_%d' % k], err_msg=name)
            checked += 1
    assert checked >= 11


def _clean_quadratic(old_indices, old_times, values, min_dt):
    """template_segmentation.py:793-815 restated as written: O(k^2)"""
    if len(old_indices) <= 1:
        return old_indices
    order = old_indices[np.argsort(values[old_indices])]
    kept = [order[0]]
    for i in order[1:]:
        if all(not abs(old_times[j] - old_times[i]) < min_dt for j in kept):
            kept.append(i)
    return np.sort(np.array(kept))


def test_clean_max_indices_matches_hand_cases(golden):
    _, hand = golden
    for name, c in hand.items():
        got = TS._clean_max_indices(c['indices'], c['times'], c['values'], min_dt=float(c['min_dt']))
        assert got.dtype == c['out'].dtype or len(got) == 0, name
        np.testing.assert_array_equal(got, c['out'], err_msg=name)


def test_clean_max_indices_matches_quadratic_restatement():
    rs = np.random.RandomState(17)
    times = np.float64(0.008) * np.arange(2000)
    for trial in range(200):
        k = rs.randint(0, 150)
        idx = np.sort(rs.choice(np.arange(1, 1999), size=k, replace=False))
        values = np.zeros(2000)
        values[idx] = rs.randint(0, 1 + trial % 6, size=k) * 0.25 + (rs.rand(k) if trial % 3 == 0 else 0)
        min_dt = [0.0, 0.008, 0.02, 0.05, 0.3][trial % 5]
        np.testing.assert_array_equal(TS._clean_max_indices(idx, times, values, min_dt),
                                      _clean_quadratic(idx, times, values, min_dt))


@pytest.mark.filterwarnings("ignore:loadtxt")
def test_segment_files_writer_and_dict(golden, tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    cases, _ = golden
    c = cases['edges_int16_512']
    p = c['p']
    _, files = TC.audio_of(c['recipe'])
    audio_dirs = [tmp_path / "a0", tmp_path / "a1"]
    seg_dirs = [str(tmp_path / "s0"), str(tmp_path / "s1")]
    want = {}
    for d in audio_dirs:
        d.mkdir()
    for k, a in enumerate(files):
        fn = str(audio_dirs[k % 2] / ("f%d.wav" % k))
        wavfile.write(fn, p['fs'], a)
        want[fn] = c['seg_%d' % k]
    (audio_dirs[0] / "notes.txt").write_text("not audio")
    calls = []

    def fake_batch(dev_audio, template, q, num_mad=2.0, min_dt=0.05, min_extra_time_bins=5, names=None):
        calls.append(list(names))
        return [want[n] for n in names]
    monkeypatch.setattr(TS, "segment_batch", fake_batch)
    monkeypatch.setattr(TS, "DeviceAudio", lambda audio, device="cuda": audio)
    res = TS.segment_files([str(d) for d in audio_dirs], seg_dirs, None, p, max_chunk_bytes=1)
    assert sorted(res) == sorted(want) and len(calls) == len(files)
    out = capsys.readouterr().out
    n = sum(len(s) for s in want.values())
    assert out == "Segmenting files. n = %d\n\tFound %d segments.\n\tDone.\n" % (len(files), n)
    for fn, segs in want.items():
        assert res[fn] is segs
        d = seg_dirs[0] if os.path.dirname(fn).endswith("a0") else seg_dirs[1]
        text = open(os.path.join(d, os.path.basename(fn)[:-4] + ".txt")).read()
        assert text == "".join("%.5f %.5f\n" % (a, b) for a, b in segs)
    back = TS.read_segment_decisions([str(d) for d in audio_dirs], seg_dirs, verbose=False)
    for fn, segs in want.items():
        np.testing.assert_allclose(back[fn], segs, rtol=0, atol=5e-6)
        assert back[fn].shape == (len(segs), 2)


def test_install_patches_a_stand_in_module():
    mod = types.ModuleType("template_segmentation_stand_in")
    mod.get_template = mod.segment_files = mod._segment_file = None
    assert TS.install(mod) is mod
    assert mod.get_template is TS.get_template and mod.segment_files is TS.segment_files
    assert mod._segment_file is TS._segment_file


def test_argument_checks_without_device():
    from ava_amd.spec import DeviceAudio
    a = DeviceAudio([np.zeros(5000, dtype=np.int16)], device="cpu")
    tpl = np.zeros((153, 10))
    for nperseg, noverlap in ((400, 200), (4096, 2048), (32, 16), (512, 512)):
        with pytest.raises(NotImplementedError):
            TS.segment_batch(a, tpl, dict(TC.FINCH, nperseg=nperseg, noverlap=noverlap))
        with pytest.raises(NotImplementedError):
            TS.xcorr_batch(a, tpl, dict(TC.FINCH, nperseg=nperseg, noverlap=noverlap))
    with pytest.raises(ValueError):
        TS.segment_batch(a, np.zeros(10), TC.FINCH)                          # not [F, L]
    with pytest.raises(ValueError):
        TS.segment_batch(a, tpl, dict(TC.FINCH, min_freq=5000, max_freq=4000))   # empty band
    with pytest.raises(ValueError):
        TS.get_template_from_audio([np.zeros(100, dtype=np.int16)], TC.FINCH)    # shorter than nperseg
