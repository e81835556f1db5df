"""CPU tests of the amplitude segmentation's host side (ava_amd.segment): the golden's
integrity and margins, the host helpers against scipy, the greedy chain and duration filter on the golden traces,
and install()."""
import types

import numpy as np
import pytest

import segment_cases as SC
from ava_amd import segment as S


@pytest.fixture(scope="module")
def golden():
    return SC.load()


def _files(c):
    return range(int(c['n_files']))


def test_golden_integrity_and_margins(golden):
    cases, hand = golden
    assert len(cases) >= 19 and len(hand) >= 20
    dtypes = set()
    for name, c in cases.items():
        p, tol = c['p'], float(c['tol'])
        assert tol > 0
        for k in _files(c):
            if int(c['nframes_%d' % k]) == 0:
                assert len(c['on_%d' % k]) == 0
                continue
            tr = c['trace_%d' % k]
            dtypes.add(tr.dtype)
            assert tr.dtype == S.trace_dtype(np.dtype(c['recipe']['dtype']))
            assert np.abs(tr.astype(np.float64) - c['trace64_%d' % k]).max() <= tol / 4 + 1e-300 or \
                tol == pytest.approx(4 * float(np.spacing(np.float32(np.abs(tr).max()))))
            for key in ('th_1', 'th_2', 'th_3'):
                assert np.abs(tr.astype(np.float64) - p[key]).min() >= 10 * tol, (name, k, key)
            np.testing.assert_array_equal(c['on_%d' % k], c['on64_%d' % k])
            np.testing.assert_array_equal(c['off_%d' % k], c['off64_%d' % k])
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float64)}
    found = sum(len(cases[n]['on_0']) for n in cases)
    assert found >= 60
    # the edge cases hold files below nperseg, T = 2 and T = 3
    nfr = [int(cases['mouse_int16_edges']['nframes_%d' % k]) for k in range(6)]
    nfr += [int(cases['finch_float32_hop0_edges']['nframes_%d' % k]) for k in range(6)]
    assert 0 in nfr and 2 in nfr and 3 in nfr


def test_frame_count_dt_and_band_match_scipy(golden):
    from scipy.signal import stft
    cases, _ = golden
    for name in ('mouse_int16_sum', 'finch_int16_softmax', 'finch_float32_hop0_edges'):
        c = cases[name]
        p = c['p']
        audio = SC.audio_of(c['recipe'])
        for a in audio:
            n = int(S.frame_count(len(a), p['nperseg'], p['noverlap']))
            if len(a) < p['nperseg']:
                assert n == 0
                continue
            f, t, _ = stft(a[:len(a)], fs=p['fs'], nperseg=p['nperseg'], noverlap=p['noverlap'])
            assert n == len(t)
            assert S.frame_step(p['fs'], p['nperseg'], p['noverlap']) == t[1] - t[0]
            i1, i2, ff = S.band_indices(p)
            np.testing.assert_array_equal(ff, f)
            assert (i1, i2) == (np.searchsorted(f, p['min_freq']), np.searchsorted(f, p['max_freq']))
        if 'dt' in c:                                       # file 0 long enough for get_spec
            assert float(c['dt']) == S.frame_step(p['fs'], p['nperseg'], p['noverlap'])
            i1, i2, ff = S.band_indices(p)
            np.testing.assert_array_equal(c['f'], ff[i1:i2])


@pytest.mark.parametrize("sigma", [0.0, 1e-16, 0.4, 0.875, 3.41796875, 7.3])
def test_gaussian_weights_and_reflect_match_scipy(sigma):
    from scipy.ndimage import gaussian_filter
    w, r = S.gaussian_weights(sigma)
    assert r == (int(4.0 * sigma + 0.5) if sigma > 1e-15 else 0) and len(w) == 2 * r + 1
    assert abs(w.sum() - 1.0) < 1e-15
    rs = np.random.RandomState(3)
    for T in (1, 2, 3, 5, 40):
        x = rs.standard_normal(T)
        # the device's 'reflect' indexing (segment.hip: amp_smooth_kernel), period 2 T
        P = 2 * T
        m = (np.arange(T)[:, None] + np.arange(-r, r + 1)[None, :]) % P
        m = np.where(m >= T, P - 1 - m, m)
        got = (x[m] * w[None, :]).sum(axis=1)
        np.testing.assert_allclose(got, gaussian_filter(x, sigma), rtol=0, atol=1e-14)


def test_trace_dtype_and_thresholds():
    assert S.trace_dtype(np.int16) == np.float32 and S.trace_dtype(np.float32) == np.float32
    assert S.trace_dtype(np.int32) == np.float64 and S.trace_dtype(np.float64) == np.float64
    p = {'th_1': 0.1, 'th_2': 2, 'th_3': np.float64(0.3)}
    th = S.decide_thresholds(p, np.float32)
    assert th[0] == float(np.float32(0.1)) and th[1] == 2.0 and th[2] == 0.3      # np.float64 stays strong
    assert S.decide_thresholds(dict(p, th_3=0.3), np.float32)[2] == float(np.float32(0.3))
    assert S.decide_thresholds(p, np.float64) == [0.1, 2.0, 0.3]


def _candidates(a, p, dtype):
    """maxima and nearest stops with numpy (the reference's predicates), for the host chain"""
    th1, th2, th3 = S.decide_thresholds(p, dtype)
    a = a.astype(np.float64)
    T = len(a)
    mx = [i for i in range(1, T - 1) if a[i] > th3 and a[i] == a[i - 1:i + 2].max()]

    def stop(j):
        return a[j] < th1 or (a[j] < th2 and a[j] == a[j - 1:j + 2].min())
    left = [next((j for j in range(m - 1, 0, -1) if stop(j)), -1) for m in mx]
    right = [next((j for j in range(m + 1, T) if stop(j)), -1) for m in mx]
    return mx, left, right


def test_host_chain_and_duration_filter_on_golden_traces(golden):
    cases, hand = golden
    checked = 0
    for name, c in cases.items():
        p = c['p']
        dt = S.frame_step(p['fs'], p['nperseg'], p['noverlap'])
        for k in _files(c):
            if int(c['nframes_%d' % k]) == 0:
                continue
            tr = c['trace_%d' % k]
            on, off = S.duration_filter(*S.chain(*_candidates(tr, p, tr.dtype)), dt, p)
            assert all(type(x) is np.float64 for x in on + off)
            np.testing.assert_array_equal(np.array(on), c['on_%d' % k])
            np.testing.assert_array_equal(np.array(off), c['off_%d' % k])
            checked += 1
    for name, c in hand.items():
        tr, dt = c['trace'], np.float64(c['dt'])
        on, off = S.duration_filter(*S.chain(*_candidates(tr, c['p'], tr.dtype)), dt, c['p'])
        np.testing.assert_array_equal(np.array(on, dtype=np.float64), c['on'])
        np.testing.assert_array_equal(np.array(off, dtype=np.float64), c['off'])
        checked += 1
    assert checked >= 60


def test_unsupported_nperseg_is_refused():
    with pytest.raises(NotImplementedError):
        S._check_shape(400, 200)
    with pytest.raises(NotImplementedError):
        S._check_shape(4096, 2048)
    with pytest.raises(NotImplementedError):
        S._check_shape(512, 512)


def test_install_patches_a_stand_in_module():
    mod = types.ModuleType("amplitude_segmentation_stand_in")
    mod.get_onsets_offsets = lambda audio, p, return_traces=False: None
    assert S.install(mod) is mod
    assert mod.get_onsets_offsets is S.get_onsets_offsets
    ref_like = types.FunctionType(S.get_onsets_offsets.__code__, {}, "get_onsets_offsets")
    ref_like.__module__ = "ava.segmenting.amplitude_segmentation"
    assert S._is_amplitude_segmentation(ref_like) and S._is_amplitude_segmentation(S.get_onsets_offsets)
    assert not S._is_amplitude_segmentation(lambda a, p: ([], []))
