"""CPU tests of the amplitude segmentation's host side (ava_amd.segment): the golden's
integrity and margins, the host helpers against scipy, the greedy chain and duration filter on the golden traces,
install(), and the seeded edge cases of tests/segment_cases.py: that each case has the edge it is built for, that the
numpy restatement agrees with scipy within half of every bound, and that wrong variants of it break the bounds."""
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


_candidates = SC.candidates


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


# ---- the seeded decision cases ---------------------------------------------------------------------------------------
DT = ("float32", "float64")
TH1, TH2, TH3 = SC.TH['th_1'], SC.TH['th_2'], SC.TH['th_3']


@pytest.mark.parametrize("dtype", DT)
def test_far_stops_has_every_side_rule_and_distance(dtype):
    a, fo = SC.decision_case("far_stops")
    assert len(fo) == 2
    mx, left, right = SC.decision_want("far_stops", dtype)[0]
    seen = set()
    for m, lo, hi in zip(mx, left, right):
        for side, s in (("left", lo), ("right", hi)):
            assert s >= 1
            between = a[min(m, s) + 1:max(m, s)]
            assert (between >= TH1).all() and (np.diff(a[min(m, s):max(m, s) + 1]) != 0).all()
            assert (np.diff(between) > 0).all() or (np.diff(between) < 0).all() or len(between) < 2
            seen.add((side, 1 if a[s] < TH1 else 2, abs(m - s)))
    assert seen == {(side, rule, D) for side in ("left", "right") for rule in (1, 2) for D in SC.DISTANCES}
    assert set(SC.DISTANCES) == {1, 2, 63, 64, 65, 127, 128, 129, 300}


@pytest.mark.parametrize("dtype", DT)
def test_many_maxima_exceeds_the_capped_grid(dtype):
    a, fo = SC.decision_case("many_maxima")
    mx, left, right = SC.decision_want("many_maxima", dtype)[0]
    assert len(a) == 20001 and len(mx) >= 9000 > 8192
    assert mx[0] == 1 and left[0] == -1 and min(left[1:]) >= 1 and min(right) >= 1
    assert len(set(np.subtract(mx, left)[1:])) >= 3 and len(set(np.subtract(right, mx))) >= 3


@pytest.mark.parametrize("dtype", DT)
def test_boundaries_has_its_edges(dtype):
    a, fo = SC.decision_case("boundaries")
    want = SC.decision_want("boundaries", dtype)
    T = np.diff(fo)
    files = [a[fo[f]:fo[f + 1]] for f in range(len(T))]
    assert len(T) >= 12 and (T >= 0).all()
    assert T[0] == 0 and T[-1] == 0 and any(T[f] == 0 and T[:f].any() and T[f:].any() for f in range(len(T)))
    assert {1, 2, 3} <= set(T.tolist())
    # a maximum at T - 2 without a right stop, the next file starting below th_1
    mx, left, right = want[5]
    assert mx == [T[5] - 2] and right == [-1] and left == [1] and files[6][0] < TH1
    # the mirror: the file before ends below th_1, the maximum at 1 has no left stop; frame 0 itself below th_1 in file 6
    assert files[6][-1] < TH1 and want[7][0][0] == 1 and want[7][1][0] == -1
    assert want[6][0] == [1] and want[6][1] == [-1] and files[6][0] < TH1
    # the last frame is a stop by the th_2 rule through the clipped slice alone
    mx, left, right = want[9]
    last = files[9][-1]
    assert right == [T[9] - 1] and TH1 <= last < TH2 and files[9][-2] > last > files[10][0]
    # first and last frame above every neighbour, the adjacent files' included: not maxima
    f11 = files[11]
    assert f11[0] > max(f11[1], files[10][-1]) and f11[-1] > max(f11[-2], files[12][0]) and min(f11[0], f11[-1]) > TH3
    assert want[11][0] == [2]
    for f in np.flatnonzero(T < 3):
        assert want[f] == ([], [], [])
    assert want[4] == ([1], [-1], [2])


@pytest.mark.parametrize("dtype", DT)
def test_plateaus_nan_has_its_ties_and_nans(dtype):
    a, _ = SC.decision_case("plateaus_nan")
    mx, left, right = SC.decision_want("plateaus_nan", dtype)[0]
    assert (mx, left, right) == ([1, 2, 8, 14, 20], [-1, -1, 6, 13, 18], [3, 3, 9, 18, 25])
    assert a[1] == a[2] and a[5] == a[6] and TH1 <= a[5] < TH2                      # tied maxima, tied minima
    nan = np.flatnonzero(np.isnan(a)).tolist()
    assert nan == [11, 17, 22]
    assert a[10] > TH3 and a[12] > TH3 and a[10] > a[9] and a[12] > a[13]           # NaN at / next to a would-be maximum
    assert a[16] < TH2 and a[16] < a[15] and a[18] < TH1                            # next to a would-be stop, and to a stop
    assert a[23] < TH2 and a[23] < a[24]


@pytest.mark.parametrize("dtype", DT)
def test_waves_fill_the_waves_of_a_workgroup_unevenly(dtype):
    a, _ = SC.decision_case("waves")
    mx, left, right = SC.decision_want("waves", dtype)[0]
    assert len(a) == 1100 and mx == sorted(SC.WAVE_MAXIMA)
    per_wave = np.bincount(np.array(mx) // 64, minlength=18)
    assert per_wave[:4].tolist() == [32, 0, 1, 1] and per_wave[8:12].tolist() == [32, 0, 1, 0]
    assert set(per_wave.tolist()) == {0, 1, 32}
    lanes = set(m % 64 for m in mx)
    assert 0 in lanes and 63 in lanes and {255, 256, 1023, 1024, 1098} <= set(mx)
    assert -1 in left and min(right) >= 1 and right[-1] == 1099


@pytest.mark.parametrize("name", sorted(SC.DECISION_CASES))
@pytest.mark.parametrize("dtype", DT)
def test_candidates_equal_the_references_while_loops(name, dtype):
    a, fo = SC.decision_case(name)
    want = SC.decision_want(name, dtype)
    for f in range(len(fo) - 1):
        assert SC.while_loop_candidates(a[fo[f]:fo[f + 1]], SC.TH, dtype) == want[f]
    assert SC.wrong_candidates(a.astype(dtype), fo, SC.TH, np.dtype(dtype), None) == want


@pytest.mark.parametrize("wrong", ["span64", "stop0", "across"])
def test_decision_cases_tell_wrong_kernels_apart(wrong):
    differ = []
    for name in sorted(SC.DECISION_CASES):
        a, fo = SC.decision_case(name)
        if SC.wrong_candidates(a, fo, SC.TH, np.dtype(np.float64), wrong) != SC.decision_want(name, "float64"):
            differ.append(name)
    assert differ, wrong
    if wrong == "span64":
        assert "far_stops" in differ
    else:
        assert "boundaries" in differ


# ---- the seeded band cases -------------------------------------------------------------------------------------------
def _ratio(err, bound):
    return float((np.abs(err) / bound).max())


@pytest.mark.parametrize("row", sorted(SC.BAND_ROWS))
def test_band_rows_have_their_edges(row):
    c = SC.BAND_ROWS[row]
    N, hop = c['nperseg'], c['hop']
    audio = SC.band_audio(row)
    assert [len(a) for a in audio][1:] == [N, N - 1] and (len(audio[0]) % hop != 0 or hop == 1)
    assert all(a.dtype == np.float64 for a in audio)
    x = audio[0]
    zero = np.flatnonzero(x == 0.0)
    assert len(zero) > N + hop and (np.diff(zero) == 1).all()
    p = SC.band_params(row, c['modes'][0])
    assert S.band_indices(p)[:2] == (c['k0'], c['k1'])
    want = SC.band_want(row, c['modes'][0])
    T = S.frame_count([len(a) for a in audio], N, N - hop)
    assert T[2] == 0 and T[1] >= 2
    np.testing.assert_array_equal(want['frame_off'], np.concatenate([[0], np.cumsum(T)]))
    assert want['v'].shape == (c['k1'] - c['k0'], T.sum())
    if row == "n64_hop64_4200":
        assert T[0] >= 4200
    if row == "n2048_hop1365_full":
        assert T.sum() <= 24
    if row == "n512_hop171_full":
        assert want['v'].shape[0] > 256
    if row == "n64_hop1_b3_20":
        assert want['v'].shape[0] < 64


@pytest.mark.parametrize("row,mode,dtype", [(r, m, "float64") for r, m in SC.BAND_MODES] +
                         [(r, m, d) for r, m in SC.DTYPE_ROWS.items() for d in SC.DTYPES])
def test_band_cases_use_the_clips_and_the_inside(row, mode, dtype):
    want = SC.band_want(row, mode, dtype)
    u, bound = want['u'], SC.v_bound(want, SC.band_params(row, mode, dtype))
    assert ((u > bound) & (u < 1 - bound)).mean() >= 0.5
    assert (u < -bound).mean() >= 0.01 and (u > 1 + bound).mean() >= 0.01
    if dtype != "float64":
        audio = SC.band_audio(row, dtype)
        assert all(a.dtype == np.dtype(dtype) for a in audio)
        assert max(np.abs(a).max() for a in audio) > (0.01 if dtype == "float32" else 1000)


@pytest.mark.parametrize("row,mode", SC.BAND_MODES)
def test_scipy_stays_within_half_of_every_bound(row, mode):
    """scipy's own fp64 stft, the arithmetic of the reference, against the longdouble restatement"""
    from scipy.signal import stft
    p, want = SC.band_params(row, mode), SC.band_want(row, mode)
    c = SC.BAND_ROWS[row]
    Z = [stft(a, fs=p['fs'], nperseg=p['nperseg'], noverlap=p['noverlap'])[2][c['k0']:c['k1']]
         for a in SC.band_audio(row) if len(a) >= p['nperseg']]
    Z = np.concatenate(Z, axis=1)
    assert Z.dtype == np.complex128 and Z.shape == want['v'].shape
    r_spec = _ratio(np.hypot(Z.real - want['re'], Z.imag - want['im']), SC.spectrum_bound(want, p)[None, :] + 1e-300)
    v = np.clip((np.log(np.abs(Z) + S.EPSILON) - p['spec_min_val']) / (p['spec_max_val'] - p['spec_min_val']), 0, 1)
    r_v = _ratio(v - want['v'], SC.v_bound(want, p))
    if mode == "softmax":
        e = np.exp(v / p['temperature'])
        value = np.sum(v * e, axis=0) / (np.sum(e, axis=0) + S.EPSILON)
    else:
        value = np.sum(v, axis=0)
    r_value = _ratio(value - want['value'], SC.value_bound(want, p))
    print("%s %s: scipy / bound: spectrum %.3f v %.3f value %.3f" % (row, mode, r_spec, r_v, r_value))
    assert r_spec <= 0.5 and r_v <= 0.5 and r_value <= 0.5


@pytest.mark.parametrize("wrong", ["hann", "nyquist", "eps", "lastbin", "left"])
def test_wrong_band_restatements_break_the_bounds(wrong):
    """a bound loose enough to pass these would hide a wrong kernel"""
    worst = 0.0
    for row, mode in (("n64_hop64_full", "sum"), ("n64_hop64_full", "softmax"), ("n128_hop43_full", "softmax")):
        p, want = SC.band_params(row, mode), SC.band_want(row, mode)
        got = SC.band_values(SC.band_audio(row), p, wrong=wrong)
        if wrong == "lastbin":
            worst = max(worst, _ratio(got['value'] - want['value'], SC.value_bound(want, p)))
        else:
            worst = max(worst, _ratio(got['v'] - want['v'], SC.v_bound(want, p)))
    assert worst >= 10.0, (wrong, worst)


def _smooth_inputs():
    from ava_amd import synthetic as syn
    fo = np.concatenate([[0], np.cumsum(SC.SMOOTH_FRAMES)]).astype(np.int64)
    return 3.0 + syn.gauss(int(fo[-1]), 5500), fo


@pytest.mark.parametrize("radius", SC.SMOOTH_RADII)
def test_smoothed_matches_scipy_and_its_mirror_variant_breaks_the_bound(radius):
    from scipy.ndimage import gaussian_filter
    raw, fo = _smooth_inputs()
    p = dict(SC.SMOOTH_P, smoothing_timescale=SC.smooth_timescale(radius))
    dt = S.frame_step(p['fs'], p['nperseg'], p['noverlap'])
    sigma = p['smoothing_timescale'] / dt
    w, r = S.gaussian_weights(sigma)
    assert r == radius and dt == 1.0
    assert S.frame_count([64 * (T - 1) for T in SC.SMOOTH_FRAMES], 64, 0).tolist() == list(SC.SMOOTH_FRAMES)
    got = SC.smoothed(raw, fo, w, r)
    for f, T in enumerate(SC.SMOOTH_FRAMES):
        x = raw[fo[f]:fo[f + 1]]
        np.testing.assert_allclose(got[fo[f]:fo[f + 1]].astype(np.float64), gaussian_filter(x, sigma, mode='reflect'),
                                   rtol=0, atol=1e-14)
    bound = SC.smooth_bound(raw, fo, w, r)
    assert _ratio(SC.wrong_smoothed(raw, fo, w, r) - got, bound) >= 10.0
    assert float(bound.max()) < 1e-13
