"""Amplitude segmentation on the MI355X (ava_amd.segment) against the reference's outputs
stored in tests/golden/segment.npz (tests/golden/make_golden_segment.py), and every kernel of csrc/segment.hip against
the numpy restatement of tests/segment_cases.py on seeded cases at the kernels' tile, grid and file edges."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import segment_cases as SC
from ava_amd import _lib, segment as S
from ava_amd.spec import DeviceAudio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return SC.load()


def _eq(got, want):
    assert len(got) == len(want)
    assert all(type(x) is np.float64 for x in got)
    np.testing.assert_array_equal(np.array(got, dtype=np.float64), want)


def test_trace_and_decisions_match_reference(golden):
    cases, _ = golden
    for name, c in cases.items():
        p, tol = c['p'], float(c['tol'])
        want_dtype = S.trace_dtype(np.dtype(c['recipe']['dtype']))
        for k, a in enumerate(SC.audio_of(c['recipe'])):
            res = S.get_onsets_offsets(a, p, return_traces=True)
            on, off, tr = res
            _eq(on, c['on_%d' % k])
            _eq(off, c['off_%d' % k])
            if int(c['nframes_%d' % k]) == 0:
                assert tr is None and on == [] and off == []
                continue
            got = tr[0]
            assert got.dtype == want_dtype, name
            ref = c['trace_%d' % k]
            assert got.shape == ref.shape
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
            assert err <= tol, (name, k, err, tol)
            if c['recipe']['dtype'] == 'float64':
                assert np.abs(got - c['trace64_%d' % k]).max() <= 1e-10, name
            on2, off2 = S.get_onsets_offsets(a, p)
            assert on2 == on and off2 == off


def test_decisions_on_hand_made_traces(golden):
    _, hand = golden
    for name, c in hand.items():
        on, off = S.onsets_offsets_from_trace(c['trace'], np.float64(c['dt']), c['p'])
        _eq(on, c['on'])
        _eq(off, c['off'])


def _mixed_files(c):
    """~64 files: the case's recordings and the edge files of the same dtype, interleaved"""
    return [a for _ in range(11) for a in c]


def test_batch_equals_per_file_and_golden(golden):
    cases, _ = golden
    rec, edge = cases['mouse_int16_sum'], cases['mouse_int16_edges']
    p = rec['p']
    src = [(a, rec, k) for k, a in enumerate(SC.audio_of(rec['recipe']))] + \
          [(a, edge, k) for k, a in enumerate(SC.audio_of(edge['recipe']))]
    files = [src[(7 * i) % len(src)] for i in range(64)]
    res = S.get_onsets_offsets_batch(DeviceAudio([a for a, _, _ in files]), p, return_traces=True)
    assert len(res) == 64
    for (a, c, k), (on, off, tr) in zip(files, res):
        _eq(on, c['on_%d' % k])
        _eq(off, c['off_%d' % k])
        one = S.get_onsets_offsets(a, p, return_traces=True)
        assert one[0] == on and one[1] == off
        if tr is None:
            assert one[2] is None
        else:
            np.testing.assert_array_equal(tr[0], one[2][0])
    plain = S.get_onsets_offsets_batch(DeviceAudio([a for a, _, _ in files]), p)
    assert [r[:2] for r in res] == [tuple(r) for r in plain]


def test_band_spectrogram_matches_reference_sample(golden):
    cases, _ = golden
    n = 0
    for name, c in cases.items():
        if 'spec_idx' not in c:
            continue
        a = SC.audio_of(c['recipe'])[0]
        spec, dt, f = S.get_spec(a, c['p'])
        assert spec.shape == tuple(c['spec_shape']) and spec.dtype == c['spec_val'].dtype, name
        assert dt == float(c['dt']) and type(dt) is np.float64
        np.testing.assert_array_equal(f, c['f'])
        err = np.abs(spec.reshape(-1)[c['spec_idx']].astype(np.float64) - c['spec_val'].astype(np.float64)).max()
        assert err <= float(c['spec_tol']), (name, err)
        n += 1
    assert n >= 17


def test_segment_directory_in_chunks(golden, tmp_path):
    from scipy.io import wavfile
    cases, _ = golden
    c = cases['mouse_int16_sum']
    p = dict(c['p'], algorithm=S.get_onsets_offsets)
    audio = SC.audio_of(c['recipe'])
    edge = SC.audio_of(cases['mouse_int16_edges']['recipe'])
    audio_dir, seg_dir = tmp_path / "audio", tmp_path / "segs"
    audio_dir.mkdir()
    names = []
    want = {}
    for i in range(6):
        k = i % 2
        nm = "rec_%02d" % i
        wavfile.write(str(audio_dir / (nm + ".wav")), p['fs'], audio[k])
        want[nm] = (c['on_%d' % k], c['off_%d' % k])
        names.append(nm)
    wavfile.write(str(audio_dir / "short.wav"), p['fs'], edge[0])
    want["short"] = (np.zeros(0), np.zeros(0))
    (audio_dir / "notes.txt").write_text("not audio")
    budget = audio[1].nbytes * 2                                        # two files per chunk: >= 3 chunks
    calls = []
    orig = S.get_onsets_offsets_batch

    def counting(dev_audio, q, return_traces=False):
        calls.append(len(dev_audio))
        return orig(dev_audio, q, return_traces)
    S.get_onsets_offsets_batch = counting
    try:
        S.segment(str(audio_dir), str(seg_dir), p, verbose=False, max_chunk_bytes=budget)
    finally:
        S.get_onsets_offsets_batch = orig
    assert len(calls) >= 3 and sum(calls) == 7
    assert sorted(os.listdir(seg_dir)) == sorted(n + ".txt" for n in want)
    for nm, (on, off) in want.items():
        text = (seg_dir / (nm + ".txt")).read_text()
        assert text.splitlines()[0] == "# Onsets/offsets for " + str(audio_dir / (nm + ".wav"))
        expect = "".join("%.5f %.5f\n" % (a, b) for a, b in zip(on, off))
        assert text.split("\n", 1)[1] == expect
    # the same files one per chunk, and through a per-file algorithm: identical files
    seg2 = tmp_path / "segs2"
    S.segment(str(audio_dir), str(seg2), p, verbose=False, max_chunk_bytes=1)
    seg3 = tmp_path / "segs3"
    S.segment(str(audio_dir), str(seg3), dict(p, algorithm=lambda a, q: S.get_onsets_offsets(a, q)), verbose=False)
    for nm in want:
        t = (seg_dir / (nm + ".txt")).read_text()
        assert (seg2 / (nm + ".txt")).read_text() == t and (seg3 / (nm + ".txt")).read_text() == t


def test_two_runs_are_bit_identical(golden):
    cases, _ = golden
    for name in ('mouse_int16_softmax', 'finch_float64_sum'):
        c = cases[name]
        dev = DeviceAudio(SC.audio_of(c['recipe']))
        r1 = S.get_onsets_offsets_batch(dev, c['p'], return_traces=True)
        r2 = S.get_onsets_offsets_batch(dev, c['p'], return_traces=True)
        for a, b in zip(r1, r2):
            assert a[0] == b[0] and a[1] == b[1]
            assert a[2][0].tobytes() == b[2][0].tobytes()


def test_c_abi_argument_checks():
    lib = _lib.load()
    dev = torch.device("cuda")
    audio = torch.zeros(4096, dtype=torch.int16, device=dev)
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    length = torch.full((1,), 4096, dtype=torch.int64, device=dev)
    fo = torch.tensor([0, 9], dtype=torch.int64, device=dev)
    win = torch.ones(1024, dtype=torch.float64, device=dev)
    gw = torch.ones(1, dtype=torch.float64, device=dev)
    trace = torch.empty(9, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.ava_amp_workspace_bytes(9), dtype=torch.uint8, device=dev)
    s = _lib.stream()
    P = lambda t: t.data_ptr()                                             # noqa: E731
    good = [P(audio), 0, P(off), P(length), P(fo), 1, 9, 1024, 512, P(win), 1.0, 10, 100, 2.0, 6.0, 0, 0.5, P(gw), 0, 0,
            P(trace), None, P(ws), ws.numel(), s]
    assert lib.ava_amp_trace(*good) == 0
    torch.cuda.synchronize()
    bad = {0: None, 4: None, 9: None, 20: None, 22: None,                  # null pointers
           7: 1000, 8: 1024,                                               # nperseg not a power of two; noverlap >= nperseg
           12: 10, 11: 200,                                                # empty band; band beyond nperseg / 2 + 1
           23: ws.numel() - 1}                                             # workspace too small
    for i, v in bad.items():
        args = list(good)
        args[i] = v
        if i == 11:
            args[12] = 600
        assert lib.ava_amp_trace(*args) == -1, i
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    buf = torch.empty((3, 9), dtype=torch.int64, device=dev)
    dgood = [P(trace), 0, P(fo), 1, 9, 0.1, 0.2, 0.3, P(cnt), P(buf[0]), P(buf[1]), P(buf[2]), 9, s]
    assert lib.ava_amp_decide(*dgood) == 0
    for i, v in {0: None, 2: None, 8: None, 9: None, 12: 8}.items():
        args = list(dgood)
        args[i] = v
        assert lib.ava_amp_decide(*args) == -1, i
    torch.cuda.synchronize()


# ---- the kernels against the numpy restatement of tests/segment_cases.py, at their own edges -------------------------
LD = np.longdouble


def _triples(trace, fo, files):
    """ava_amp_decide's (count, [maxima, left, right] sorted by maximum) through the C ABI"""
    lib = _lib.load()
    frames = trace.numel()
    f64 = trace.dtype == torch.float64
    th1, th2, th3 = S.decide_thresholds(SC.TH, np.float64 if f64 else np.float32)
    cnt = torch.full((1,), 77, dtype=torch.int64, device=trace.device)          # the entry point zeroes it
    buf = torch.full((3, frames), -7, dtype=torch.int64, device=trace.device)
    rc = lib.ava_amp_decide(trace.data_ptr(), 1 if f64 else 0, fo.data_ptr(), files, frames, th1, th2, th3,
                            cnt.data_ptr(), buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), frames,
                            _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    n = int(cnt.item())
    assert 0 <= n <= frames
    t = buf[:, :n].cpu().numpy()
    return n, t[:, np.argsort(t[0], kind='stable')]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", sorted(SC.DECISION_CASES))
def test_decisions_against_the_restatement(name, dtype):
    a, frame_off = SC.decision_case(name)
    want = SC.decision_want(name, dtype)
    files = len(frame_off) - 1
    trace = torch.from_numpy(a.astype(dtype)).cuda()
    fo = torch.from_numpy(np.array(frame_off)).cuda()
    n, (mx, left, right) = _triples(trace, fo, files)
    assert n == sum(len(w[0]) for w in want)
    cut = np.searchsorted(mx, frame_off)
    for f in range(files):
        s = slice(cut[f], cut[f + 1])
        assert (mx[s] - frame_off[f]).tolist() == want[f][0], (f, "maxima")
        assert left[s].tolist() == want[f][1], (f, "left")
        assert right[s].tolist() == want[f][2], (f, "right")
    assert S._decide(trace, np.array(frame_off), fo, SC.TH) == [S.chain(*w) for w in want]
    n2, again = _triples(trace, fo, files)
    assert n2 == n and np.array_equal(again, np.stack([mx, left, right]))


def test_decisions_of_a_batch_equal_each_file_alone():
    a, frame_off = SC.decision_case("boundaries")
    p = dict(SC.TH, min_dur=0.0, max_dur=1e9)
    dt = np.float64(1.0)
    for dtype in ("float32", "float64"):
        want = SC.decision_want("boundaries", dtype)
        trace = torch.from_numpy(a.astype(dtype)).cuda()
        fo = torch.from_numpy(np.array(frame_off)).cuda()
        batch = S._decide(trace, np.array(frame_off), fo, p)
        alone = 0
        for f in range(len(frame_off) - 1):
            one = a[frame_off[f]:frame_off[f + 1]].astype(dtype)
            chain = S.duration_filter(*S.chain(*want[f]), dt, p)
            assert S.duration_filter(*batch[f], dt, p) == chain
            if len(one) >= 3:
                assert S.onsets_offsets_from_trace(one, dt, p) == chain, f
                alone += 1
        assert alone >= 7


def _ratio(err, bound):
    return float((np.abs(err) / bound).max())


def _band_run(audio, p):
    """(trace, spec) of S._trace as host arrays, the frame offsets checked against frame_count"""
    N, noverlap = p['nperseg'], p['noverlap']
    dev = DeviceAudio(list(audio))
    T = S.frame_count([len(a) for a in audio], N, noverlap)
    frame_off = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    dt = S.frame_step(p['fs'], N, noverlap)
    trace, fo, spec = S._trace(dev, frame_off, p, dt, want_spec=True)
    torch.cuda.synchronize()
    i1, i2, _ = S.band_indices(p)
    assert trace.shape == (frame_off[-1],) and spec.shape == (i2 - i1, frame_off[-1]) and spec.dtype == torch.float64
    np.testing.assert_array_equal(fo.cpu().numpy(), frame_off)
    return dev, trace, spec, frame_off


def _check_band(tag, trace, spec, frame_off, want, p, float32):
    np.testing.assert_array_equal(frame_off, want['frame_off'])
    got_v, got = spec.cpu().numpy(), trace.cpu().numpy()
    assert got.dtype == (np.float32 if float32 else np.float64)
    vb, fb = SC.v_bound(want, p), SC.value_bound(want, p)
    if float32:
        fb = fb + 2.0 ** -24 * np.abs(want['value'])
    r_v, r_value = _ratio(got_v.astype(LD) - want['v'], vb), _ratio(got.astype(LD) - want['value'], fb)
    print("%s: device / bound: v %.3f value %.3f (%d x %d elements)" % ((tag, r_v, r_value) + got_v.shape))
    assert np.isfinite(got_v).all() and np.isfinite(got).all()
    assert r_v <= 1.0, tag                                                        # every element, none left out
    assert r_value <= 1.0, tag
    low, high = want['u'] < -vb, want['u'] > 1 + vb
    assert low.any() and high.any()
    assert (got_v[low] == 0.0).all() and (got_v[high] == 1.0).all()


@pytest.mark.parametrize("row,mode", SC.BAND_MODES)
def test_band_values_against_the_restatement(row, mode):
    p, want = SC.band_params(row, mode), SC.band_want(row, mode)
    dev, trace, spec, frame_off = _band_run(SC.band_audio(row), p)
    _check_band("%s %s" % (row, mode), trace, spec, frame_off, want, p, False)
    if mode == "sum":                                       # the template segmenter's band stage: the same bits
        from ava_amd import template_segmentation as TS
        tspec, fsum, tfo, tfo_host, _ = TS._band(dev, p)
        np.testing.assert_array_equal(tfo_host, frame_off)
        assert torch.equal(tspec, spec) and torch.equal(fsum, trace)


@pytest.mark.parametrize("dtype", SC.DTYPES)
@pytest.mark.parametrize("row", sorted(SC.DTYPE_ROWS))
def test_band_values_of_integer_and_float32_audio(row, dtype):
    mode = SC.DTYPE_ROWS[row]
    p, want = SC.band_params(row, mode, dtype), SC.band_want(row, mode, dtype)
    audio = SC.band_audio(row, dtype)
    assert audio[0].dtype == np.dtype(dtype)
    _, trace, spec, frame_off = _band_run(audio, p)
    _check_band("%s %s %s" % (row, mode, dtype), trace, spec, frame_off, want, p, dtype != "int32")


@pytest.mark.parametrize("dtype", ["float64", "int16"])
def test_smoothing_against_the_restatement(dtype):
    audio = SC.smooth_audio(dtype)
    same = [np.asarray(a, dtype=np.float64) for a in audio]                      # the same samples: the same fp64 raw trace
    p = dict(SC.SMOOTH_P)
    _, raw_t, _, frame_off = _band_run(same, p)                                  # radius 0: one fma with the weight 1
    raw = raw_t.cpu().numpy()
    assert np.diff(frame_off).tolist() == list(SC.SMOOTH_FRAMES) and raw.dtype == np.float64
    want_raw = SC.band_values(same, p)
    assert _ratio(raw.astype(LD) - want_raw['value'], SC.value_bound(want_raw, p)) <= 1.0
    assert raw.min() > 0.5 and raw.max() - raw.min() > 1.0
    dt = S.frame_step(p['fs'], p['nperseg'], p['noverlap'])
    worst = 0.0
    for radius in SC.SMOOTH_RADII:
        q = dict(p, smoothing_timescale=SC.smooth_timescale(radius))
        w, r = S.gaussian_weights(q['smoothing_timescale'] / dt)
        assert r == radius
        _, trace, _, _ = _band_run(audio, q)
        got = trace.cpu().numpy()
        assert got.dtype == (np.float32 if dtype == "int16" else np.float64)
        want = SC.smoothed(raw, frame_off, w, r)
        bound = SC.smooth_bound(raw, frame_off, w, r, want, float32=dtype == "int16")
        ratio = _ratio(got.astype(LD) - want, bound)
        worst = max(worst, ratio)
        assert ratio <= 1.0, radius
    print("smoothing %s: device / bound %.3f" % (dtype, worst))


def test_unsupported_nperseg_raises():
    p = dict(SC.MOUSE, nperseg=1000, noverlap=500, th_1=2.0, th_2=5.0, th_3=10.0, softmax=False)
    with pytest.raises(NotImplementedError):
        S.get_onsets_offsets(np.zeros(5000, dtype=np.int16), p)
