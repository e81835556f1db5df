"""Amplitude segmentation on the MI355X (ava_amd.segment) against the reference's outputs
stored in tests/golden/segment.npz (tests/golden/make_golden_segment.py)."""
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


def test_unsupported_nperseg_raises():
    p = dict(SC.MOUSE, nperseg=1000, noverlap=500, th_1=2.0, th_2=5.0, th_3=10.0, softmax=False)
    with pytest.raises(NotImplementedError):
        S.get_onsets_offsets(np.zeros(5000, dtype=np.int16), p)
