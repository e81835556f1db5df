"""CPU tests of the integer-shift fit: no kernel runs here.  They pin the numpy restatement of
tests/shiftfit_cases.py, the oracle of tests/test_gpu_shiftfit.py, to the model's definition and show that it recovers
planted shifts; and they check the host halves of ``segment_sylls_from_songs`` / ``segment_sylls_from_warped_songs``
(slicing, edge padding, the written files) against the plain statement of the reference's lines in the same module."""
import os

import numpy as np
import pytest
import torch

import shiftfit_cases as SC


@pytest.fixture(scope="module")
def fits():
    out = {}
    for case in SC.CASES:
        x, sh = SC.planted(*case)
        out[case] = (x, sh, SC.fit(x, SC.MAXLAG, SC.SMOOTHNESS, SC.ITERATIONS))
    return out


@pytest.mark.parametrize("case", SC.CASES)
def test_restatement_recovers_planted_shifts(case, fits):
    """the fitted shifts are the planted ones up to one offset common to all renditions; they are a fixed point from
    iteration 1 on; neither half-step raises J"""
    x, sh, r = fits[case]
    offsets = set((r['shifts'] - sh).tolist())
    print(case, "offset", offsets, "J", r['J'][:3])
    assert len(offsets) == 1
    assert all((h == r['history'][1]).all() for h in r['history'][1:])
    assert not (r['history'][0] == 0).all()
    steps = [v for pair in zip(r['J_template'], r['J']) for v in pair]      # template step, shift step, template step, ...
    assert all(b <= a * (1 + 1e-13) for a, b in zip(steps[:-1], steps[1:]))
    assert all(b <= a for a, b in zip(r['J'][:-1], r['J'][1:]))


@pytest.mark.parametrize("case", SC.CASES)
def test_best_lag_is_clear_of_the_second_best(case, fits):
    """what makes exact shift equality a fair demand of the device: the best loss of every rendition in every iteration
    lies a relative 1e-8 or more below the second best, far above the 4 F T 2^-52 the two sums may differ by"""
    r = fits[case][2]
    print(case, "smallest relative gap %.3e" % r['gap'])
    assert r['gap'] >= 1e-8
    assert 4 * case[1] * case[2] * 2.0 ** -52 < 1e-3 * r['gap']


def test_lag_order():
    from ava_amd import shift_fit
    assert SC.lag_order(0).tolist() == [0]
    assert SC.lag_order(3).tolist() == [0, -1, 1, -2, 2, -3, 3]
    for L in (0, 1, 2, 7, 40):
        got = shift_fit.lag_order(L)
        assert got.dtype == np.int64 and got.tolist() == SC.lag_order(L).tolist()
        assert sorted(got.tolist()) == list(range(-L, L + 1))
    with pytest.raises(ValueError):
        shift_fit.lag_order(-1)


def test_constant_and_nan_traces_keep_shift_zero():
    """an all-zero trace ties at every lag and candidate 0 wins; a NaN loss never wins"""
    x, _ = SC.planted(6, 1, 40, 4, 5200)
    x[2] = 0.0
    r = SC.fit(x, 0.2, 10.0, 4)
    assert r['shifts'][2] == 0 and all(h[2] == 0 for h in r['history'])
    losses = np.array([[np.nan, 2.0, 1.0, 1.0], [np.nan] * 4, [3.0, 3.0, np.nan, 3.0]])
    assert SC.argmin(losses).tolist() == [2, 0, 0]


@pytest.mark.parametrize("T,K,lam", [(3, 1, 10.0), (4, 5, 0.5), (9, 40, 10.0), (37, 7, 0.0)])
def test_banded_A_against_dense(T, K, lam):
    ab = SC.banded_A(T, K, lam)
    A = SC.dense_A(T, K, lam)
    dense = np.zeros((T, T))
    for u in range(3):                                   # ab[2 - u, j] = A[j - u, j]
        for j in range(u, T):
            dense[j - u, j] = dense[j, j - u] = ab[2 - u, j]
    assert np.array_equal(dense, A)
    assert np.array_equal(A, A.T) and np.count_nonzero(np.triu(A, 3)) == 0
    mbar = np.linspace(-1, 2, 2 * T).reshape(2, T) ** 2
    m, _ = SC.template(np.tile(mbar, (K, 1, 1)), np.zeros(K, dtype=int), lam)
    assert np.abs(m @ A - mbar).max() <= 1e-12 * (1 + 16 * lam)


# ---- the host halves of the segmenters -----------------------------------------------------------------------------

FS = 1000


def _song_fixture(tmp_path):
    """two directories; recordings of 2 s at 1 kHz; segments that start before the file, end behind it, lie inside it
    (with onsets whose ``fs * t`` truncates and rounds differently), and one recording without song"""
    dirs = [str(tmp_path / "audio_a"), str(tmp_path / "audio_b")]
    names = [os.path.join(dirs[0], "one.wav"), os.path.join(dirs[0], "two.wav"), os.path.join(dirs[1], "three.wav")]
    audio_of = {fn: (FS, np.arange(2000, dtype=np.int16) + 7 * i) for i, fn in enumerate(names)}
    song_segs = {names[0]: np.array([[0.02, 0.5206], [0.7007, 1.2013], [1.48, 1.9806]]),
                 names[1]: np.zeros((0, 2)),
                 names[2]: np.array([[0.3339, 0.8345]])}
    return dirs, names, audio_of, song_segs


def test_song_slices_truncate_like_int(tmp_path):
    from ava_amd import template_segmentation as ts
    dirs, names, audio_of, song_segs = _song_fixture(tmp_path)
    shoulder = 0.05
    info = ts._song_slices(song_segs, shoulder, lambda fn: audio_of[fn])
    rows, empty = SC.song_slices(song_segs, audio_of, shoulder)
    assert info['empty_audio_files'] == empty == [names[1]]
    assert info['fns'] == [r[0] for r in rows] and info['song_onsets'] == [r[1] for r in rows]
    assert info['edge'] == [r[4] for r in rows] == [True, False, True, False]
    dt = 0.004
    for k, (fn, onset, i1, i2, edge) in enumerate(rows):
        audio = audio_of[fn][1]
        assert np.array_equal(info['slices'][k], audio[max(i1, 0):i2])
        assert ts._edge_bins(info['pad_secs'][k], dt) == SC.edge_bins(i1, i2, len(audio), FS, dt)
    # int() truncates where round() would go up, and towards zero below zero
    assert rows[1][2] == int(FS * (0.7007 - 0.05)) == 650 and int(round(FS * (0.7007 - 0.05))) == 651
    assert rows[0][2] < 0 and rows[0][4] and info['slices'][0][0] == audio_of[names[0]][1][0]    # an edge; starts at sample 0
    near = ts._song_slices({names[0]: np.array([[0.0496, 0.55]])}, shoulder, lambda fn: audio_of[fn])
    assert near['edge'] == [False] and near['pad_secs'][0][0] == 0          # int(-0.4) = 0: not before the file
    assert ts._edge_bins(info['pad_secs'][0], dt) == (8, 0)                 # round(0.03 / 0.004) = round(7.5) = 8
    assert ts._edge_bins(info['pad_secs'][2], dt) == (0, 8)                 # 30 samples behind the end


def test_syllable_segment_files_byte_for_byte(tmp_path):
    from ava_amd import template_segmentation as ts
    dirs, names, audio_of, song_segs = _song_fixture(tmp_path)
    rows, empty = SC.song_slices(song_segs, audio_of, 0.05)
    fns, onsets = [r[0] for r in rows], [r[1] for r in rows]
    shifts = np.array([0, -3, 7, 2])
    quantiles = [0.8, 0.2, 0.5]                          # unsorted on purpose: both sort
    got = [str(tmp_path / "got_a"), str(tmp_path / "got_b")]
    want = [str(tmp_path / "want_a"), str(tmp_path / "want_b")]
    ts._write_syll_segments(fns, onsets, shifts, quantiles, 141, 0.004, dirs, got, empty)
    SC.write_syllable_segments(fns, onsets, shifts, quantiles, 141, 0.004, dirs, want, empty)
    for g, w in zip(got, want):
        assert sorted(os.listdir(g)) == sorted(os.listdir(w))
        for name in os.listdir(w):
            assert open(os.path.join(g, name), 'rb').read() == open(os.path.join(w, name), 'rb').read()
    assert sorted(os.listdir(got[0])) == ["one.txt", "two.txt"] and os.listdir(got[1]) == ["three.txt"]
    one = open(os.path.join(got[0], "one.txt")).read().splitlines()
    assert one[0] == "# Syllables from song: " + names[0]
    assert [l for l in one if l.startswith("#")][1:] == ["# Song onset: " + str(o) for o in onsets[:3]]   # appended
    assert len([l for l in one if not l.startswith("#")]) == 3 * 2
    first = one[2].split()
    assert first == ['%.5f' % (onsets[0] + 141 * 0.004 * 0.2), '%.5f' % (onsets[0] + 141 * 0.004 * 0.5)]
    assert open(os.path.join(got[0], "two.txt")).read() == "# Syllables from song: " + names[1] + "\n"
    # a second run starts the files afresh ('wb' for a file's first segment)
    ts._write_syll_segments(fns, onsets, shifts, quantiles, 141, 0.004, dirs, got, empty)
    assert open(os.path.join(got[0], "one.txt"), 'rb').read() == open(os.path.join(want[0], "one.txt"), 'rb').read()


class _FakeWarped:
    """the surface ``_write_warped_sylls`` uses, with windows that encode (file, target times)"""

    def __init__(self, names):
        self.audio_filenames = names
        self.p = {'num_time_bins': 6}
        self.start_q, self.stop_q = -0.1, 1.1
        self.template_dur = 0.5
        self.calls = []

    def _target_times(self, index, q1, q2, time_bins):
        return (np.linspace(q1, q2, time_bins) * (1 + 0.1 * index) + 0.01 * index) * self.template_dur

    def windows(self, file_index, target_times):
        file_index, target_times = np.asarray(file_index), np.asarray(target_times)
        self.calls.append(len(file_index))
        rows = np.stack([(f + 1) * np.outer(np.arange(1, 4), tt) for f, tt in zip(file_index, target_times)])
        return torch.from_numpy(rows.astype(np.float32))


def test_warped_syllable_files(tmp_path, monkeypatch):
    from ava_amd import template_segmentation as ts
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    names = [os.path.join(dirs[0], "m1.wav"), os.path.join(dirs[0], "m2.wav"), os.path.join(dirs[1], "m3.wav")]
    spec_dirs = [str(tmp_path / "sa"), str(tmp_path / "sb")]
    dset = _FakeWarped(names)
    monkeypatch.setattr(ts, "WARPED_BATCH", 4)            # 3 files x 3 pairs = 9 windows: batches of 4, 4 and 1
    quantiles = [0.9, 0.1, 0.6, 0.3]
    assert ts._write_warped_sylls(dset, dirs, spec_dirs, quantiles) == 9
    assert dset.calls == [4, 4, 1]
    want = SC.warped_syllables(_FakeWarped(names), quantiles)
    for fn in names:
        spec_dir = spec_dirs[dirs.index(os.path.split(fn)[0])]
        with np.load(os.path.join(spec_dir, os.path.split(fn)[-1][:-4] + '.npz')) as f:
            assert sorted(f.files) == ['audio_filenames', 'offsets', 'onsets', 'specs']
            specs, onsets, offsets, fns = want[fn]
            assert f['specs'].dtype == np.float64 and np.array_equal(f['specs'], specs.astype(np.float64))
            assert np.array_equal(f['onsets'], onsets) and np.array_equal(f['offsets'], offsets)
            assert f['onsets'].tolist() == [0.1, 0.3, 0.6] and f['offsets'].tolist() == [0.3, 0.6, 0.9]
            assert np.array_equal(f['audio_filenames'], fns)


def test_quantile_keyword_is_checked():
    from ava_amd import template_segmentation as ts
    assert ts._check_quantiles([0.5, 0.25], 0.0, 1.0) == [0.5, 0.25]
    for bad in ([], [0.5], [0.0, 0.5], [0.5, 1.0]):
        with pytest.raises(ValueError):
            ts._check_quantiles(bad, 0.0, 1.0)
