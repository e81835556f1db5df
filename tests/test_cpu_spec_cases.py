"""The cases of tests/spec_cases.py mean something: with the oracle alone (no device), every case reaches the edge it is
built for, and a kernel that got that edge wrong would leave the tolerance of tests/test_gpu_spec_edges.py."""
import numpy as np
import pytest
from scipy.signal import stft

import spec_cases as SC
from oracle import spec_oracle as so

ULP = 6e-8


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_targets_are_strictly_increasing_and_shapes_agree(name):
    c = SC.case(name)
    n, T = c['target_times'].shape
    F = len(c['target_freqs'])
    assert 3 <= n <= 8
    assert T == 1 or (np.diff(c['target_times'], axis=1) > 0).all()
    assert F == 1 or (np.diff(c['target_freqs']) > 0).all()
    assert all(len(a) <= 1.3 * c['fs'] for a in c['audio'])
    tt, tf = SC.device_targets(c)
    assert np.isnan(tt).sum() == n * len(c['nan_times']) and np.isnan(tf).sum() == len(c['nan_freqs'])
    want = SC.expected(name)
    assert want.shape == (n, F, T) and np.isfinite(want).all() and want.min() >= 0.0 and want.max() <= 1.0


def test_table_shapes_reach_the_second_stride_and_the_partial_row_group():
    shapes = set(SC.TABLE_SHAPES)
    assert {(1, 1), (15, 255), (16, 256), (17, 257), (33, 511), (31, 512)} == shapes
    for name in SC.TABLE_NAMES:
        want = SC.expected(name)
        assert want.max() > 0.5                                     # not blank
    one = SC.expected("table_1_1")
    assert one.shape == (3, 1, 1) and ((one > 0.0) & (one < 1.0)).all()     # F = T = 1: every pixel strictly inside
    assert SC.case("table_1_1")['p']['mel'] is False
    from ava_amd import spec as sp
    with pytest.raises(NotImplementedError):
        sp._check_stft_shape(SC.case("table_31_512")['p'], 513)


# ---- slice mean --------------------------------------------------------------------------------------------------------
def test_slice_mean_windows_cover_every_alignment():
    for name in SC.MEAN_NAMES:
        c = SC.case(name)
        lengths = [len(a) for a in c['audio']]
        assert tuple(lengths) == SC.MEAN_LENGTHS and all(n % 8 for n in lengths)
        off = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        assert off[1] % 2 == 1
        lo_hi = [SC.slice_of(c, i) for i in range(len(c['t1']))]
        assert [(lo, hi) for lo, hi in lo_hi][:-1] == [(w[1], w[2]) for w in SC.MEAN_WINDOWS][:-1]
        starts = sorted((off[c['fidx'][i]] + lo) % 8 for i, (lo, _) in enumerate(lo_hi))
        assert starts == list(range(8))
        assert len({(hi - lo) % 8 for lo, hi in lo_hi}) >= 4
        assert lo_hi[0][0] == 0 and c['t1'][0] == 0.0                                   # starts at sample 0
        assert lo_hi[-1][1] == lengths[c['fidx'][-1]] < round(c['t2'][-1] * c['fs'])    # cut by the file's end
        assert (c['target_freqs'] == np.linspace(0.0, 500.0, 16)).all() and not c['p']['mel']
        assert SC.expected(name).min() > 0.0                        # every pixel above the clip floor: the mean shows


def test_slice_mean_cases_hold_the_same_samples_in_every_dtype():
    a16, a32, a64 = (SC.case("mean_" + d)['audio'] for d in SC.MEAN_DTYPES)
    for x, y, z in zip(a16, a32, a64):
        assert x.dtype == np.int16 and y.dtype == np.int32 and z.dtype == np.float64
        assert (y == x.astype(np.int64) * 4096).all()
        assert np.abs(z * 32768.0 - x).max() <= 0.5 + 1e-9         # the float recording before rint
        assert abs(x.astype(np.float64).mean() - SC.MEAN_OFFSET) < 100.0
    e16, e32 = SC.expected("mean_int16"), SC.expected("mean_int32")
    assert np.abs(e16 - e32).max() <= 1e-10                        # the shift of the clip values by log 4096 is all


def test_a_wrong_slice_mean_moves_pixels_by_far_more_than_the_tolerance():
    c = SC.case("mean_float64")
    want = SC.expected("mean_float64")
    low = {'tail3': np.inf, 'head1': np.inf}
    for i in range(len(c['t1'])):
        base = SC.wrong_mean_window(c, i, None)
        assert np.abs(base - want[i]).max() <= 1e-9               # centring by hand is the oracle's own subtraction
        for wrong in low:
            d = np.abs(SC.wrong_mean_window(c, i, wrong) - base).max()
            low[wrong] = min(low[wrong], d)
            assert d > 100 * ULP, (i, wrong, d)
    print("slice mean, smallest max pixel change over the windows: last three samples forgotten %.3g, "
          "first sample forgotten %.3g (tolerance %.1g)" % (low['tail3'], low['head1'], ULP))


# ---- knots -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["time", "freq"])
def test_knot_targets_are_the_oracles_knots_bit_for_bit(which):
    c = SC.case("knots_%s_fill" % which)
    p, fs = c['p'], c['fs']
    fillc = (SC.KNOT_FILL - p['spec_min_val']) / (p['spec_max_val'] - p['spec_min_val'])
    assert p['spec_min_val'] == 2.0 and p['spec_max_val'] == 6.5 and fillc == (4.0 - 2.0) / 4.5
    want = SC.expected("knots_%s_fill" % which)
    for i in range(len(c['t1'])):
        lo, hi = SC.slice_of(c, i)
        f, t, _ = stft(c['audio'][c['fidx'][i]][lo:hi] - np.mean(c['audio'][c['fidx'][i]][lo:hi]), fs=fs,
                       nperseg=p['nperseg'], noverlap=p['noverlap'])
        t += max(0, c['t1'][i])
        if which == 'time':
            x, exact, outside = SC.knot_times_of(t)
            assert (x == c['target_times'][i]).all()
            assert [x[k] for k in exact] == [t[0], t[1], t[-1]]
            for k in exact:
                assert x[k - 1] == np.nextafter(x[k], -np.inf) and x[k + 1] == np.nextafter(x[k], np.inf)
            out = (x < t[0]) | (x > t[-1])
            assert sorted(np.flatnonzero(out)) == sorted(outside)
            assert (want[i][:, out] == fillc).all() and not (want[i][:, ~out] == fillc).any()
        else:
            y, exact, bins, outside = SC.knot_freqs_of(p['nperseg'], fs)
            assert (y == c['target_freqs']).all()
            assert SC.fbin_of(p['nperseg'], fs) == f[1] and len(f) == p['nperseg'] // 2 + 1
            assert [y[k] for k in exact] == [f[b] for b in bins] and bins[0] == 0 and bins[-1] == len(f) - 1
            for k in exact:
                assert y[k - 1] == np.nextafter(y[k], -np.inf) and y[k + 1] == np.nextafter(y[k], np.inf)
            out = (y < f[0]) | (y > f[-1])
            assert sorted(np.flatnonzero(out)) == sorted(outside)
            assert (want[i][out, :] == fillc).all() and not (want[i][~out, :] == fillc).any()
    # the window from sample 0 has its first frame at time 0: its neighbours are the two smallest subnormals
    if which == 'time':
        assert c['target_times'][0][2] == 0.0 and c['target_times'][0][1] < 0.0 < c['target_times'][0][3]


@pytest.mark.parametrize("which", ["time", "freq"])
def test_knot_cases_sit_above_the_clip_floor_and_nan_stands_for_outside(which):
    c = SC.case("knots_" + which)
    want = SC.expected("knots_" + which)
    out_t = np.zeros(want.shape, dtype=bool)
    if which == 'time':
        for i in range(len(c['t1'])):
            ft = SC.frame_times(c['audio'][c['fidx'][i]], c['t1'][i], c['t2'][i], c['p'])
            out_t[i][:, (c['target_times'][i] < ft[0]) | (c['target_times'][i] > ft[-1])] = True
    else:
        ny = (c['p']['nperseg'] // 2) * SC.fbin_of(c['p']['nperseg'])
        out_t[:, (c['target_freqs'] < 0) | (c['target_freqs'] > ny), :] = True
    assert not want[out_t].any()                                   # the default fill clips to 0
    inside = ((want > 0.0) & (want < 1.0))[~out_t]
    assert inside.mean() >= 0.5, inside.mean()
    # the NaN case: the device's NaN targets are out-of-grid targets of the oracle, and the fill shows there
    cn, wn = SC.case("knots_%s_nan" % which), SC.expected("knots_%s_nan" % which)
    assert (wn == SC.expected("knots_%s_fill" % which)).all()
    tt, tf = SC.device_targets(cn)
    fillc = (SC.KNOT_FILL - 2.0) / 4.5
    if which == 'time':
        assert np.isnan(tt).any(axis=0).sum() == 2 and (wn[:, :, np.isnan(tt[0])] == fillc).all()
    else:
        assert np.isnan(tf).sum() == 2 and (wn[:, np.isnan(tf), :] == fillc).all()


# ---- pruning -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.PRUNE_NAMES)
def test_pruned_cases_transform_less_than_a_quarter_of_frames_and_bins(name):
    c = SC.case(name)
    nperseg = c['p']['nperseg']
    firsts = []
    for i in range(len(c['t1'])):
        j0, j1, nf, k0, k1, K = SC.pruned_ranges(c, i)
        assert nf == len(SC.frame_times(c['audio'][c['fidx'][i]], c['t1'][i], c['t2'][i], c['p']))
        assert 30 < nf < 1300 and K == nperseg // 2 + 1
        assert 4 * (j1 - j0 + 1) < nf and 4 * (k1 - k0 + 1) < K
        firsts.append(j0 / nf)
    assert firsts[0] < 0.05 and 0.4 < firsts[1] < 0.6 and firsts[2] > 0.8      # near the start, the middle, the end
    band = name.rsplit('_', 1)[1]
    if band == 'lowest':
        assert k0 == 0
    if band == 'highest':
        assert k1 == K - 1
    if band in ('narrow', 'upper'):                                # both ends of the range come from the slack, not a clamp
        assert 0 < k0 and k1 < K - 1
    want = SC.expected(name)
    assert ((want > 0) & (want < 1)).mean() > 0.9                  # above the clip floor: a wrong frame or bin shows


def test_prune_rows_cover_both_transforms_and_hop_one():
    assert set(SC.PRUNE_STFT) == {(512, 256), (512, 0), (400, 200), (64, 63)}
    assert len(SC.PRUNE_NAMES) == 16


# ---- frame count -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.FRAME_NAMES)
def test_frame_cases_are_the_smallest_slices(name):
    c = SC.case(name)
    nperseg, hop = c['p']['nperseg'], c['p']['nperseg'] - c['p']['noverlap']
    got = [hi - lo for lo, hi in (SC.slice_of(c, i) for i in range(4))]
    assert got == [nperseg, nperseg - 1, 10 * hop, 10 * hop + 1]
    nf = [len(SC.frame_times(c['audio'][c['fidx'][i]], c['t1'][i], c['t2'][i], c['p'])) for i in (0, 2, 3)]
    assert nf == [nperseg // hop + 1, 11, 12]
    want = SC.expected(name)
    assert not want[1].any() and all(want[i].any() for i in (0, 2, 3))


# ---- quantile select ---------------------------------------------------------------------------------------------------
def test_quantiles_select_the_intended_order_statistics():
    from ava_amd import spec as sp
    assert [F * T for F, T in SC.QUANT_SHAPES] == [1, 1023, 1025, 17 * 257]
    seen = set()
    for F, T in SC.QUANT_SHAPES:
        n = F * T
        for which in [q for f, t, q in SC.QUANT_GRID if (f, t) == (F, T)]:
            p = SC.case("quant_%d_%d_%s" % (F, T, which))['p']
            q, q_lo = SC.quantile_of(which, n)
            assert p['normalize_quantile'] == q and p['within_syll_normalize']
            norm, lo, gamma = sp._quantile_index(p, F, T)
            assert norm == 1 and lo == q_lo and 0.0 <= gamma < 1.0
            seen.add((n, which))
        assert n == 1 or {SC.quantile_of(w, n)[1] for w in ('0', 'nm2', '1')} == {0, n - 2, n - 1}
    assert len(seen) == 15 == len(SC.QUANT_GRID) == len(SC.QUANT_GRID_NAMES)
    assert all(n % 1024 for n, _ in seen)                          # no F T is a multiple of the workgroup


def test_quantile_cases_hold_a_silent_window_and_an_all_ones_window():
    for name in SC.QUANT_GRID_NAMES:
        c, want = SC.case(name), SC.expected(name)
        assert not c['audio'][c['fidx'][-1]].any() and not want[-1].any()      # silence: zeros
        if want[0].size > 1 and c['p']['normalize_quantile'] < 1.0:
            assert (want[:3].reshape(3, -1).max(axis=1) > 0.99).all()       # no ties at the top: q_lo = n - 2 shows
    assert len(SC.QUANT_ONES_NAMES) == 2
    for name in SC.QUANT_ONES_NAMES:
        c = SC.case(name)
        q = dict(c['p'], within_syll_normalize=False)
        for i in range(len(c['t1'])):
            clipped = so.get_spec(c['t1'][i], c['t2'][i], c['audio'][c['fidx'][i]], q, fs=c['fs'],
                                  target_times=c['target_times'][i], target_freqs=c['target_freqs'])[0]
            assert (clipped == 1.0).all()                           # every pixel clips to 1 ...
        assert not SC.expected(name).any()                          # ... and the oracle answers zeros


# ---- scratch too small ---------------------------------------------------------------------------------------------------
def test_scratch_case_has_one_window_longer_than_the_others():
    c = SC.case("scratch")
    n = np.array([hi - lo for lo, hi in (SC.slice_of(c, i) for i in range(len(c['t1'])))])
    assert n.argmax() == SC.SCRATCH_LONG and n[SC.SCRATCH_LONG] > 1.5 * np.delete(n, SC.SCRATCH_LONG).max()
    assert SC.expected("scratch").max() > 0.5
