"""GPU tests of the integer-shift fit: the kernels of csrc/shift_fit.hip through
ava_amd.shift_fit against the numpy restatement of tests/shiftfit_cases.py (pinned by tests/test_cpu_shiftfit.py), and
the two ``segment_sylls_*`` functions of ava_amd.template_segmentation built on them.

Tolerances:
  shift_loss      relative 4 F T 2^-52, the order of an F T-term sum of non-negative terms: every term is the oracle's
                  operation for operation, only the order of the sum differs; two runs bit-identical
  m̄               absolute 2 K 2^-52 max|x|: two K-term sums in different orders, each divided once
  m               absolute 64 T (1 + 16 λ) 2^-52 max|m̄|: the backward error of a banded Cholesky / LDLᵀ solve times the
                  condition bound 1 + 16 λ of A (|D₂ᵀD₂| <= 16, the smallest eigenvalue of A is above 1)
  shifts          exact: tests/test_cpu_shiftfit.py shows the best lag at least a relative 1e-8 clear of the second best
  transform       exact: copies
"""
import builtins
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import shiftfit_cases as SC
import template_cases as TC
import warped_cases as WC
from ava_amd import synthetic as syn

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
EINVAL = -1


@pytest.fixture(scope="module")
def sf():
    from ava_amd import shift_fit
    return shift_fit


def _hashed(K, F, T, dtype, salt):
    return (2 * syn.u01(K * F * T, salt).reshape(K, F, T) - 0.7).astype(dtype)


# ---- the loss -------------------------------------------------------------------------------------------------------

LOSS_SHAPES = [(3, 9, 200, 40), (5, 1, 37, 33), (1, 5, 67, 13), (2, 2, 4, 0), (2, 1, 2048, 409)]


@pytest.mark.parametrize("shape", LOSS_SHAPES)
@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_loss_against_the_restatement(shape, dtype, sf):
    """F over the staged rows and lags off the workgroup's block of 64 (81 lags); nearly every tap clipped (L = 33 of
    T = 37); K = 1; a single lag; T at the cap with 819 lags in 13 blocks"""
    K, F, T, L = shape
    x = _hashed(K, F, T, dtype, 5301)
    m = syn.u01(F * T, 5302).reshape(F, T) - 0.2
    want = SC.loss(x, m, L)
    got = sf.shift_loss(torch.from_numpy(x).cuda(), m, L)
    again = sf.shift_loss(torch.from_numpy(x).cuda(), m, L)
    assert torch.is_tensor(got) and got.dtype == torch.float64 and tuple(got.shape) == (K, 2 * L + 1)
    bound = 4 * F * T * U
    rel = float(np.abs(got.cpu().numpy() / want - 1).max())
    print("%s %s: max rel err %.3e (bound %.3e)" % (shape, dtype, rel, bound))
    assert np.isfinite(want).all() and (want > 0).all()
    assert rel <= bound
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    host = sf.shift_loss(x, m, L)                                            # numpy in, numpy out
    assert isinstance(host, np.ndarray) and np.array_equal(host, got.cpu().numpy())


@pytest.mark.parametrize("shape", [s for s in LOSS_SHAPES if s[2] <= 512])
@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_loss_against_warp_loss_at_integer_shifts(shape, dtype, sf):
    """the shift objective of warp_fit fed (lag, 0) candidates interpolates with weight 0: the same terms, in another
    order"""
    from ava_amd import warp_fit as wf
    K, F, T, L = shape
    x = _hashed(K, F, T, dtype, 5311)
    m = syn.u01(F * T, 5312).reshape(F, T) - 0.2
    cand = np.zeros((K, 2 * L + 1, 2))
    cand[:, :, 0] = SC.lag_order(L)
    want = wf.warp_loss(x, m, cand, 0.0, np.inf) / (F * T)
    got = sf.shift_loss(x, m, L)
    rel = float(np.abs(got / want - 1).max())
    print("%s %s: max rel err against warp_loss %.3e" % (shape, dtype, rel))
    assert rel <= 4 * F * T * U


def test_loss_nan_and_argmin_tie_rule(sf):
    """a NaN rendition has NaN losses and keeps shift 0; an all-zero rendition ties at every lag and keeps shift 0; the
    others move"""
    x, sh = SC.planted(6, 1, 40, 4, 5200)
    x[2] = 0.0
    x[4, 0, 20] = np.nan                                                     # a column every lag reads
    model = sf.ShiftWarping(maxlag=0.2, smoothness_reg_scale=10.0)
    clean = np.delete(x, 4, axis=0)
    model.fit(clean.transpose(0, 2, 1), iterations=4)
    want = SC.fit(clean, 0.2, 10.0, 4)
    assert model.shifts.tolist() == want['shifts'].tolist() and model.shifts[2] == 0 and np.abs(model.shifts).max() > 0
    m = want['template']
    loss = sf.shift_loss(x, m, 8)
    assert np.isnan(loss[4]).all() and np.isfinite(np.delete(loss, 4, axis=0)).all()
    from ava_amd import _lib
    lib, st = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_loss = torch.from_numpy(loss).cuda()
    d_loss[5, 3] = float('nan')                                              # a single NaN among finite losses
    shifts = torch.full((6,), 99, dtype=torch.int32, device="cuda")
    best = torch.empty(6, dtype=torch.float64, device="cuda")
    assert lib.ava_shiftfit_argmin(d_loss.data_ptr(), 6, 8, shifts.data_ptr(), best.data_ptr(), st) == 0
    host = d_loss.cpu().numpy()
    assert shifts.tolist() == SC.lag_order(8)[SC.argmin(host)].tolist()
    assert shifts[4].item() == 0 and shifts[2].item() == 0 and np.isnan(best[4].item())


# ---- the template ---------------------------------------------------------------------------------------------------

# (K, F, T, L, λ): K = 1; K over one chunk of 128 and off a chunk boundary; exactly two chunks; T = 3; T at the cap
TEMPLATE_SHAPES = [(1, 2, 3, 1, 10.0), (300, 1, 67, 13, 10.0), (129, 3, 40, 8, 0.0), (256, 2, 130, 26, 10.0),
                   (5, 1, 2048, 409, 10.0), (3, 20, 2048, 409, 0.0)]


@pytest.mark.parametrize("shape", TEMPLATE_SHAPES)
@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_template_against_the_restatement(shape, dtype, sf):
    K, F, T, L, lam = shape
    x = _hashed(K, F, T, dtype, 5321)
    shifts = np.round((2 * syn.u01(K, 5322) - 1) * L).astype(np.int64)
    shifts[0], shifts[-1] = L, -L                                            # K = 1: -L
    want_m, want_mbar = SC.template(x, shifts, lam)
    m, mbar = sf.shift_template(torch.from_numpy(x).cuda(), torch.from_numpy(shifts).cuda(), lam, return_mean=True)
    assert m.dtype == torch.float64 and tuple(m.shape) == tuple(mbar.shape) == (F, T)
    m, mbar = m.cpu().numpy(), mbar.cpu().numpy()
    e_mbar, b_mbar = float(np.abs(mbar - want_mbar).max()), 2 * K * U * float(np.abs(x).max())
    e_m, b_m = float(np.abs(m - want_m).max()), 64 * T * (1 + 16 * lam) * U * float(np.abs(want_mbar).max())
    print("%s %s: m̄ err %.3e (bound %.3e), m err %.3e (bound %.3e)" % (shape, dtype, e_mbar, b_mbar, e_m, b_m))
    assert e_mbar <= b_mbar
    assert e_m <= b_m
    if lam == 0.0:
        assert np.abs(m - mbar / (1 + SC.L2 / K)).max() <= 4 * U * np.abs(mbar).max()
    host = sf.shift_template(x, shifts, lam)
    assert isinstance(host, np.ndarray) and np.array_equal(host, m)


# ---- the fit --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted_fits():
    out = {}
    for case in SC.CASES:
        x, sh = SC.planted(*case)
        for dtype in SC.DTYPES:
            xd = x.astype(dtype)
            out[case, dtype] = (xd, sh, SC.fit(xd, SC.MAXLAG, SC.SMOOTHNESS, SC.ITERATIONS))
    return out


@pytest.mark.parametrize("kind", ["numpy", "tensor"])
@pytest.mark.parametrize("dtype", SC.DTYPES)
@pytest.mark.parametrize("case", SC.CASES)
def test_fit_on_planted_shifts(case, dtype, kind, sf, planted_fits):
    K, F, T, _, _ = case
    x, sh, want = planted_fits[case, dtype]
    assert want['gap'] >= 1e-8
    data = np.ascontiguousarray(x.transpose(0, 2, 1))                        # affinewarp's [K, T, N]
    if kind == "tensor":
        data = torch.from_numpy(data).cuda()
    model = sf.ShiftWarping(maxlag=SC.MAXLAG, smoothness_reg_scale=SC.SMOOTHNESS)
    assert model.fit(data, iterations=SC.ITERATIONS) is model
    assert isinstance(model.shifts, np.ndarray) and model.shifts.dtype.kind == 'i' and model.shifts.shape == (K,)
    assert model.shifts.tolist() == want['shifts'].tolist()
    assert len(set((model.shifts - sh).tolist())) == 1                       # the planted shifts up to one offset
    template = model.template.cpu().numpy() if kind == "tensor" else model.template
    assert torch.is_tensor(model.template) == (kind == "tensor") and template.shape == (T, F)
    _, mbar = SC.template(x, want['history'][-2], SC.SMOOTHNESS)
    err, bound = float(np.abs(template.T - want['template']).max()), 64 * T * (1 + 16 * SC.SMOOTHNESS) * U * np.abs(mbar).max()
    print("%s %s %s: template err %.3e (bound %.3e); loss_hist %s" % (case, dtype, kind, err, bound, model.loss_hist[:3]))
    assert err <= bound
    aligned = model.transform(data)
    assert torch.is_tensor(aligned) == (kind == "tensor")
    aligned = aligned.cpu().numpy() if kind == "tensor" else aligned
    assert aligned.dtype == np.dtype(dtype) and np.array_equal(aligned, SC.aligned(x, want['shifts']).transpose(0, 2, 1))
    pred = model.predict()
    pred = pred.cpu().numpy() if kind == "tensor" else pred
    idx = np.clip(np.arange(T)[None, :] - want['shifts'][:, None], 0, T - 1)
    assert pred.shape == (K, T, F) and np.array_equal(pred, template[idx])
    hist = model.loss_hist
    assert len(hist) == SC.ITERATIONS and all(b <= a for a, b in zip(hist[:-1], hist[1:]))
    assert np.abs(np.array(hist) / (np.array(want['J']) / (K * F * T)) - 1).max() <= 1e-9


def test_argument_errors(sf):
    cap = sf._lib.load().ava_shiftfit_max_t()
    assert cap >= 2048
    with pytest.raises(NotImplementedError):
        sf.ShiftWarping(maxlag=0.1).fit(np.zeros((2, cap + 1, 1)))
    with pytest.raises(NotImplementedError):
        sf.shift_loss(np.zeros((2, 1, cap + 1)), np.zeros((1, cap + 1)), 3)
    with pytest.raises(ValueError):
        sf.ShiftWarping(maxlag=0.1).fit(np.zeros((2, 2, 1)))                 # T < 3
    with pytest.raises(ValueError):
        sf.ShiftWarping(maxlag=1.0)
    with pytest.raises(ValueError):
        sf.ShiftWarping(maxlag=-0.1)
    with pytest.raises(ValueError):
        sf.ShiftWarping().fit(np.zeros((4, 9)))                              # wrong rank
    with pytest.raises(ValueError):
        sf.shift_loss(np.zeros((2, 1, 9)), np.zeros((1, 9)), 9)              # L > T - 1
    with pytest.raises(ValueError):
        sf.shift_template(np.zeros((2, 1, 9)), np.zeros(3, dtype=np.int64), 1.0)
    # the C ABI refuses the same before any launch: the outputs keep their sentinel
    lib, st = sf._lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros((2, 1, 9), dtype=torch.float64, device="cuda")
    m = torch.zeros((1, 9), dtype=torch.float64, device="cuda")
    loss = torch.full((2, 19), -7.0, dtype=torch.float64, device="cuda")
    shifts = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    for T, L in [(9, 9), (9, -1), (2, 0), (cap + 1, 3)]:
        assert lib.ava_shiftfit_loss(x.data_ptr(), 1, 2, 1, T, m.data_ptr(), L, loss.data_ptr(), st) == EINVAL
    assert lib.ava_shiftfit_loss(x.data_ptr(), 2, 2, 1, 9, m.data_ptr(), 3, loss.data_ptr(), st) == EINVAL
    for lam in (-1.0, float('nan'), float('inf')):
        assert lib.ava_shiftfit_template(x.data_ptr(), 1, 2, 1, 9, shifts.data_ptr(), lam, 1e-7, None, loss.data_ptr(),
                                         ws.data_ptr(), ws.numel(), st) == EINVAL
    assert lib.ava_shiftfit_template(x.data_ptr(), 1, 2, 1, 9, shifts.data_ptr(), 1.0, 1e-7, None, loss.data_ptr(),
                                     ws.data_ptr(), 8, st) == -3
    assert lib.ava_shiftfit_workspace_bytes(2, 1, 2) == 0
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all())


# ---- segment_sylls_from_songs ---------------------------------------------------------------------------------------

QUANTILES = [0.2, 0.5, 0.8]
SONG_P = dict(TC.FINCH)
MOTIF = 0.5


@pytest.fixture(scope="module")
def song_dirs(tmp_path_factory):
    """two audio directories: three recordings with three renditions each whose segments are the true onsets moved by
    up to 40 ms; one of the recordings also has a segment that reaches past its end; a fourth recording has no song"""
    root = tmp_path_factory.mktemp("shiftfit_songs")
    fs = SONG_P['fs']
    _, songs, onsets = syn.songs(n_exemplars=1, n_songs=4, fs=fs, seconds=3.0, motif_seconds=MOTIF, renditions=3, salt=5400)
    audio_dirs = [str(root / "audio_a"), str(root / "audio_b")]
    seg_dirs = [str(root / "songs_a"), str(root / "songs_b")]
    for d in audio_dirs + seg_dirs:
        os.makedirs(d)
    for s, (audio, on) in enumerate(zip(songs, onsets)):
        d = 0 if s < 2 else 1
        wavfile.write(os.path.join(audio_dirs[d], "song_%d.wav" % s), fs, audio)
        jitter = (2 * syn.u01(len(on), 5410 + s) - 1) * 0.04
        segs = np.stack([on + jitter, on + jitter + MOTIF], axis=1)
        if s == 1:
            dur = len(audio) / fs
            segs = np.concatenate([segs, [[dur - MOTIF - 0.02, dur - 0.02]]])
        if s == 3:
            segs = np.zeros((0, 2))
        np.savetxt(os.path.join(seg_dirs[d], "song_%d.txt" % s), segs, fmt='%.5f')
    return root, audio_dirs, seg_dirs


def _same_files(got_dirs, want_dirs):
    for g, w in zip(got_dirs, want_dirs):
        assert sorted(os.listdir(g)) == sorted(os.listdir(w)) and len(os.listdir(w)) > 0
        for name in os.listdir(w):
            assert open(os.path.join(g, name), 'rb').read() == open(os.path.join(w, name), 'rb').read(), name


def test_segment_sylls_from_songs(song_dirs, sf, monkeypatch, capsys):
    from ava_amd import segment as S
    from ava_amd import template_segmentation as ts
    root, audio_dirs, seg_dirs = song_dirs
    p = SONG_P
    got = [str(root / "sylls_a"), str(root / "sylls_b")]
    ts.segment_sylls_from_songs(audio_dirs, seg_dirs, got, p, quantiles=QUANTILES, verbose=False)
    # the device's own traces and shifts
    info = ts._song_traces(audio_dirs, seg_dirs, p, verbose=False)
    traces = info['traces']
    K, T = traces.shape
    model = sf.ShiftWarping(maxlag=0.2, smoothness_reg_scale=10.0).fit(traces[:, :, None], iterations=50)
    # the host's view of the same segments
    song_segs = ts.read_segment_decisions(audio_dirs, seg_dirs, verbose=False)
    audio_of = {fn: wavfile.read(fn) for fn in song_segs}
    rows, empty = SC.song_slices(song_segs, audio_of, 0.05)
    dt = S.frame_step(p['fs'], p['nperseg'], p['noverlap'])
    assert K == len(rows) == 10 and [r[4] for r in rows].count(True) == 1 and len(empty) == 1
    edge = [r[4] for r in rows].index(True)
    # the traces: the band spectrogram summed over frequency, z-scored over the segment's own columns
    specs, host_traces = info['specs'].cpu().numpy(), traces.cpu().numpy()
    bins = []
    for k, (fn, onset, i1, i2, is_edge) in enumerate(rows):
        n = len(audio_of[fn][1][max(i1, 0):i2])
        own = int(S.frame_count(n, p['nperseg'], p['noverlap']))
        pre, post = SC.edge_bins(i1, i2, len(audio_of[fn][1]), p['fs'], dt) if is_edge else (0, 0)
        bins.append(own + pre + post)
        amps = specs[k, :, :own].sum(axis=0)
        amps = (amps - amps.mean()) / (amps.std() + ts.EPSILON)
        if is_edge:
            assert post > 0 and pre == 0 and not host_traces[k].any()
        else:
            assert np.abs(host_traces[k] - amps[:T]).max() <= 1e-12 * np.abs(amps).max()
    assert T == min(bins) and info['bins'].tolist() == bins
    # the shifts are the restatement's on those traces, and not trivial
    want = SC.fit(host_traces[:, None, :], 0.2, 10.0, 50)
    assert want['gap'] >= 1e-8
    assert model.shifts.tolist() == want['shifts'].tolist()
    assert model.shifts[edge] == 0 and len(set(model.shifts.tolist())) > 2
    # the written files are the host statement's under those shifts
    want_dirs = [str(root / "want_a"), str(root / "want_b")]
    SC.write_syllable_segments([r[0] for r in rows], [r[1] for r in rows], model.shifts, QUANTILES, T, dt, audio_dirs,
                               want_dirs, empty)
    _same_files(got, want_dirs)
    assert open(os.path.join(got[1], "song_3.txt")).read() == "# Syllables from song: " + empty[0] + "\n"
    # the interactive path: the same files, and the picture
    answers = iter(['0.2', 'x', '0.5', '0.8', 's'])
    monkeypatch.setattr(builtins, "input", lambda prompt="": next(answers))
    again = [str(root / "again_a"), str(root / "again_b")]
    img = str(root / "quantiles.pdf")
    capsys.readouterr()
    ts.segment_sylls_from_songs(audio_dirs, seg_dirs, again, p, img_fn=img)
    out = capsys.readouterr().out
    assert "Invalid input!" in out and "Writing syllable segments..." in out
    _same_files(again, want_dirs)
    assert os.path.getsize(img) > 0
    with pytest.raises(ValueError):
        ts.segment_sylls_from_songs(audio_dirs, seg_dirs, again, p, quantiles=[0.5])


# ---- segment_sylls_from_warped_songs --------------------------------------------------------------------------------

def test_segment_sylls_from_warped_songs(tmp_path, monkeypatch):
    from ava_amd import syllable_dataset as sd
    from ava_amd import template_segmentation as ts
    from ava_amd import warped_window as ww
    p = dict(syn.FINCH_PARAMS)
    audio = WC.motifs(dict(n_files=3, fs=p['fs'], motif_seconds=0.3, salt=4411, dtype='int16'))
    xk, yk = WC.knots(3, 4, 5500)
    ds = ww.DeviceWarpedWindowDataset.from_arrays(audio, p['fs'], p, x_knots=xk, y_knots=yk)
    audio_dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    spec_dirs = [str(tmp_path / "specs_a"), str(tmp_path / "specs_b")]
    ds.audio_filenames = [os.path.join(audio_dirs[0], "m0.wav"), os.path.join(audio_dirs[1], "m1.wav"),
                          os.path.join(audio_dirs[1], "m2.wav")]
    quantiles = [0.7, 0.05, 0.4, 1.0]
    monkeypatch.setattr(ts, "WARPED_BATCH", 4)                               # 9 windows: launches of 4, 4 and 1
    ts.segment_sylls_from_warped_songs(ds, audio_dirs, spec_dirs, quantiles=quantiles, verbose=False)
    want = SC.warped_syllables(ds, quantiles)
    files = []
    for fn in ds.audio_filenames:
        write_fn = os.path.join(spec_dirs[audio_dirs.index(os.path.split(fn)[0])], os.path.split(fn)[-1][:-4] + '.npz')
        files.append(write_fn)
        specs, onsets, offsets, fns = want[fn]
        with np.load(write_fn) as f:
            assert f['specs'].shape == (3, p['num_freq_bins'], p['num_time_bins']) and f['specs'].any()
            assert np.array_equal(f['specs'], specs.astype(np.float64))
            assert f['onsets'].tolist() == [0.05, 0.4, 0.7] and f['offsets'].tolist() == [0.4, 0.7, 1.0]
            assert np.array_equal(f['audio_filenames'], fns)
    part = sd.get_syllable_partition(spec_dirs, 1.0, shuffle=False)
    assert part['train'] == sorted(files) and part['test'] == []
    loaded = sd.DeviceSyllableDataset(part['train'])
    assert len(loaded) == 9
    first = np.load(sorted(files)[0])['specs'][1]
    assert np.array_equal(loaded[1].cpu().numpy(), first.astype(np.float32))
    # the interactive path writes the same arrays (a .npz member carries its time stamp, so the members are compared)
    answers = iter(['0.7', '0.05', '2.0', '0.4', '', '1.0', 's'])
    monkeypatch.setattr(builtins, "input", lambda prompt="": next(answers))
    again = [str(tmp_path / "again_a"), str(tmp_path / "again_b")]
    img = str(tmp_path / "warped.pdf")
    ts.segment_sylls_from_warped_songs(ds, audio_dirs, again, time_bins=64, num_specs=1, img_fn=img, verbose=False)
    assert os.path.getsize(img) > 0
    for d1, d2 in zip(spec_dirs, again):
        assert sorted(os.listdir(d1)) == sorted(os.listdir(d2))
        for name in os.listdir(d1):
            with np.load(os.path.join(d1, name)) as a, np.load(os.path.join(d2, name)) as b:
                assert sorted(a.files) == sorted(b.files)
                for key in a.files:
                    assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes()
    with pytest.raises(ValueError):
        ts.segment_sylls_from_warped_songs(ds, audio_dirs, again, quantiles=[0.3], verbose=False)
