"""Template segmentation on the MI355X (ava_amd.template_segmentation) against the
reference's outputs stored in tests/golden/template.npz (tests/golden/make_golden_template.py) and against an fp64
numpy restatement of the correlation at sizes the golden does not hold."""
import warnings

import numpy as np
import pytest
import torch

import template_cases as TC
from ava_amd import _lib, segment as S, template_segmentation as TS
from ava_amd.spec import DeviceAudio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return TC.load()


def _templates(cases, c):
    src = c['opts']['template_from']
    g = cases[src] if src else c
    return g['template'], g['template64']


def _run(files, template, c):
    o = c['opts']
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        dev = DeviceAudio(files)
        tr = TS.xcorr_batch(dev, template, c['p'])
        seg = TS.segment_batch(dev, template, c['p'], num_mad=o['num_mad'], min_dt=o['min_dt'])
    return tr, seg


@pytest.mark.parametrize("path", ["given", "float64"])
def test_trace_and_segments_match_reference(golden, path):
    cases, _ = golden
    for name, c in cases.items():
        tol = float(c['tol'])
        tpl, tpl64 = _templates(cases, c)
        _, files = TC.audio_of(c['recipe'])
        if path == "float64":
            files, tpl = [a.astype(np.float64) for a in files], tpl64
        tr, seg = _run(files, tpl, c)
        for k in range(int(c['n_files'])):
            assert seg[k].dtype == np.float64
            np.testing.assert_array_equal(seg[k], c['seg_%d' % k], err_msg="%s file %d" % (name, k))
            if int(c['nlags_%d' % k]) == 0:
                assert tr[k] is None
                continue
            want = c[('trace_%d' if path == "given" else 'trace64_%d') % k]
            assert tr[k].dtype == np.float64 and tr[k].shape == want.shape, name
            err = np.abs(tr[k] - want).max()
            assert err <= tol, (name, k, err, tol)


def test_warnings_of_skipped_files(golden):
    cases, _ = golden
    c = cases['edges_int16_512']
    _, files = TC.audio_of(c['recipe'])
    with pytest.warns(UserWarning) as rec:
        TS.segment_batch(DeviceAudio(files[:2]), _templates(cases, c)[0], c['p'])
    msgs = [str(w.message) for w in rec]
    assert any("too short to make a spectrogram" in m for m in msgs)
    assert any("too short to extract segments" in m for m in msgs)


def test_get_template_matches_reference(golden, tmp_path):
    from scipy.io import wavfile
    cases, _ = golden
    n = 0
    for name, c in cases.items():
        if c['opts']['template_from']:
            continue
        tp, sm, tol = c['tp'], tuple(c['opts']['smoothing']), float(c['template_tol'])
        ex, _ = TC.audio_of(c['recipe'])
        d = tmp_path / name
        d.mkdir()
        for i, a in enumerate(ex):
            wavfile.write(str(d / ("ex_%d.wav" % i)), tp['fs'], a)
        (d / "readme.txt").write_text("not audio")
        got = TS.get_template(str(d), tp, smoothing_kernel=sm, verbose=False)
        got2 = TS.get_template_from_audio(ex, tp, smoothing_kernel=sm)
        want = c['template']
        for g in (got, got2):
            assert g.dtype == want.dtype and g.shape == want.shape, name
            assert np.abs(g.astype(np.float64) - want).max() <= tol, name
        g64 = TS.get_template_from_audio([a.astype(np.float64) for a in ex], tp, smoothing_kernel=sm)
        assert g64.dtype == np.float64 and np.abs(g64 - c['template64']).max() <= tol
        n += 1
    assert n >= 4


def test_silent_and_saturated_traces_are_exactly_zero(golden):
    cases, _ = golden
    for name, k in (('edges_int16_512', 3), ('saturated_int16_512', 0)):
        c = cases[name]
        _, files = TC.audio_of(c['recipe'])
        tr = TS.xcorr_batch(DeviceAudio([files[k]]), _templates(cases, c)[0], c['p'])[0]
        assert tr.tobytes() == np.zeros(len(tr)).tobytes(), name


def test_bitwise_reproducible_and_independent_of_batch(golden, tmp_path):
    cases, _ = golden
    c = cases['songs_int16_512']
    tpl = c['template']
    _, files = TC.audio_of(c['recipe'])
    _, edges = TC.audio_of(cases['edges_int16_512']['recipe'])
    mixed = [edges[2], files[1], edges[0], files[0], edges[3], files[1], edges[4]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        dev = DeviceAudio(mixed)
        r1 = TS.xcorr_batch(dev, tpl, c['p'])
        r2 = TS.xcorr_batch(dev, tpl, c['p'])
        for a, b, x in zip(r1, r2, mixed):
            if a is None:
                assert b is None
                continue
            assert a.tobytes() == b.tobytes()
            alone = TS.xcorr_batch(DeviceAudio([x]), tpl, c['p'])[0]
            assert alone.tobytes() == a.tobytes()
    # segment_files: the same .txt files whatever the chunking
    from scipy.io import wavfile
    ad = tmp_path / "audio"
    ad.mkdir()
    for i, a in enumerate(mixed):
        wavfile.write(str(ad / ("m%d.wav" % i)), c['p']['fs'], a)
    outs = []
    for budget in (1, files[0].nbytes * 2, 1 << 30):
        sd = tmp_path / ("seg_%d" % budget)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            res = TS.segment_files([str(ad)], [str(sd)], tpl, c['p'], verbose=False, max_chunk_bytes=budget)
        outs.append(({k: v.tobytes() for k, v in res.items()},
                     {f.name: f.read_text() for f in sorted(sd.iterdir())}))
    assert outs[0] == outs[1] == outs[2]
    # and _segment_file, one file at a time
    for i in range(len(mixed)):
        fn = str(ad / ("m%d.wav" % i))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            d, f, seg = TS._segment_file("sd", fn, tpl, c['p'])
        assert (d, f) == ("sd", fn) and seg.tobytes() == outs[0][0][fn]


def _restated(spec, frame_off, template, keep):
    """fp64 numpy restatement of the correlation (template_segmentation.py:239-245) on the device's spectrogram, and per
    lag the scale its rounding errors are relative to: sum |T| |S - mu| / (Q + 1e-9)"""
    from numpy.lib.stride_tricks import sliding_window_view
    F, L = template.shape
    out = []
    for f in range(len(frame_off) - 1):
        if not keep[f]:
            out.append((None, None))
            continue
        S_f = spec[:, frame_off[f]:frame_off[f + 1]]
        n = S_f.shape[1] - L
        win = sliding_window_view(S_f, L, axis=1)[:, :n]                  # [F, n, L]
        r, c = np.empty(n), np.empty(n)
        for a in range(0, n, 32):
            w = win[:, a:a + 32]
            d = w - w.mean(axis=(0, 2))[None, :, None]
            q = (d * d).sum(axis=(0, 2)) + TS.EPSILON
            r[a:a + 32] = np.einsum('kl,knl->n', template, d) / q
            c[a:a + 32] = np.einsum('kl,knl->n', np.abs(template), np.abs(d)) / q
        out.append((r, c))
    return out


@pytest.mark.parametrize("nperseg,L,full_band", [(512, 300, True), (512, 1024, False), (2048, 64, True),
                                                 (256, 7, False)])
def test_sizes_without_golden_match_numpy(nperseg, L, full_band):
    from ava_amd import synthetic as syn
    p = dict(TC.FINCH, nperseg=nperseg, noverlap=nperseg // 2)
    if full_band:
        p.update(min_freq=0.0, max_freq=1e9)                               # F = nperseg / 2 + 1
    i1, i2, _ = S.band_indices(p)
    F = i2 - i1
    tile = _lib.load().ava_tpl_tile_lags()
    hop = nperseg // 2
    _, songs, _ = syn.songs(n_songs=3, seconds=2.0)
    files = []
    for n_lags in (tile + 5, 3 * tile - 1, 17):                          # not a multiple of any tile
        frames = L + n_lags
        n = (frames - 1) * hop                                             # ceil(n / hop) + 1 = frames
        base = np.concatenate(songs * (1 + n // sum(len(s) for s in songs)))
        files.append(base[:n].copy())
    tpl = syn.gauss(F * L, 77).reshape(F, L) * 1e-3
    dev = DeviceAudio(files)
    band = TS._band(dev, p)
    spec, frame_off = band[0].cpu().numpy(), band[3]
    got = TS.xcorr_batch(dev, tpl, p)
    want = _restated(spec, frame_off, tpl, [True] * len(files))
    for g, (w, scale) in zip(got, want):
        assert g.shape == w.shape and len(g) > 0
        ok = np.abs(g - w) <= 1e-12 * scale                              # scale 0: an all-equal patch, both exactly 0
        assert ok.all(), (nperseg, L, (np.abs(g - w) / np.where(ok, 1.0, scale)).max())
    if full_band:
        assert F == nperseg // 2 + 1


@pytest.mark.parametrize("dtype", [np.int16, np.float64])
@pytest.mark.parametrize("nperseg", [256, 1024])
def test_band_stage_is_the_amplitude_band_stage(dtype, nperseg):
    # ava_tpl_spec is ava_amp_trace's band stage in sum mode: the same fp64 spectrogram, bit for bit.  Without
    # smoothing_timescale the amplitude trace is the raw band sum (radius 0, weights {1}); for float64 audio it is
    # stored unrounded, so it equals the template path's frame sums bit for bit too.
    from ava_amd import synthetic as syn
    shift = TC.LOG_INT16_SCALE if dtype == np.float64 else 0.0
    p = dict(TC.FINCH, nperseg=nperseg, noverlap=nperseg // 3, spec_min_val=TC.FINCH['spec_min_val'] - shift,
             spec_max_val=TC.FINCH['spec_max_val'] - shift)
    _, songs, _ = syn.songs(n_songs=3, seconds=2.0, dtype=dtype)
    dev = DeviceAudio(songs + [songs[0][:nperseg // 2]])                     # a file without frames among them
    spec, fsum, _, frame_off, _ = TS._band(dev, p)
    trace, _, aspec = S._trace(dev, frame_off, p, S.frame_step(p['fs'], nperseg, p['noverlap']), want_spec=True)
    spec, aspec = spec.cpu().numpy(), aspec.cpu().numpy()
    assert spec.shape == aspec.shape and spec.shape[1] == frame_off[-1] > 0
    assert np.array_equal(spec, aspec)
    if dtype == np.float64:
        assert trace.dtype == torch.float64
        assert np.array_equal(fsum.cpu().numpy(), trace.cpu().numpy())


def test_template_band_mismatch_raises(golden):
    cases, _ = golden
    c = cases['songs_int16_512']
    _, files = TC.audio_of(c['recipe'])
    with pytest.raises(ValueError):
        TS.segment_batch(DeviceAudio(files[:1]), c['template'][:-1], c['p'])


def test_c_abi_argument_checks():
    lib = _lib.load()
    dev = torch.device("cuda")
    frames, F, L = 40, 8, 10
    audio = torch.zeros((frames - 1) * 256, dtype=torch.int16, device=dev)
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    length = torch.full((1,), audio.numel(), dtype=torch.int64, device=dev)
    fo = torch.tensor([0, frames], dtype=torch.int64, device=dev)
    win = torch.ones(512, dtype=torch.float64, device=dev)
    spec = torch.empty((F, frames), dtype=torch.float64, device=dev)
    fsum = torch.empty(frames, dtype=torch.float64, device=dev)
    s = _lib.stream()
    P = lambda t: t.data_ptr()                                             # noqa: E731
    good = [P(audio), 0, P(off), P(length), P(fo), 1, frames, 512, 256, P(win), 1.0, 10, 10 + F, 2.0, 6.5, P(spec),
            P(fsum), s]
    assert lib.ava_tpl_spec(*good) == 0
    bad = {0: None, 2: None, 4: None, 9: None, 15: None, 16: None,         # null pointers
           7: 1000, 8: 512,                                                # nperseg not a power of two; noverlap >= nperseg
           11: 300, 12: 10}                                                # k0 past k1; empty band
    for i, v in bad.items():
        args = list(good)
        args[i] = v
        assert lib.ava_tpl_spec(*args) == -1, i
    lags = frames - L
    lo = torch.tensor([0, lags], dtype=torch.int64, device=dev)
    to = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    tm = torch.ones((F, L), dtype=torch.float64, device=dev)
    trace = torch.empty(lags, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.ava_tpl_workspace_bytes(lags), dtype=torch.uint8, device=dev)
    xgood = [P(spec), P(fsum), F, frames, P(fo), P(lo), P(to), 1, lags, 1, P(tm), F, L, P(trace), P(ws), ws.numel(), s]
    assert lib.ava_tpl_xcorr(*xgood) == 0
    torch.cuda.synchronize()
    xbad = {0: None, 1: None, 4: None, 5: None, 6: None, 10: None, 13: None, 14: None,     # null pointers
            12: 0, 11: F - 1, 15: ws.numel() - 1}                         # L <= 0; F mismatch; workspace too small
    for i, v in xbad.items():
        args = list(xgood)
        args[i] = v
        assert lib.ava_tpl_xcorr(*args) == -1, i
    args = list(xgood)
    args[12] = -3
    assert lib.ava_tpl_xcorr(*args) == -1
    torch.cuda.synchronize()


def test_unsupported_nperseg_raises(golden):
    cases, _ = golden
    c = cases['songs_int16_512']
    with pytest.raises(NotImplementedError):
        TS.segment_batch(DeviceAudio([np.zeros(5000, dtype=np.int16)]), c['template'], dict(c['p'], nperseg=400,
                                                                                           noverlap=200))
