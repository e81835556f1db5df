"""Amplitude segmentation computed on the device.

Mirror of the reference's amplitude segmentation:

  ``get_onsets_offsets``        ava/segmenting/amplitude_segmentation.py:20-121   same signature, one recording
  ``get_onsets_offsets_batch``  the same for every recording of a ``DeviceAudio`` in one set of launches
  ``onsets_offsets_from_trace`` the decisions (lines 69-121) on a given amplitude trace
  ``get_spec``                  ava/segmenting/utils.py:22-61
  ``padded_specs``              ``get_spec`` of many audio slices in batches, zero-padded to one length
  ``segment``                   ava/segmenting/segment.py:28-66
  ``install``                   points ``ava.segmenting.amplitude_segmentation.get_onsets_offsets`` here

The STFT of whole files, the band reduction, the Gaussian smoothing, the local maxima and the nearest stop frame on
either side of every maximum run on the device (``csrc/segment.hip``); the host receives O(#maxima) integers and runs
the greedy chain and the duration filter.  The spectral arithmetic is fp64; the trace is returned (and decided on) in
the dtype the reference holds it in: float32 for int16 / float32 audio, float64 for int32 / float64 audio
(``scipy.signal.stft`` computes in complex64 or complex128 accordingly).  Thresholds are rounded to that dtype as
numpy rounds a Python float compared with the trace.

``nperseg`` must be a power of two in 64..2048 (every example script of the reference); other lengths raise
``NotImplementedError``.  There is no CPU fallback.
"""
import os

import numpy as np
import torch

from . import _lib
from .spec import DeviceAudio, _read_wav, _stft_constants

__all__ = ["EPSILON", "get_onsets_offsets", "get_onsets_offsets_batch", "onsets_offsets_from_trace", "get_spec",
           "padded_specs", "segment", "install", "frame_count", "frame_step", "band_indices", "gaussian_weights",
           "trace_dtype", "decide_thresholds", "chain", "duration_filter"]

EPSILON = 1e-9                       # segmenting/utils.py:19
DEFAULT_CHUNK_BYTES = 1 << 30        # audio bytes per batch of segment()


# ---- host helpers (the reference's own numpy arithmetic, restated) --------------------------------------------------

def _check_shape(nperseg, noverlap):
    if nperseg < 64 or nperseg > 2048 or nperseg & (nperseg - 1) or not 0 <= noverlap < nperseg:
        raise NotImplementedError("device segmentation needs nperseg a power of two in 64..2048 and "
                                  "0 <= noverlap < nperseg (got %d, %d)" % (nperseg, noverlap))


def frame_count(n_samples, nperseg, noverlap):
    """frames of scipy.signal.stft (boundary='zeros', padded=True) of n samples; 0 below nperseg samples, where the
    reference returns before any transform (amplitude_segmentation.py:51-54)"""
    n_samples = np.asarray(n_samples, dtype=np.int64)
    nstep = nperseg - noverlap
    return np.where(n_samples >= nperseg, (n_samples + nstep - 1) // nstep + 1, 0).astype(np.int64)


def frame_step(fs, nperseg, noverlap):
    """``t[1] - t[0]`` of scipy.signal.stft's time axis, with its operations (segmenting/utils.py:61)"""
    time = np.array([nperseg / 2, nperseg / 2 + (nperseg - noverlap)]) / float(fs)
    time -= (nperseg / 2) / fs
    return time[1] - time[0]


def band_indices(p):
    """(i1, i2, f): the kept bins [i1, i2) of rfftfreq(nperseg, 1 / fs) (segmenting/utils.py:54-56)"""
    f = np.fft.rfftfreq(int(p['nperseg']), 1 / p['fs'])
    return int(np.searchsorted(f, p['min_freq'])), int(np.searchsorted(f, p['max_freq'])), f


def _band_params(p):
    """(nperseg, noverlap, i1, i2) of the band stage shared with template_segmentation, checked before any device
    work: the shape, then the band, then spec_min_val != spec_max_val"""
    nperseg, noverlap = int(p['nperseg']), int(p['noverlap'])
    _check_shape(nperseg, noverlap)
    i1, i2, _ = band_indices(p)
    if i2 <= i1:
        raise ValueError("empty frequency band [%s, %s)" % (p['min_freq'], p['max_freq']))
    if not np.isfinite(float(p['spec_max_val']) - float(p['spec_min_val'])) or p['spec_max_val'] == p['spec_min_val']:
        raise ValueError("spec_max_val must differ from spec_min_val")
    return nperseg, noverlap, i1, i2


def _frame_offsets(lengths, nperseg, noverlap):
    """(frames of each file, frame_off [files + 1]: first global frame of each file) for files of these lengths"""
    T = frame_count(lengths, nperseg, noverlap)
    return T, np.concatenate([[0], np.cumsum(T)]).astype(np.int64)


def gaussian_weights(sigma, truncate=4.0):
    """(weights, radius) of scipy.ndimage.gaussian_filter1d for ``sigma``; ``([1.], 0)`` when gaussian_filter skips the
    axis (sigma <= 1e-15)"""
    if not sigma > 1e-15:
        return np.ones(1), 0
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), radius


def trace_dtype(audio_dtype):
    """dtype of the reference's spectrogram and trace for audio of this dtype (np.result_type(x, np.complex64))"""
    return np.dtype(np.float32) if np.result_type(np.dtype(audio_dtype), np.complex64) == np.complex64 \
        else np.dtype(np.float64)


def decide_thresholds(p, dtype):
    """th_1..th_3 as numpy compares them with a trace of ``dtype`` (a Python float against float32 is a float32
    comparison), returned as the fp64 values the device compares with"""
    out = []
    for key in ('th_1', 'th_2', 'th_3'):
        th = p[key]
        out.append(float(np.asarray(th, dtype=np.result_type(np.dtype(dtype), th))))
    return out


def chain(maxima, left, right):
    """the greedy onset / offset chain (amplitude_segmentation.py:76-99) over the maxima of one file in increasing
    order, given the nearest stop on either side of each (-1: none)"""
    onsets, offsets = [], []
    for m, lo, hi in zip(maxima, left, right):
        if offsets and m < offsets[-1]:
            continue
        if lo < 0 or hi < 0:
            continue
        onsets.append(int(lo))
        offsets.append(int(hi))
    return onsets, offsets


def duration_filter(onsets, offsets, dt, p):
    """amplitude_segmentation.py:57-58, 101-114: keep min_syll_len <= t2 - t1 + 1 <= max_syll_len, frames -> seconds"""
    min_syll_len = int(np.floor(p['min_dur'] / dt))
    max_syll_len = int(np.ceil(p['max_dur'] / dt))
    new_onsets, new_offsets = [], []
    for t1, t2 in zip(onsets, offsets):
        if min_syll_len <= t2 - t1 + 1 <= max_syll_len:
            new_onsets.append(t1 * dt)
            new_offsets.append(t2 * dt)
    return new_onsets, new_offsets


# ---- device stages --------------------------------------------------------------------------------------------------

def _trace(audio, frame_off, p, dt, want_spec=False):
    """the smoothed trace [frames] (torch, reference dtype) of every file of ``audio`` and the band spectrogram
    [F, frames] (float64) with ``want_spec``"""
    nperseg, noverlap, i1, i2 = _band_params(p)
    softmax = bool(p.get('softmax', False))
    temperature = float(p['temperature']) if softmax else 1.0
    if softmax and temperature == 0.0:
        raise ZeroDivisionError("softmax temperature 0")
    lib, dev = _lib.load(), audio.device
    frames = int(frame_off[-1])
    window, scale = _stft_constants(nperseg, dev)
    sigma = p['smoothing_timescale'] / dt if 'smoothing_timescale' in p else 0.0
    w, radius = gaussian_weights(sigma)
    tdt = trace_dtype(audio.dtype)
    fo = torch.from_numpy(np.ascontiguousarray(frame_off, dtype=np.int64)).to(dev)
    gw = torch.from_numpy(w).to(dev)
    trace = torch.empty(frames, dtype=torch.float64 if tdt == np.float64 else torch.float32, device=dev)
    spec = torch.empty((i2 - i1, frames), dtype=torch.float64, device=dev) if want_spec else None
    ws = _lib.workspace(lib.ava_amp_workspace_bytes(frames), dev, "%d frames" % frames)
    rc = lib.ava_amp_trace(audio.samples.data_ptr(), audio.code, audio.file_off.data_ptr(), audio.file_len.data_ptr(),
                           fo.data_ptr(), len(audio), frames, nperseg, noverlap, window.data_ptr(), scale, i1, i2,
                           float(p['spec_min_val']), float(p['spec_max_val']), 1 if softmax else 0, temperature,
                           gw.data_ptr(), radius, 1 if tdt == np.float64 else 0, trace.data_ptr(),
                           _lib.ptr(spec), ws.data_ptr(), ws.numel(), _lib.stream())
    _lib.check(rc, "ava_amp_trace")
    return trace, fo, spec


def _decide(trace, frame_off, fo_dev, p):
    """per file: (onset frames, offset frames) of the greedy chain on the device trace"""
    lib = _lib.load()
    frames, files = trace.numel(), len(frame_off) - 1
    dev = trace.device
    f64 = trace.dtype == torch.float64
    th1, th2, th3 = decide_thresholds(p, np.float64 if f64 else np.float32)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    buf = torch.empty((3, frames), dtype=torch.int64, device=dev)
    rc = lib.ava_amp_decide(trace.data_ptr(), 1 if f64 else 0, fo_dev.data_ptr(), files, frames, th1, th2, th3,
                            count.data_ptr(), buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), frames,
                            _lib.stream())
    _lib.check(rc, "ava_amp_decide")
    n = int(count.item())
    mx, left, right = buf[:, :n].cpu().numpy()
    order = np.argsort(mx, kind='stable')                 # the device appends in no fixed order
    mx, left, right = mx[order], left[order], right[order]
    cut = np.searchsorted(mx, frame_off)
    out = []
    for f in range(files):
        s = slice(cut[f], cut[f + 1])
        out.append(chain((mx[s] - frame_off[f]).tolist(), left[s].tolist(), right[s].tolist()))
    return out


def get_onsets_offsets_batch(device_audio, p, return_traces=False):
    """``get_onsets_offsets`` for every recording of a ``DeviceAudio``: one list entry per file, ``(onsets, offsets)``
    or ``(onsets, offsets, [amps])`` with ``return_traces`` (``([], [], None)`` for files shorter than nperseg)."""
    nperseg, noverlap = int(p['nperseg']), int(p['noverlap'])
    _check_shape(nperseg, noverlap)
    T, frame_off = _frame_offsets(device_audio.lengths, nperseg, noverlap)
    dt = frame_step(p['fs'], nperseg, noverlap)
    results = [([], [], None) if return_traces else ([], []) for _ in range(len(T))]
    if frame_off[-1] == 0:
        return results
    trace, fo, _ = _trace(device_audio, frame_off, p, dt)
    decisions = _decide(trace, frame_off, fo, p)
    host_trace = trace.cpu().numpy() if return_traces else None
    for f in range(len(T)):
        if T[f] == 0:
            continue
        onsets, offsets = duration_filter(*decisions[f], dt, p)
        if return_traces:
            results[f] = (onsets, offsets, [host_trace[frame_off[f]:frame_off[f + 1]].copy()])
        else:
            results[f] = (onsets, offsets)
    return results


def get_onsets_offsets(audio, p, return_traces=False):
    """Drop-in for ``ava.segmenting.amplitude_segmentation.get_onsets_offsets`` (same arguments and returns), computed
    on the device; ``audio`` is a 1-D numpy array (uploaded per call) or a ``DeviceAudio`` holding one recording."""
    dev_audio = audio if isinstance(audio, DeviceAudio) else None
    n = int(dev_audio.lengths[0]) if dev_audio is not None else len(audio)
    if n < p['nperseg']:                                                  # amplitude_segmentation.py:51-54
        if return_traces:
            return [], [], None
        return [], []
    if dev_audio is None:
        dev_audio = DeviceAudio([np.asarray(audio)])
    return get_onsets_offsets_batch(dev_audio, p, return_traces=return_traces)[0]


def onsets_offsets_from_trace(amps, dt, p):
    """The decisions of get_onsets_offsets (amplitude_segmentation.py:57-121) on a given amplitude trace, in that
    trace's dtype (float32 or float64), on the device: ``(onsets, offsets)`` in seconds."""
    amps = np.ascontiguousarray(amps)
    if amps.ndim != 1 or amps.dtype not in (np.float32, np.float64):
        raise TypeError("expected a 1-D float32 or float64 trace")
    if len(amps) < 3:
        return duration_filter([], [], dt, p)
    frame_off = np.array([0, len(amps)], dtype=np.int64)
    trace = torch.from_numpy(amps).cuda()
    fo = torch.from_numpy(frame_off).cuda()
    onsets, offsets = _decide(trace, frame_off, fo, p)[0]
    return duration_filter(onsets, offsets, dt, p)


def get_spec(audio, p):
    """Drop-in for ``ava.segmenting.utils.get_spec``: ``(spec [F, T], dt, f)`` as numpy, ``spec`` in the reference's
    dtype (float32 for int16 / float32 audio, float64 otherwise)."""
    audio = np.asarray(audio)
    assert len(audio) >= p['nperseg'], "len(audio): " + str(len(audio)) + ", nperseg: " + str(p['nperseg'])
    nperseg, noverlap = int(p['nperseg']), int(p['noverlap'])
    dev_audio = DeviceAudio([audio])
    _, frame_off = _frame_offsets([len(audio)], nperseg, noverlap)
    dt = frame_step(p['fs'], nperseg, noverlap)
    q = {k: p[k] for k in ('fs', 'nperseg', 'noverlap', 'min_freq', 'max_freq', 'spec_min_val', 'spec_max_val')}
    _, _, spec = _trace(dev_audio, frame_off, q, dt, want_spec=True)
    i1, i2, f = band_indices(p)
    return spec.cpu().numpy().astype(trace_dtype(dev_audio.dtype)), dt, f[i1:i2]


def padded_specs(slices, p, max_len=None, device='cuda', max_chunk_bytes=None):
    """The band spectrogram (``get_spec``) of every audio slice of the list ``slices`` (each at least ``nperseg``
    samples), zero-padded or truncated to ``max_len`` time bins (default: the longest): ``(specs, max_len, dt)``.
    ``specs`` is one device tensor ``[N, F, max_len]``, float64, holding the values of the reference's spectrogram dtype
    (float32-rounded for int16 / float32 audio).  The slices go to the device in batches of at most ``max_chunk_bytes``
    (default ``DEFAULT_CHUNK_BYTES``); the result does not depend on the batching.  Shared by
    ``refine_segments.get_specs`` and ``template_segmentation.segment_specs``."""
    max_chunk_bytes = DEFAULT_CHUNK_BYTES if max_chunk_bytes is None else max_chunk_bytes
    nperseg, noverlap = int(p['nperseg']), int(p['noverlap'])
    _check_shape(nperseg, noverlap)
    T = frame_count([len(a) for a in slices], nperseg, noverlap)
    dt = frame_step(p['fs'], nperseg, noverlap)
    if max_len is None:
        max_len = int(T.max())
    max_len = int(max_len)
    q = {k: p[k] for k in ('fs', 'nperseg', 'noverlap', 'min_freq', 'max_freq', 'spec_min_val', 'spec_max_val')}
    i1, i2, _ = band_indices(p)
    dev = torch.device(device)
    specs = torch.empty((len(slices), i2 - i1, max_len), dtype=torch.float64, device=dev)
    cols = torch.arange(max_len, device=dev)
    for chunk in _chunks(enumerate(slices), max_chunk_bytes):
        audio = DeviceAudio([a for _, a in chunk], device)
        rows = [i for i, _ in chunk]
        _, frame_off = _frame_offsets(audio.lengths, nperseg, noverlap)
        _, fo, spec = _trace(audio, frame_off, q, dt, want_spec=True)                    # [F, frames of the chunk]
        if trace_dtype(audio.dtype) == np.float32:
            spec = spec.to(torch.float32).to(torch.float64)
        # padding / truncation: a device gather of every slice's first max_len frames, zeros behind its last
        kept = torch.clamp(fo[1:] - fo[:-1], max=max_len)
        src = torch.clamp(fo[:-1, None] + cols[None, :], max=spec.shape[1] - 1)
        out = spec[:, src] * (cols[None, :] < kept[:, None])
        specs[rows[0]:rows[-1] + 1] = out.permute(1, 0, 2)
    return specs, max_len, dt


# ---- files ----------------------------------------------------------------------------------------------------------

def _audio_seg_filenames(audio_dir, seg_dir):
    """segment.py:194-216, whose own name test also takes a file named exactly ``.wav`` (``len >= 4``): not
    ``spec._is_wav_file``, the ``len > 4`` test of the reference's other modules"""
    names = [i for i in sorted(os.listdir(audio_dir)) if len(i) >= 4 and i[-4:] == '.wav']
    return [os.path.join(audio_dir, i) for i in names], [os.path.join(seg_dir, i[:-4] + '.txt') for i in names]


def _is_amplitude_segmentation(fn):
    return fn is get_onsets_offsets or (getattr(fn, '__module__', None) == 'ava.segmenting.amplitude_segmentation'
                                        and getattr(fn, '__name__', None) == 'get_onsets_offsets')


def _chunks(files, max_bytes):
    """groups of the (index, samples) pairs of ``files``, in order: a new group starts where the group would exceed
    ``max_bytes`` of audio or the dtype changes (a larger file is a group of its own); no group is empty"""
    chunk, nbytes = [], 0
    for i, audio in files:
        if chunk and (nbytes + audio.nbytes > max_bytes or audio.dtype != chunk[0][1].dtype):
            yield chunk
            chunk, nbytes = [], 0
        chunk.append((i, audio))
        nbytes += audio.nbytes
    if chunk:
        yield chunk


def _write(audio_fn, seg_fn, onsets, offsets):
    combined = np.stack([onsets, offsets]).T
    header = "Onsets/offsets for " + audio_fn
    np.savetxt(seg_fn, combined, fmt='%.5f', header=header)
    return len(combined)


def segment(audio_dir, seg_dir, p, verbose=True, max_chunk_bytes=DEFAULT_CHUNK_BYTES, device="cuda"):
    """Mirror of ``ava.segmenting.segment.segment``: segment every ``*.wav`` of ``audio_dir`` and write one ``.txt`` of
    onsets / offsets per file into ``seg_dir``.  When ``p['algorithm']`` is amplitude segmentation (the reference's
    function or this module's), the files go through ``get_onsets_offsets_batch`` in chunks of at most
    ``max_chunk_bytes`` of audio (a file larger than that is a chunk of its own; files of different dtypes are never
    mixed); otherwise ``p['algorithm']`` is called per file.  The output does not depend on the chunking."""
    if verbose:
        print("Segmenting audio in", audio_dir)
    if not os.path.exists(seg_dir):
        os.makedirs(seg_dir)
    num_sylls = 0
    audio_fns, seg_fns = _audio_seg_filenames(audio_dir, seg_dir)
    if not _is_amplitude_segmentation(p['algorithm']):
        for audio_fn, seg_fn in zip(audio_fns, seg_fns):
            onsets, offsets = p['algorithm'](_read_wav(audio_fn)[1], p)
            num_sylls += _write(audio_fn, seg_fn, onsets, offsets)
    else:
        files = ((i, _read_wav(fn)[1]) for i, fn in enumerate(audio_fns))
        for chunk in _chunks(files, max_chunk_bytes):
            res = get_onsets_offsets_batch(DeviceAudio([a for _, a in chunk], device), p)
            num_sylls += sum(_write(audio_fns[i], seg_fns[i], on, off) for (i, _), (on, off) in zip(chunk, res))
    if verbose:
        print("\tFound", num_sylls, "segments in", audio_dir)


def install(module=None):
    """Point ``ava.segmenting.amplitude_segmentation.get_onsets_offsets`` at this module (call after importing the
    reference package).  Parameter dicts that already hold the reference function as ``'algorithm'`` are still
    batched by ``segment``."""
    if module is None:
        import ava.segmenting.amplitude_segmentation as module
    module.get_onsets_offsets = get_onsets_offsets
    return module
