"""Template segmentation computed on the device.

Mirror of the computational surface of ava/segmenting/template_segmentation.py, the birdsong path:

  ``get_template``             lines 37-84     same signature; exemplar spectrograms on the device
  ``get_template_from_audio``  the same on arrays instead of files
  ``segment_files``            lines 87-153    same dict, files and prints; files go through ``segment_batch`` in chunks
  ``read_segment_decisions``   lines 156-191   the plain reader
  ``_segment_file``            lines 194-264   drop-in, same return tuple
  ``xcorr_batch``              the normalised cross-correlation trace of every file of a ``DeviceAudio``
  ``segment_batch``            ``_segment_file``'s segments for every file of a ``DeviceAudio``
  ``segments_from_trace``      the decisions (lines 246-264) on a given trace
  ``segment_specs``            the batch counterpart of ``_get_spec`` (lines 758-790) as ``clean_collected_segments``
                               uses it (lines 311-334): one zero-padded band spectrogram per collected segment
  ``clean_collected_segments`` lines 281-452   same signature, prints, prompts and picture; ``clean_collected_data`` is
                               its deprecated alias (lines 267-278)
  ``_in_region``               lines 817-827
  ``segment_sylls_from_songs`` lines 455-627   same signature, prompts, prints and files; the alignment is
                               ``shift_fit.ShiftWarping`` (row f15), this project's model in place of affinewarp's
  ``segment_sylls_from_warped_songs``  lines 630-755   on a ``DeviceWarpedWindowDataset``; writes ``.npz``
  ``install``                  points the reference module's ``get_template``, ``segment_files``, ``_segment_file``,
                               ``clean_collected_segments``, ``clean_collected_data`` and the two ``segment_sylls_*``
                               here and adds ``segment_specs``

The band spectrogram of whole files (``_get_spec``, lines 758-790) and the correlation with the template run on the
device in fp64 (the band kernel of ``csrc/segment.hip`` in sum mode, then ``csrc/template_seg.hip``); the host
receives the fp64 trace and runs the threshold, the maxima and ``_clean_max_indices`` on it (O(lags) per file,
vectorised numpy).  ``clean_collected_segments`` makes its spectrograms with the band kernel too
(``segment.padded_specs``, shared with ``refine_segments.get_specs``) and embeds them with
``projection.TransformableUMAP(metric='correlation')``: the correlation kNN of ``csrc/projection.hip`` for the fit and
for the ``transform`` of every directory's segments.  Directories are processed one after the other in this process.
The template's smoothing, truncation, mean and normalisation are the reference's own numpy calls on a few F x L
arrays.  Unlike the reference, this module imports without affinewarp, umap, h5py or bokeh.

``nperseg`` must be a power of two in 64..2048; other lengths raise ``NotImplementedError``.  There is no CPU fallback.
"""
import bisect
import os
import warnings

import numpy as np
import torch

from . import _lib
from . import projection
from . import segment as _seg
from .spec import DeviceAudio, _is_wav_file, _read_wav, _stft_constants

__all__ = ["EPSILON", "get_template", "get_template_from_audio", "segment_files", "read_segment_decisions",
           "xcorr_batch", "segment_batch", "segments_from_trace", "segment_specs", "clean_collected_segments",
           "clean_collected_data", "_in_region", "segment_sylls_from_songs", "segment_sylls_from_warped_songs", "install"]

EPSILON = 1e-9                       # template_segmentation.py:31
DEFAULT_CHUNK_BYTES = 1 << 30        # audio bytes per batch of segment_files()


def _read(filename, p):
    fs, audio = _read_wav(filename)
    assert fs == p['fs'], "Found samplerate=" + str(fs) + ", expected " + str(p['fs'])
    return audio


# ---- device stages --------------------------------------------------------------------------------------------------

def _band(device_audio, p):
    """(spec [F, frames] float64, frame sums [frames], frame_off device, frame_off host, frames per file) of every file;
    spec is None when no file reaches nperseg samples"""
    nperseg, noverlap, i1, i2 = _seg._band_params(p)
    T, frame_off = _seg._frame_offsets(device_audio.lengths, nperseg, noverlap)
    frames = int(frame_off[-1])
    dev = device_audio.device
    fo = torch.from_numpy(frame_off).to(dev)
    if frames == 0:
        return None, None, fo, frame_off, T
    lib = _lib.load()
    window, scale = _stft_constants(nperseg, dev)
    spec = torch.empty((i2 - i1, frames), dtype=torch.float64, device=dev)
    fsum = torch.empty(frames, dtype=torch.float64, device=dev)
    rc = lib.ava_tpl_spec(device_audio.samples.data_ptr(), device_audio.code, device_audio.file_off.data_ptr(),
                          device_audio.file_len.data_ptr(), fo.data_ptr(), len(device_audio), frames, nperseg,
                          noverlap, window.data_ptr(), scale, i1, i2, float(p['spec_min_val']),
                          float(p['spec_max_val']), spec.data_ptr(), fsum.data_ptr(), _lib.stream())
    _lib.check(rc, "ava_tpl_spec")
    return spec, fsum, fo, frame_off, T


def _xcorr(band, template, keep):
    """the device trace (host float64) of the files with keep[f], and the per-file lag offsets"""
    spec, fsum, fo, frame_off, T = band
    F, L = template.shape
    n_lags = np.where(keep, T - L, 0).astype(np.int64)
    lag_off = np.concatenate([[0], np.cumsum(n_lags)]).astype(np.int64)
    lags = int(lag_off[-1])
    if lags == 0:
        return np.zeros(0), lag_off
    lib = _lib.load()
    dev = spec.device
    tile = lib.ava_tpl_tile_lags()
    tile_off = np.concatenate([[0], np.cumsum((n_lags + tile - 1) // tile)]).astype(np.int64)
    offs = torch.from_numpy(np.stack([lag_off, tile_off])).to(dev)
    tm = torch.from_numpy(np.ascontiguousarray(template, dtype=np.float64)).to(dev)
    trace = torch.empty(lags, dtype=torch.float64, device=dev)
    ws = _lib.workspace(lib.ava_tpl_workspace_bytes(lags), dev, "%d lags" % lags)
    rc = lib.ava_tpl_xcorr(spec.data_ptr(), fsum.data_ptr(), spec.shape[0], spec.shape[1], fo.data_ptr(),
                           offs[0].data_ptr(), offs[1].data_ptr(), len(T), lags, int(tile_off[-1]), tm.data_ptr(), F, L,
                           trace.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream())
    _lib.check(rc, "ava_tpl_xcorr")
    return trace.cpu().numpy(), lag_off


def _traces(device_audio, template, p, min_extra_time_bins, names):
    """per file: the trace, or None where _segment_file returns early (with its warning)"""
    template = np.asarray(template)
    if template.ndim != 2:
        raise ValueError("expected a template [F, L]")
    band = _band(device_audio, p)
    T = band[4]
    dt = _seg.frame_step(p['fs'], int(p['nperseg']), int(p['noverlap']))
    L = template.shape[1]
    names = names if names is not None else ["<file %d>" % f for f in range(len(T))]
    keep = np.zeros(len(T), dtype=bool)
    for f in range(len(T)):
        n = int(device_audio.lengths[f])
        if n < p['nperseg']:                                            # template_segmentation.py:218-225
            warnings.warn("Found an audio file that is too short to make a spectrogram: " + names[f] +
                          "\nSamples: " + str(n) + "\np['nperseg']: " + str(p['nperseg']), UserWarning)
        elif T[f] - L < min_extra_time_bins:                            # lines 229-237
            d1, d2 = dt * L, dt * T[f]
            warnings.warn("Found an audio file that is too short to extract segments from: " + names[f] +
                          "\nTemplate duration: " + str(d1) + "\nFile duration: " + str(d2) +
                          "\nConsider reducing the template duration.", UserWarning)
        else:
            keep[f] = True
    if not keep.any():
        return [None] * len(T), dt
    F = band[0].shape[0]
    if template.shape[0] != F:          # where the reference's np.dot(template, temp) fails on mismatched lengths
        raise ValueError("template has %d frequency bins, the band has %d" % (template.shape[0], F))
    trace, lag_off = _xcorr(band, template, keep)
    return [trace[lag_off[f]:lag_off[f + 1]].copy() if keep[f] else None for f in range(len(T))], dt


def xcorr_batch(device_audio, template, p, min_extra_time_bins=5):
    """The normalised cross-correlation of ``_segment_file`` (template_segmentation.py:239-245) for every file of a
    ``DeviceAudio``: a list of float64 arrays of n_f - L values, ``None`` where the reference skips the file."""
    return _traces(device_audio, template, p, min_extra_time_bins, None)[0]


def _clean_max_indices(old_indices, old_times, values, min_dt=0.05):
    """template_segmentation.py:793-815 (remove maxima that are too close together), same output, ties included: the
    maxima in ``np.argsort`` order of their values, each kept unless a kept one lies within ``min_dt``.  The kept times
    stay sorted, so only the nearest kept time on either side is compared (|a - t| rounds monotonically in a)."""
    if len(old_indices) <= 1:
        return old_indices
    old_indices = old_indices[np.argsort(values[old_indices])]
    times = old_times[old_indices]
    kept, acc = [0], [times[0]]
    for i in range(1, len(old_indices)):
        time = times[i]
        pos = bisect.bisect_left(acc, time)
        if pos > 0 and abs(acc[pos - 1] - time) < min_dt:
            continue
        if pos < len(acc) and abs(acc[pos] - time) < min_dt:
            continue
        acc.insert(pos, time)
        kept.append(i)
    indices = np.array(old_indices[kept])
    indices.sort()
    return indices


def segments_from_trace(result, dt, spec_len, num_mad=2.0, min_dt=0.05):
    """The decisions of _segment_file (template_segmentation.py:246-264) on a trace: ``[n, 2]`` (onset, offset)."""
    result = np.asarray(result, dtype=np.float64)
    median = np.median(result)
    abs_devs = np.abs(result - median)
    mad = np.median(abs_devs) + EPSILON
    times = dt * np.arange(len(result))
    indices = np.argwhere(result > median + num_mad * mad).flatten()[1:-1]
    cand = indices[2:len(indices) - 1]                                  # range(2, len(indices) - 1)
    is_max = np.maximum(result[cand - 1], result[cand + 1]) < result[cand]
    max_indices = np.array(cand[is_max], dtype='int')
    max_indices = _clean_max_indices(max_indices, times, result, min_dt=min_dt)
    segments = np.zeros((len(max_indices), 2))
    segments[:, 0] = dt * max_indices
    segments[:, 1] = segments[:, 0] + spec_len * dt
    return segments


def segment_batch(device_audio, template, p, num_mad=2.0, min_dt=0.05, min_extra_time_bins=5, names=None):
    """``_segment_file``'s segments for every file of a ``DeviceAudio``: one ``[n, 2]`` float64 array of (onset,
    offset) in seconds per file, ``(0, 2)`` with the reference's warning where it skips the file.  ``names`` (optional)
    name the files in those warnings."""
    traces, dt = _traces(device_audio, template, p, min_extra_time_bins, names)
    L = np.asarray(template).shape[1]
    return [np.zeros((0, 2)) if tr is None else segments_from_trace(tr, dt, L, num_mad, min_dt) for tr in traces]


# ---- templates ------------------------------------------------------------------------------------------------------

def _exemplar_specs(audio_list, p):
    """(_get_spec's spectrogram of each exemplar in the reference's dtype, dt), all from one device launch"""
    audio_list = [np.asarray(a) for a in audio_list]
    if not audio_list:
        raise ValueError("no exemplars")
    short = [len(a) for a in audio_list if len(a) < p['nperseg']]
    if short:
        raise ValueError("an exemplar of %d samples is shorter than nperseg = %d" % (short[0], p['nperseg']))
    spec, _, _, frame_off, _ = _band(DeviceAudio(audio_list), p)
    host = spec.cpu().numpy()
    dt = _seg.frame_step(p['fs'], int(p['nperseg']), int(p['noverlap']))
    return [host[:, frame_off[f]:frame_off[f + 1]].astype(_seg.trace_dtype(a.dtype))
            for f, a in enumerate(audio_list)], dt


def _template_from_specs(specs, smoothing_kernel):
    """template_segmentation.py:73-80 on the exemplar spectrograms"""
    from scipy.ndimage import gaussian_filter
    specs = [gaussian_filter(spec, smoothing_kernel) for spec in specs]
    min_time_bins = min(spec.shape[1] for spec in specs)
    specs = np.array([i[:, :min_time_bins] for i in specs])
    template = np.mean(specs, axis=0)
    template -= np.mean(template)
    template /= np.sum(np.power(template, 2)) + EPSILON
    return template, min_time_bins


def get_template_from_audio(audio_list, p, smoothing_kernel=(0.5, 0.5)):
    """``get_template`` on a list of 1-D audio arrays (the samples ``scipy.io.wavfile.read`` returns)."""
    specs, _ = _exemplar_specs(audio_list, p)
    return _template_from_specs(specs, smoothing_kernel)[0]


def get_template(feature_dir, p, smoothing_kernel=(0.5, 0.5), verbose=True):
    """Drop-in for ``ava.segmenting.template_segmentation.get_template``: the template from every ``*.wav`` of
    ``feature_dir`` (``os.listdir`` order), float32 for int16 / float32 exemplars, float64 otherwise."""
    filenames = [os.path.join(feature_dir, i) for i in os.listdir(feature_dir) if _is_wav_file(i)]
    audio = [_read(fn, p) for fn in filenames]
    specs, dt = _exemplar_specs(audio, p)
    template, min_time_bins = _template_from_specs(specs, smoothing_kernel)
    if verbose:
        duration = min_time_bins * dt
        print("Made template from", len(filenames), "files. Duration:", duration)
    return template


# ---- files ----------------------------------------------------------------------------------------------------------

def _segment_file(segment_dir, filename, template, p, num_mad=2.0, min_dt=0.05, min_extra_time_bins=5):
    """Drop-in for ``ava.segmenting.template_segmentation._segment_file``: ``(segment_dir, filename, segments)``."""
    audio = _read(filename, p)
    if len(audio) < p['nperseg']:
        warnings.warn("Found an audio file that is too short to make a spectrogram: " + filename + "\nSamples: " +
                      str(len(audio)) + "\np['nperseg']: " + str(p['nperseg']), UserWarning)
        return segment_dir, filename, np.zeros((0, 2))
    segments = segment_batch(DeviceAudio([audio]), template, p, num_mad=num_mad, min_dt=min_dt,
                             min_extra_time_bins=min_extra_time_bins, names=[filename])[0]
    return segment_dir, filename, segments


def segment_files(audio_dirs, segment_dirs, template, p, num_mad=2.0, min_dt=0.05, n_jobs=1, verbose=True,
                  max_chunk_bytes=DEFAULT_CHUNK_BYTES, device="cuda"):
    """Drop-in for ``ava.segmenting.template_segmentation.segment_files``: same dict, same ``.txt`` files and prints.
    ``n_jobs`` is accepted and ignored: the files go through ``segment_batch`` in chunks of at most
    ``max_chunk_bytes`` of audio (a larger file is a chunk of its own; dtypes are never mixed).  The output does not
    depend on the chunking."""
    all_audio_fns, all_seg_dirs = [], []
    for audio_dir, segment_dir in zip(audio_dirs, segment_dirs):
        if not os.path.exists(segment_dir):
            os.makedirs(segment_dir)
        audio_fns = [os.path.join(audio_dir, i) for i in os.listdir(audio_dir) if _is_wav_file(i)]
        all_audio_fns = all_audio_fns + audio_fns
        all_seg_dirs = all_seg_dirs + [segment_dir] * len(audio_fns)
    if verbose:
        print("Segmenting files. n =", len(all_audio_fns))
    res = []
    files = ((i, _read(fn, p)) for i, fn in enumerate(all_audio_fns))
    for chunk in _seg._chunks(files, max_chunk_bytes):
        segs = segment_batch(DeviceAudio([a for _, a in chunk], device), template, p, num_mad=num_mad, min_dt=min_dt,
                             names=[all_audio_fns[i] for i, _ in chunk])
        res.extend((all_seg_dirs[i], all_audio_fns[i], s) for (i, _), s in zip(chunk, segs))
    result = {}
    num_segments = 0
    for segment_dir, audio_fn, segments in res:
        result[audio_fn] = segments
        segment_fn = os.path.split(audio_fn)[-1][:-4] + '.txt'
        segment_fn = os.path.join(segment_dir, segment_fn)
        np.savetxt(segment_fn, segments, fmt='%.5f')
        num_segments += len(segments)
    if verbose:
        print("\tFound", num_segments, "segments.")
        print("\tDone.")
    return result


def read_segment_decisions(audio_dirs, segment_dirs, verbose=True):
    """Mirror of ``ava.segmenting.template_segmentation.read_segment_decisions``: the dict ``segment_files``
    returned, read back from the ``.txt`` files."""
    if verbose:
        print("Reading segments...")
    result = {}
    n_segs = 0
    for audio_dir, segment_dir in zip(audio_dirs, segment_dirs):
        audio_fns = [os.path.join(audio_dir, i) for i in os.listdir(audio_dir) if _is_wav_file(i)]
        for audio_fn in audio_fns:
            segment_fn = os.path.split(audio_fn)[-1][:-4] + '.txt'
            segment_fn = os.path.join(segment_dir, segment_fn)
            segments = np.loadtxt(segment_fn).reshape(-1, 2)
            result[audio_fn] = segments
            n_segs += len(segments)
    if verbose:
        print("\tFound", n_segs, "segments.")
        print("\tDone.")
    return result


# ---- removal of false positives -------------------------------------------------------------------------------------

def _segment_slices(audio, segments, fs, p, name):
    """the samples ``audio[int(round(onset fs)):int(round(offset fs))]`` of every segment (lines 318-320)"""
    slices = []
    for segment in segments:
        i1 = int(round(segment[0] * fs))
        i2 = int(round(segment[1] * fs))
        piece = audio[i1:i2]
        if len(piece) < p['nperseg']:
            raise ValueError("segment [%s, %s] of %s has %d samples, fewer than nperseg = %d"
                             % (segment[0], segment[1], name, len(piece), p['nperseg']))
        slices.append(piece)
    return slices


def _padded(slices, p, max_len, device, max_chunk_bytes):
    specs, max_len, _ = _seg.padded_specs(slices, p, max_len, device, max_chunk_bytes)
    return specs


def segment_specs(result, p, device='cuda', max_chunk_bytes=DEFAULT_CHUNK_BYTES):
    """The reference's ``_get_spec(fs, audio[i1:i2], p)[0]`` of every segment of ``result`` (``{filename: [[onset,
    offset], ...]}``, what ``segment_files`` returns), ``i = int(round(t fs))``, files in dict order, zero-padded to
    the longest one's length as lines 330-334 pad them: one device tensor ``[N, F, max_t]`` with the dtype convention
    of ``refine_segments.get_specs`` (float64 holding the reference's values: float32-rounded for int16 / float32
    audio).  ``[0, F, 0]`` when there is no segment.  The slices go through the band kernel in batches of at most
    ``max_chunk_bytes`` of audio; the result does not depend on the batching.

    A segment of fewer than ``nperseg`` samples raises ``ValueError`` (the reference lets scipy shrink the window
    there; template segments, one template long, never are that short)."""
    slices = []
    for filename in result.keys():
        segments = np.asarray(result[filename]).reshape(-1, 2)
        if len(segments) == 0:
            continue
        fs, audio = _read_wav(filename)
        assert fs == p['fs'], "Found samplerate=" + str(fs) + ", expected " + str(p['fs'])
        slices += _segment_slices(audio, segments, fs, p, filename)
    if not slices:
        _, _, i1, i2 = _seg._band_params(p)
        return torch.zeros((0, i2 - i1, 0), dtype=torch.float64, device=torch.device(device))
    return _padded(slices, p, None, device, max_chunk_bytes)


def _in_region(point, bounds):
    """Is the point strictly inside one of the rectangles of ``bounds`` (lines 817-827)?  The two x answers and the
    two y answers of a rectangle may come in either order."""
    for i in range(len(bounds['x1s'])):
        x_min = min(bounds['x1s'][i], bounds['x2s'][i])
        x_max = max(bounds['x1s'][i], bounds['x2s'][i])
        y_min = min(bounds['y1s'][i], bounds['y2s'][i])
        y_max = max(bounds['y1s'][i], bounds['y2s'][i])
        if point[0] > x_min and point[0] < x_max and point[1] > y_min and point[1] < y_max:
            return True
    return False


def _is_number(answer):
    try:
        float(answer)
        return True
    except (TypeError, ValueError):
        if answer != 'initial input':
            print("Invalid input!")
        return False


def _new_transform():
    """``umap.UMAP(random_state=42, metric='correlation')`` (line 354; umap-learn's defaults n_neighbors=15,
    min_dist=0.1) as the device class that keeps its training rows for ``transform``"""
    return projection.TransformableUMAP(n_components=2, n_neighbors=15, min_dist=0.1, metric='correlation',
                                        random_state=42)


def _region_plot(embedding, colors, title, img_fn):
    """the scatter plot with unit grid lines of lines 382-390"""
    import matplotlib.pyplot as plt
    plt.switch_backend('agg')
    X, Y = embedding[:, 0], embedding[:, 1]
    plt.scatter(X, Y, c=colors, s=0.9, alpha=0.5)
    for x_tick in np.arange(np.floor(np.min(X)), np.ceil(np.max(X))):
        plt.axvline(x=x_tick, c='k', alpha=0.1, lw=0.5)
    for y_tick in np.arange(np.floor(np.min(Y)), np.ceil(np.max(Y))):
        plt.axhline(y=y_tick, c='k', alpha=0.1, lw=0.5)
    plt.title(title)
    plt.savefig(img_fn)
    plt.close('all')


def _to_numpy(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def clean_collected_segments(result, audio_dirs, segment_dirs, p, max_num_specs=10000, verbose=True,
                             img_fn='temp.pdf', tooltip_plot_dir='html'):
    """Mirror of ``ava.segmenting.template_segmentation.clean_collected_segments`` (same arguments, prints and
    prompts): embed the spectrograms of up to ``max_num_specs`` collected segments (the seed-42 subsample) with
    correlation-metric UMAP, let the user box the real song in the embedding (the picture is saved to ``img_fn`` before
    every box; the tooltip plot is written when ``ava.plotting.tooltip_plot`` imports, with a warning otherwise), then
    embed every file's segments with the fitted object's ``transform`` and rewrite the segment files in place with the
    segments inside the boxes (a file none of whose segments is kept is rewritten empty).

    Differences from the reference: the segments of a whole directory go through one ``transform`` (the rows do not
    depend on each other), the directories are processed serially in this process, and a segment whose spectrogram is
    longer than the longest fitted one raises ``ValueError`` (the reference fails there with a numpy broadcast
    error), as does one of fewer than ``nperseg`` samples.  The fitted object keeps ``max_num_specs x F x max_t x 4``
    bytes of training rows on the device until this function returns."""
    from .refine_segments import _tooltip_plot
    # Collect spectrograms.
    if verbose:
        print("Collecting spectrograms...")
    specs = segment_specs(result, p) if any(len(result[fn]) for fn in result.keys()) else []
    if len(specs) == 0:
        warnings.warn("Found no spectrograms in ava.segmenting.template_segmentation.clean_collected_segments.\n" +
                      "Consider reducing the `num_mad` parameter in `segment_files`.", UserWarning)
        return
    max_t = int(specs.shape[2])
    if len(specs) > max_num_specs:
        warnings.warn("Found more spectrograms than `max_num_specs` (" + str(max_num_specs) +
                      "). Consider increasing `max_num_specs` or `num_mad`.", UserWarning)
    if verbose:
        print("\tCollected", len(specs), "spectrograms.")
        print("\tSpectrogram shape:", tuple(specs.shape[1:]))
        if len(specs) > max_num_specs:
            print("\tRandomly sampling", max_num_specs, "spectrograms.")
        print("\tDone.")
    perm = np.random.RandomState(42).permutation(len(specs))[:max_num_specs]      # np.random.seed(42); permutation
    specs = specs[torch.from_numpy(perm).to(specs.device)]
    # UMAP the spectrograms.
    if verbose:
        print("Running UMAP. n =", len(specs))
    transform = _new_transform()
    embedding = _to_numpy(transform.fit_transform(specs.reshape(len(specs), -1)))
    if verbose:
        print("\tDone.")
    # Plot and ask for user input.
    bounds = {'x1s': [], 'x2s': [], 'y1s': [], 'y2s': []}
    bounds_keys = ['x1s', 'x2s', 'y1s', 'y2s']
    queries = ['x1: ', 'x2: ', 'y1: ', 'y2: ']
    i = 0
    while True:
        colors = ['b' if _in_region(embed, bounds) else 'r' for embed in embedding]
        print("Selected", len([c for c in colors if c == 'b']), "out of", len(colors))
        title = "Find relevant song"
        _region_plot(embedding, colors, title, img_fn)
        # Plot the tooltip plot.
        if i == 0:
            tooltip_plot = _tooltip_plot()
            if tooltip_plot is not None:
                if verbose:
                    print("Writing tooltip plot...")
                tooltip_plot(embedding, _to_numpy(specs), output_dir=tooltip_plot_dir, num_imgs=1000, title=title,
                             grid=True)
                if verbose:
                    print("\tDone.")
        # Get input from user.
        for key, query in zip(bounds_keys, queries):
            answer = 'initial input'
            while not _is_number(answer):
                answer = input(query)
            bounds[key].append(float(answer))
        # Continue?
        temp = input('[Enter] to select more regions, [c] to continue: ')
        if temp == 'c':
            break
        i += 1
    del specs
    # Save only the good segments.
    if verbose:
        print("Saving segments...")
    num_deleted, num_total = 0, 0
    for audio_dir, seg_dir in zip(audio_dirs, segment_dirs):
        audio_fns = [os.path.join(audio_dir, i) for i in os.listdir(audio_dir) if _is_wav_file(i)]
        slices, files = [], []                                          # files: (segment file, its segments)
        for audio_fn in audio_fns:
            audio = _read(audio_fn, p)
            segment_fn = os.path.join(seg_dir, os.path.split(audio_fn)[-1][:-4] + '.txt')
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)            # numpy's "input contained no data"
                segments = np.loadtxt(segment_fn).reshape(-1, 2)
            if len(segments) == 0:
                continue
            slices += _segment_slices(audio, segments, p['fs'], p, audio_fn)
            files.append((segment_fn, segments))
        if not slices:
            continue
        T = _seg.frame_count([len(a) for a in slices], int(p['nperseg']), int(p['noverlap']))
        if int(T.max()) > max_t:
            raise ValueError("a segment of %s has a spectrogram of %d time bins, more than the %d of the longest "
                             "collected one" % (audio_dir, int(T.max()), max_t))
        specs = _padded(slices, p, max_t, 'cuda', DEFAULT_CHUNK_BYTES)
        embed = _to_numpy(transform.transform(specs.reshape(len(specs), -1)))
        row = 0
        for segment_fn, segments in files:
            keep = [_in_region(embed[row + j], bounds) for j in range(len(segments))]
            row += len(segments)
            new_segments = segments[np.array(keep, dtype=bool)]
            num_total += len(new_segments)
            num_deleted += len(segments) - len(new_segments)
            np.savetxt(segment_fn, new_segments, fmt='%.5f')
    if verbose:
        print("\tdeleted:", num_deleted, "remaining:", num_total)
        print("\tDone.")


def clean_collected_data(result, audio_dirs, segment_dirs, p, max_num_specs=10000, verbose=True, img_fn='temp.pdf',
                         tooltip_plot_dir='html'):
    """Deprecated. See ``clean_collected_segments``."""
    warnings.warn("ava.segmenting.template_segmentation.clean_collected_data has been renamed to "
                  "clean_collected_segments in v0.3.0.", UserWarning)
    clean_collected_segments(result, audio_dirs, segment_dirs, p, max_num_specs=max_num_specs, verbose=verbose,
                             img_fn=img_fn, tooltip_plot_dir=tooltip_plot_dir)


# ---- song motifs into syllables ----------------------------------------------------

def _song_slices(song_segs, shoulder, read):
    """The host half of lines 487-512: for every song segment of ``song_segs`` (``{filename: [[onset, offset], ...]}``)
    the samples ``audio[max(i1, 0):i2]`` with ``i = int(fs * t)`` (Python's truncation towards zero, not the ``round``
    of ``segment_specs``) of the segment widened by ``shoulder`` on either side.  ``read(filename)`` returns ``(fs,
    audio)``.  Returns a dict of equally long lists ``slices``, ``fns``, ``song_onsets`` (the widened onsets),
    ``edge`` (does the segment reach outside the file?), ``pad_secs`` (``(-i1 / fs, (i2 - len(audio)) / fs)``: the
    seconds missing in front and behind), and ``empty_audio_files``: the recordings without song."""
    out = dict(slices=[], fns=[], song_onsets=[], edge=[], pad_secs=[], empty_audio_files=[])
    for audio_fn in song_segs:
        fs, audio = read(audio_fn)
        for seg in np.asarray(song_segs[audio_fn]).reshape(-1, 2):
            onset, offset = seg[0] - shoulder, seg[1] + shoulder
            i1, i2 = int(fs * onset), int(fs * offset)
            out['slices'].append(audio[max(i1, 0):i2])
            out['fns'].append(audio_fn)
            out['song_onsets'].append(onset)
            out['edge'].append(i1 < 0 or i2 > len(audio))
            out['pad_secs'].append((-i1 / fs, (i2 - len(audio)) / fs))
        if len(song_segs[audio_fn]) == 0:
            out['empty_audio_files'].append(audio_fn)
    return out


def _edge_bins(pad_secs, dt):
    """``(pre_bins, post_bins)`` of lines 500-501 for a segment that misses ``pad_secs`` seconds in front and behind"""
    return max(0, int(np.round(pad_secs[0] / dt))), max(0, int(np.round(pad_secs[1] / dt)))


def _song_traces(audio_dirs, song_seg_dirs, p, shoulder=0.05, verbose=True):
    """Lines 485-530 of ``segment_sylls_from_songs`` up to the fit: a dict with ``traces`` (device float64
    ``[K, T]``: per segment the band spectrogram summed over frequency, minus its mean, divided by ``std + EPSILON``,
    all on the device, then truncated to the shortest), ``specs`` (device ``[K, F, max_t]``, zero-padded), ``bins``
    (time bins of every segment's spectrogram, edge padding included), ``dt`` and the lists of ``_song_slices``."""
    song_segs = read_segment_decisions(audio_dirs, song_seg_dirs)

    def read(fn):
        fs, audio = _read_wav(fn)
        return fs, audio

    info = _song_slices(song_segs, shoulder, read)
    assert len(info['slices']) > 0, "Found no spectrograms!"
    for fn, piece in zip(info['fns'], info['slices']):
        if len(piece) < p['nperseg']:
            raise ValueError("a song segment of %s has %d samples, fewer than nperseg = %d" % (fn, len(piece), p['nperseg']))
    specs, _, dt = _seg.padded_specs(info['slices'], p)
    dev = specs.device
    bins = _seg.frame_count([len(a) for a in info['slices']], int(p['nperseg']), int(p['noverlap']))
    own = torch.from_numpy(bins).to(dev)                                  # columns the segment's own spectrogram has
    edge = np.array(info['edge'], dtype=bool)
    for k in np.flatnonzero(edge):                                        # lines 499-507: a constant, wider spectrogram
        pre_bins, post_bins = _edge_bins(info['pad_secs'][k], dt)
        bins[k] += pre_bins + post_bins
    # amplitude traces (lines 516-520), every segment over its own columns
    mask = (torch.arange(specs.shape[2], device=dev)[None, :] < own[:, None]).to(torch.float64)
    amps = specs.sum(dim=1) * mask
    mean = amps.sum(dim=1, keepdim=True) / own[:, None]
    amps = (amps - mean) * mask
    std = torch.sqrt((amps * amps).sum(dim=1, keepdim=True) / own[:, None])
    amps = amps / (std + EPSILON)
    amps[torch.from_numpy(edge).to(dev)] = 0.0                            # a constant spectrogram: an all-zero trace
    min_time_bins, max_time_bins = int(bins.min()), int(bins.max())
    if verbose and (min_time_bins != max_time_bins):
        print("Found different numbers of time bins in segments!")
        print("\tmin:" + str(min_time_bins) + ", max:", max_time_bins)
        print("\tTruncating to minimum number of time bins.")
    if min_time_bins > amps.shape[1]:                                     # every segment reaches outside its file
        amps = torch.nn.functional.pad(amps, (0, min_time_bins - amps.shape[1]))
    info.update(traces=amps[:, :min_time_bins].contiguous(), specs=specs, bins=bins, own_bins=own.cpu().numpy(), dt=dt)
    return info


def _write_syll_segments(fns, song_onsets, shifts, quantiles, num_time_bins, dt, audio_dirs, syll_seg_dirs,
                         empty_audio_files):
    """Lines 593-627: the syllable segment files.  Per song segment the onsets and offsets ``song_onset + duration *
    quantile + shift * dt``, ``'%.5f'``, under a two-line header for a file's first segment (``'wb'``) and a one-line
    header for the later ones (``'ab'``); an empty file with its header for every recording without song."""
    duration = num_time_bins * dt
    quantiles = np.array(quantiles)
    quantiles.sort()
    files_encountered = {}
    for i, (fn, song_onset) in enumerate(zip(fns, song_onsets)):
        onsets = song_onset + duration * quantiles[:-1] + shifts[i] * dt
        offsets = song_onset + duration * quantiles[1:] + shifts[i] * dt
        write_fn = _syll_filename(fn, audio_dirs, syll_seg_dirs)
        segs = np.stack([onsets, offsets]).reshape(2, -1).T
        header, mode = "", 'ab'
        if fn not in files_encountered:
            files_encountered[fn] = 1
            mode = 'wb'
            header += "Syllables from song: " + fn + "\n"
        header += "Song onset: " + str(song_onset)
        with open(write_fn, mode) as f:
            np.savetxt(f, segs, fmt='%.5f', header=header)
    for fn in empty_audio_files:
        write_fn = _syll_filename(fn, audio_dirs, syll_seg_dirs)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            np.savetxt(write_fn, np.array([]), header="Syllables from song: " + fn)


def _syll_filename(fn, audio_dirs, syll_seg_dirs):
    index = audio_dirs.index(os.path.split(fn)[0])
    write_fn = os.path.join(syll_seg_dirs[index], os.path.split(fn)[-1])[:-4] + '.txt'
    if not os.path.exists(os.path.split(write_fn)[0]):
        os.makedirs(os.path.split(write_fn)[0])
    return write_fn


def _ask_quantile(quantiles, lo, hi, error_lines, blank_redraws=False):
    """One round of the prompt of lines 571-587 / 688-705: ``True`` once the user stops"""
    while True:
        temp = input("Add or delete quantile or [s]top: ")
        if blank_redraws and temp == '':
            return False
        if temp == 's':
            return True
        try:
            temp = float(temp)
            assert lo < temp and temp < hi
        except (ValueError, AssertionError):
            for line in error_lines:
                print(line)
            continue
        if temp in quantiles:
            quantiles.remove(temp)
        else:
            quantiles.append(temp)
        return False


def _check_quantiles(quantiles, lo, hi):
    """the keyword-only ``quantiles`` as a list of floats strictly inside ``(lo, hi)``, at least two: ``ValueError``"""
    quantiles = [float(q) for q in quantiles]
    if len(quantiles) < 2:
        raise ValueError("at least two quantiles are needed to cut a segment, got %d" % len(quantiles))
    if not all(lo < q < hi for q in quantiles):
        raise ValueError("quantiles must lie strictly between %s and %s" % (lo, hi))
    return quantiles


def segment_sylls_from_songs(audio_dirs, song_seg_dirs, syll_seg_dirs, p, shoulder=0.05, img_fn='temp.pdf', verbose=True,
                             *, quantiles=None):
    """Mirror of ``ava.segmenting.template_segmentation.segment_sylls_from_songs`` (lines 455-627; same arguments,
    prompts, prints and files): split song renditions into syllables.  The band spectrograms of all song segments
    (widened by ``shoulder``) are made in one batched pass, their amplitude traces are aligned by one integer shift each
    with ``shift_fit.ShiftWarping(maxlag=0.2, smoothness_reg_scale=10.0)`` in 50 iterations on the device (this
    project's own model in place of affinewarp's), the user enters quantiles of the aligned motif, and every
    rendition's syllable segments are written to ``syll_seg_dirs``.  All song segments must be the same duration.

    ``quantiles`` (keyword-only, no counterpart in the reference): cut at these quantiles without a picture or a prompt.
    Fewer than two quantiles raise ``ValueError``, from the keyword before any device work; the reference would write
    nothing useful there.

    Edge behaviour, kept as the reference has it: a segment that reaches outside its file gets a constant spectrogram
    of ``T + pre_bins + post_bins`` columns (line 506, which should paste the real one into it, is a no-op), hence an
    all-zero amplitude trace and, by the tie rule of the fit, shift 0.  A segment of fewer than ``nperseg`` samples
    raises ``ValueError``."""
    from .shift_fit import ShiftWarping
    if quantiles is not None:
        quantiles = _check_quantiles(quantiles, 0.0, 1.0)
    info = _song_traces(audio_dirs, song_seg_dirs, p, shoulder=shoulder, verbose=verbose)
    amp_traces, dt = info['traces'], info['dt']
    num_time_bins = int(amp_traces.shape[1])
    max_t = num_time_bins * dt * 1e3
    model = ShiftWarping(maxlag=0.2, smoothness_reg_scale=10.0)
    model.fit(amp_traces[:, :, None], iterations=50)
    shifts = model.shifts
    if quantiles is None:
        import matplotlib.pyplot as plt
        plt.switch_backend('agg')
        raw = amp_traces.cpu().numpy()
        aligned = model.predict()[:, :, 0].cpu().numpy()
        max_raw_val, max_aligned_val = np.max(raw), np.max(aligned)
        quantiles = []
        while True:
            _, axarr = plt.subplots(3, 1, sharex=True)
            k = np.random.randint(len(raw))
            spec = info['specs'][k, :, :int(info['own_bins'][k])].cpu().numpy()
            if info['edge'][k]:
                spec = np.mean(spec) * np.ones((spec.shape[0], int(info['bins'][k])))
            axarr[0].imshow(spec, origin='lower', aspect='auto', extent=[0, max_t, p['min_freq'] / 1e3, p['max_freq'] / 1e3])
            temp = np.copy(raw)
            for q in quantiles:
                for i in range(len(temp)):
                    try:
                        temp[i, int(round(q * num_time_bins)) + shifts[i]] = max_raw_val
                    except IndexError:
                        pass
            axarr[1].imshow(temp, origin='lower', aspect='auto', extent=[0, max_t, 0, len(raw)])
            temp = np.copy(aligned)
            for q in quantiles:
                for i in range(len(temp)):
                    temp[i, int(round(q * num_time_bins))] = max_aligned_val
            axarr[2].imshow(temp, origin='lower', aspect='auto', extent=[0, max_t, 0, len(raw)])
            axarr[0].set_ylabel("Frequency (kHz)")
            axarr[1].set_ylabel('Amplitude')
            axarr[2].set_ylabel('Shifted')
            axarr[0].set_title('Enter segmenting quantiles:')
            axarr[2].set_xlabel('Time (ms)')
            plt.savefig(img_fn)
            plt.close('all')
            if _ask_quantile(quantiles, 0.0, 1.0, ["Invalid input!", "Must be \'s\' or a float between 0 and 1."]):
                break
        if len(quantiles) < 2:
            raise ValueError("at least two quantiles are needed to cut a segment, got %d" % len(quantiles))
    if verbose:
        print("Writing syllable segments...")
    _write_syll_segments(info['fns'], info['song_onsets'], shifts, quantiles, num_time_bins, dt, audio_dirs, syll_seg_dirs,
                         info['empty_audio_files'])


WARPED_BATCH = 1024                  # windows per launch of segment_sylls_from_warped_songs


def _write_warped_sylls(dset, audio_dirs, spec_dirs, quantiles):
    """Lines 712-752 on a dataset with ``audio_filenames``, ``p``, ``_target_times`` and ``windows``: one ``.npz`` per
    recording, written as ``process_sylls`` writes its groups.  Returns the number of spectrograms saved."""
    from .preprocess import iter_groups
    audio_dir_to_spec_dir = dict(zip(audio_dirs, spec_dirs))
    quantiles = sorted(quantiles)
    segs = [[q1, q2] for q1, q2 in zip(quantiles[:-1], quantiles[1:])]
    n_files, n_segs, T = len(dset.audio_filenames), len(segs), dset.p['num_time_bins']
    file_index = np.repeat(np.arange(n_files), n_segs)
    target_times = np.empty((n_files * n_segs, T))
    for index in range(n_files):
        for j, (q1, q2) in enumerate(segs):
            target_times[index * n_segs + j] = dset._target_times(index, q1, q2, T)
    specs = []
    for lo in range(0, len(file_index), WARPED_BATCH):
        specs.append(dset.windows(file_index[lo:lo + WARPED_BATCH], target_times[lo:lo + WARPED_BATCH]).cpu().numpy())
    specs = np.concatenate(specs)
    onsets, offsets = [q1 for q1, _ in segs], [q2 for _, q2 in segs]      # quantiles are saved, not times
    for index, audio_fn in enumerate(dset.audio_filenames):
        spec_dir = audio_dir_to_spec_dir[os.path.split(audio_fn)[0]]
        if not os.path.exists(spec_dir):
            os.makedirs(spec_dir)
        write_fn = os.path.join(spec_dir, os.path.split(audio_fn)[-1][:-4] + '.npz')
        rows = slice(index * n_segs, (index + 1) * n_segs)
        for data in iter_groups(specs[rows], onsets, offsets, [audio_fn] * n_segs, n_segs):
            np.savez(write_fn, **data)
    return len(file_index)


def segment_sylls_from_warped_songs(warped_window_dset, audio_dirs, spec_dirs, time_bins=512, num_specs=3,
                                    img_fn='temp.pdf', verbose=True, *, quantiles=None):
    """Mirror of ``ava.segmenting.template_segmentation.segment_sylls_from_warped_songs`` (lines 630-755; same
    arguments, prompts and prints) on a ``warped_window.DeviceWarpedWindowDataset``: the user enters quantiles of the
    warped motif, and for every recording the time-warped spectrogram between each pair of neighbouring quantiles is
    saved.  All recordings x all quantile pairs go through ``windows()`` in batches of ``WARPED_BATCH``.  Per recording
    one file ``<name>.npz`` in its ``spec_dir`` holds ``specs``, ``onsets``, ``offsets`` (the quantiles, as the reference
    saves them) and ``audio_filenames``, written as ``preprocess.process_sylls`` writes (``.npz`` where the reference
    writes ``.hdf5``), so ``get_syllable_partition`` / ``DeviceSyllableDataset`` read the directory.

    ``quantiles`` (keyword-only, no counterpart in the reference): cut at these quantiles without a picture or a prompt.
    Fewer than two quantiles raise ``ValueError`` (the reference asserts)."""
    dset = warped_window_dset
    for audio_fn in dset.audio_filenames:
        assert os.path.split(audio_fn)[0] in audio_dirs, "Cannot find " + os.path.split(audio_fn)[0] + " in audio_dirs!"
    start_q, stop_q = dset.start_q, dset.stop_q
    p = dset.p
    if quantiles is not None:
        quantiles = _check_quantiles(quantiles, start_q, stop_q)
    else:
        import matplotlib.pyplot as plt
        plt.switch_backend('agg')
        error_msg = "Invalid input!\nMust be \'s\' or a float between " + "{0:.2f}".format(start_q) + " and " + \
            "{0:.2f}".format(stop_q) + "."
        quantiles = []
        while True:
            _, axarr = plt.subplots(nrows=num_specs, sharex=True)
            if num_specs == 1:
                axarr = [axarr]
            axarr[0].set_title('Enter segmenting quantiles:')
            for i in range(num_specs):
                plt.sca(axarr[i])
                index = np.random.randint(len(dset.audio_filenames))
                warped_spec = dset.get_whole_warped_spectrogram(dset.audio_filenames[index], time_bins=time_bins)
                plt.imshow(warped_spec, origin='lower', aspect='auto',
                           extent=[start_q, stop_q, p['min_freq'] / 1e3, p['max_freq'] / 1e3])
                for q in quantiles:
                    plt.axvline(x=q, color='red')
                plt.ylabel("Frequency (kHz)")
            plt.xlabel('Warped Time Quantile')
            plt.savefig(img_fn)
            plt.close('all')
            if _ask_quantile(quantiles, start_q, stop_q, [error_msg], blank_redraws=True):
                break
        if len(quantiles) < 2:
            raise ValueError("Not enough quantiles to segment!")
    if verbose:
        print("Making and saving syllable spectrograms...")
    num_saved = _write_warped_sylls(dset, audio_dirs, spec_dirs, quantiles)
    if verbose:
        print("\tSaved " + str(num_saved) + " spectrograms.")
        print("\tDone.")


def install(module=None):
    """Point ``get_template``, ``segment_files``, ``_segment_file``, ``clean_collected_segments``,
    ``clean_collected_data``, ``segment_sylls_from_songs`` and ``segment_sylls_from_warped_songs`` of ``module`` (by
    default ``ava.segmenting.template_segmentation``, imported after the reference package) at this module, and give it
    ``segment_specs``, the batch counterpart of its ``_get_spec``."""
    if module is None:
        import ava.segmenting.template_segmentation as module
    module.get_template = get_template
    module.segment_files = segment_files
    module._segment_file = _segment_file
    module.clean_collected_segments = clean_collected_segments
    module.clean_collected_data = clean_collected_data
    module.segment_specs = segment_specs
    module.segment_sylls_from_songs = segment_sylls_from_songs
    module.segment_sylls_from_warped_songs = segment_sylls_from_warped_songs
    return module
