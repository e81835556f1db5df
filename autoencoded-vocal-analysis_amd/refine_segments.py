"""Removal of noise segments before a VAE is trained, computed on the device.

Mirror of the reference's ``ava/segmenting/refine_segments.py``:

  ``get_specs``                ``_get_specs`` (:232-306): one band spectrogram per segment, zero-padded / truncated
  ``embed``                    the ``umap.UMAP(...).fit_transform`` of :79-86, as a ``projection.TransformableUMAP``
  ``update_segments``          ``_update_segs_helper`` + ``_write_segs`` + ``_in_bounds`` (:338-435)
  ``refine_segments_pre_vae``  :32-124, same signature, same prompts, same grid picture
  ``install``                  points the reference module's three functions here

The segments of all files go through the band-spectrogram kernel of ``segment`` in batches (``csrc/segment.hip``), the
embedding and the ``transform`` of every directory's segments through ``csrc/projection.hip``; neither umap-learn nor
numba is needed.  The spectrograms stay on the device from the STFT to the kNN.

Directories are processed one after the other in this process.  The reference hands them to ``joblib.Parallel`` with up
to ``cpu_count - 1`` workers; here every worker would open the GPU, which shared machines do not allow, and the work of
a directory is device work anyway.

There is no CPU fallback.
"""
import os
import warnings

import numpy as np
import torch

from . import projection, segment
from .spec import _read_wav

__all__ = ["get_specs", "embed", "update_segments", "refine_segments_pre_vae", "install", "in_bounds"]


def _audio_seg_filenames(audio_dirs, seg_dirs):
    """segmenting/utils.py:370-397"""
    assert len(audio_dirs) == len(seg_dirs), f"{len(audio_dirs)} != {len(seg_dirs)}"
    audio_fns, seg_fns = [], []
    for audio_dir, seg_dir in zip(audio_dirs, seg_dirs):
        names = [i for i in sorted(os.listdir(audio_dir)) if i.endswith('.wav')]
        audio_fns += [os.path.join(audio_dir, i) for i in names]
        seg_fns += [os.path.join(seg_dir, i[:-4] + '.txt') for i in names]
    return audio_fns, seg_fns


def _read_onsets_offsets(filename):
    """segmenting/utils.py:407-429"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)              # numpy's "input contained no data"
        arr = np.loadtxt(filename, skiprows=1)
    if len(arr) == 0:
        return [], []
    if len(arr.shape) == 1:
        arr = arr.reshape(1, 2)
    assert arr.shape[1] == 2, "Found invalid shape: " + str(arr.shape)
    return arr[:, 0], arr[:, 1]


def _collect(audio_dirs, seg_dirs, p, max_num_specs):
    """the host half of ``_get_specs``: (audio slices, segment file names, onsets) of the kept segments, files in the
    seed-42 order, stopping at ``max_num_specs``"""
    audio_fns, seg_fns = _audio_seg_filenames(audio_dirs, seg_dirs)
    audio_fns, seg_fns = np.array(audio_fns), np.array(seg_fns)
    perm = np.random.RandomState(42).permutation(len(audio_fns))     # np.random.seed(42); np.random.permutation
    audio_fns, seg_fns = audio_fns[perm], seg_fns[perm]
    slices, all_fns, onsets_kept = [], [], []
    for audio_fn, seg_fn in zip(audio_fns, seg_fns):
        onsets, offsets = _read_onsets_offsets(seg_fn)
        fs, audio = _read_wav(audio_fn)
        assert len(audio) >= p['nperseg'], "Short audio file: " + audio_fn + ", duration: " + str(len(audio) / fs)
        for onset, offset in zip(onsets, offsets):
            i1, i2 = int(onset * fs), int(offset * fs)
            if i2 - i1 <= p['nperseg']:
                continue
            assert i1 >= 0, audio_fn + ", " + seg_fn
            piece = audio[i1:i2]
            assert len(piece) >= p['nperseg'], "len(audio): " + str(len(piece)) + ", nperseg: " + str(p['nperseg'])
            slices.append(piece)
            all_fns.append(os.path.split(seg_fn)[-1])
            onsets_kept.append(onset)
            if max_num_specs is not None and len(slices) >= max_num_specs:
                break
        if max_num_specs is not None and len(slices) >= max_num_specs:
            break
    assert len(slices) > 0, "Found no spectrograms!"
    return slices, all_fns, onsets_kept


def get_specs(audio_dirs, seg_dirs, p, max_num_specs=None, max_len=None, return_segs=False, device='cuda',
              max_chunk_bytes=segment.DEFAULT_CHUNK_BYTES):
    """Mirror of ``_get_specs``: the band spectrogram (``segmenting/utils.py:get_spec``) of every segment longer than
    ``nperseg`` samples, files in the reference's seed-42 order, at most ``max_num_specs`` of them, zero-padded or
    truncated to ``max_len`` time bins (default: the longest).

    Returns ``(specs, max_len, all_fns)`` and ``segs`` (``[N, 2]``: onset, onset + dt max_len) with ``return_segs``.
    ``specs`` is one device tensor ``[N, F, max_len]`` where the reference returns a list of ``N`` arrays: float64, as
    the reference's zero-padded arrays are, holding the values of the reference's spectrogram dtype (float32-rounded
    for int16 / float32 audio).  The audio slices go to the device in batches of at most ``max_chunk_bytes``; the
    result does not depend on the batching."""
    slices, all_fns, onsets = _collect(audio_dirs, seg_dirs, p, max_num_specs)
    specs, max_len, dt = segment.padded_specs(slices, p, max_len, device, max_chunk_bytes)
    segs = np.array([[onset, onset + dt * max_len] for onset in onsets])
    if return_segs:
        return specs, max_len, all_fns, segs
    return specs, max_len, all_fns


def embed(specs, n_neighbors=20, min_dist=0.1):
    """``(transform, embedding)``: a ``projection.TransformableUMAP`` with the reference's arguments (:79-80) fitted
    to the flattened spectrograms, and their float32 ``[N, 2]`` embedding.  The object keeps the float32 rows on the
    device (``N x F x max_len x 4`` bytes) for its ``transform``."""
    transform = projection.TransformableUMAP(n_components=2, n_neighbors=n_neighbors, min_dist=min_dist,
                                             metric='euclidean', random_state=42)
    rows = specs.reshape(len(specs), -1)
    return transform, transform.fit_transform(rows)


def in_bounds(point, bounds):
    """is the point strictly inside one of the rectangles ``bounds['x1'][i] .. ['x2'][i]`` x ``['y1'][i] .. ['y2'][i]``"""
    return any(x1 < point[0] < x2 and y1 < point[1] < y2
               for x1, x2, y1, y2 in zip(bounds['x1'], bounds['x2'], bounds['y1'], bounds['y2']))


def _write_segs(segs, out_fn, header_fn):
    np.savetxt(out_fn, np.stack([np.array(seg) for seg in segs]), fmt='%.5f',
               header="Cleaned onsets/offsets for " + header_fn)


def update_segments(seg_dir, audio_dir, out_seg_dir, p, max_len, transform, bounds, verbose=True):
    """Mirror of ``_update_segs_helper``: embed every segment of one directory with ``transform.transform(rows)``
    (any object with that method; ``rows`` is a device tensor ``[N, F max_len]``) and copy the lines of the segment
    files whose points lie in none of the rectangles of ``bounds`` to files of the same names in ``out_seg_dir``.

    Two things are the reference's and kept: a file none of whose segments survives gets no output file, and the line
    copied for the i-th *spectrogram* of a file is that file's i-th *line*, so a segment skipped for being no longer
    than ``nperseg`` shifts the lines after it.  The header names ``audio_dir`` joined with the segment file's name."""
    if verbose:
        print("Updating segments in:", seg_dir)
    if not os.path.exists(out_seg_dir):
        os.makedirs(out_seg_dir)
    specs, _, all_fns = get_specs([audio_dir], [seg_dir], p, max_len=max_len)
    points = transform.transform(specs.reshape(len(specs), -1))
    points = points.cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    out_segs, prev_fn, prev_segs, index = [], None, None, 0

    def flush():
        if len(out_segs) > 0:
            _write_segs(out_segs, os.path.join(out_seg_dir, prev_fn), os.path.join(audio_dir, prev_fn))

    for fn, point in zip(all_fns, points):
        if fn != prev_fn:
            flush()
            out_segs = []
            prev_fn = fn
            prev_segs = np.loadtxt(os.path.join(seg_dir, fn)).reshape(-1, 2)
            index = 0
        if not in_bounds(point, bounds):
            out_segs.append(prev_segs[index])
        index += 1
    flush()


def _grid_limits(lo, hi, delta):
    lo, hi = int(np.floor(lo)), int(np.ceil(hi))
    if lo % delta != 0:
        lo -= lo % delta
    if hi % delta != 0:
        hi -= (hi % delta) - delta
    return lo, hi


def _plot_helper(embedding, colors, title="", filename='temp.pdf', verbose=True):
    """the scatter plot with grid lines of ``_plot_helper`` (:309-335)"""
    import matplotlib.pyplot as plt
    plt.switch_backend('agg')
    plt.scatter(embedding[:, 0], embedding[:, 1], c=colors, s=0.9, alpha=0.7)
    delta = 5 if np.max(embedding) - np.min(embedding) > 20 else 1
    x_lo, x_hi = _grid_limits(np.min(embedding[:, 0]), np.max(embedding[:, 0]), delta)
    y_lo, y_hi = _grid_limits(np.min(embedding[:, 1]), np.max(embedding[:, 1]), delta)
    for x in range(x_lo, x_hi + 1):
        plt.axvline(x=x, lw=0.5, alpha=0.7)
    for y in range(y_lo, y_hi + 1):
        plt.axhline(y=y, lw=0.5, alpha=0.7)
    plt.title(title)
    plt.savefig(filename)
    plt.close('all')
    if verbose:
        print("Grid plot saved to:", filename)


def _get_input(query_str):
    while True:
        try:
            return float(input(query_str))
        except ValueError:
            print("Unrecognized input!")


def _tooltip_plot():
    try:
        from ava.plotting.tooltip_plot import tooltip_plot
        return tooltip_plot
    except ImportError as e:
        warnings.warn("ava.plotting.tooltip_plot cannot be imported (%s): no html plot is written" % e)
        return None


def refine_segments_pre_vae(seg_dirs, audio_dirs, out_seg_dirs, p, n_samples=10000, num_imgs=1000, verbose=True,
                            img_fn='temp.pdf', tooltip_output_dir='temp'):
    """Mirror of ``ava.segmenting.refine_segments.refine_segments_pre_vae`` (same arguments and prompts): embed up to
    ``n_samples`` segment spectrograms with UMAP, let the user box noise regions of the embedding (the grid picture is
    saved to ``img_fn`` after every box; the tooltip plot is written when ``ava.plotting.tooltip_plot`` imports, with a
    warning otherwise), then embed every directory's segments with the fitted object's ``transform`` and copy those
    outside the boxes to ``out_seg_dirs``.

    The directories are processed serially in this process (see the module docstring).  The fitted object keeps
    ``n_samples x F x max_len x 4`` bytes of training rows on the device until this function returns."""
    if verbose:
        print("\nCleaning segments\n-----------------")
        print("Collecting spectrograms...")
    specs, max_len, _ = get_specs(audio_dirs, seg_dirs, p, max_num_specs=n_samples)
    if verbose:
        print("Running UMAP... n =", len(specs))
    transform, embedding = embed(specs)
    if verbose:
        print("\tDone.")
    bounds = {'x1': [], 'x2': [], 'y1': [], 'y2': []}
    colors = ['b'] * len(embedding)
    first_iteration = True
    while True:
        _plot_helper(embedding, colors, verbose=verbose, filename=img_fn)
        if first_iteration:
            first_iteration = False
            tooltip_plot = _tooltip_plot()
            if tooltip_plot is not None:
                if verbose:
                    print("Writing html plot:")
                tooltip_plot(embedding, specs.cpu().numpy(), num_imgs=num_imgs, title="Identify unwanted sounds:",
                             output_dir=tooltip_output_dir, grid=True)
                if verbose:
                    print("\tDone.")
        if input("Press [q] to quit identifying noise or [return] to continue: ") == 'q':
            break
        print("Enter the coordinates of a rectangle containing noise:")
        x1, x2 = _get_input("x1: "), _get_input("x2: ")
        y1, y2 = _get_input("y1: "), _get_input("y2: ")
        bounds['x1'].append(min(x1, x2))
        bounds['x2'].append(max(x1, x2))
        bounds['y1'].append(min(y1, y2))
        bounds['y2'].append(max(y1, y2))
        colors = ['r' if c == 'b' and in_bounds(pt, bounds) else c for c, pt in zip(colors, embedding)]
    del specs
    for seg_dir, audio_dir, out_seg_dir in zip(seg_dirs, audio_dirs, out_seg_dirs):
        update_segments(seg_dir, audio_dir, out_seg_dir, p, max_len, transform, bounds, verbose)


def install(module=None):
    """Point ``_get_specs``, ``_update_segs_helper`` and ``refine_segments_pre_vae`` of
    ``ava.segmenting.refine_segments`` here (the reference module imports umap at import time, so a module object may
    be passed instead).  ``_get_specs`` then returns one device tensor where the reference returns a list."""
    if module is None:
        import ava.segmenting.refine_segments as module
    module._get_specs = get_specs
    module._update_segs_helper = update_segments
    module.refine_segments_pre_vae = refine_segments_pre_vae
    return module
