"""Shotgun-VAE projection movies with the search on the device.

Mirror of the reference's ``ava/plotting/shotgun_movie.py``:

  ``shotgun_movie_embedding``  the compute half of ``shotgun_movie_DC`` (:88-155): windows, spectrograms, latents and
                               the nearest-neighbour search, all on the device
  ``shotgun_movie_DC``         same signature: the embedding, then the reference's matplotlib frame loop and ffmpeg
  ``window_onsets``            the window schedule (:101-111), restated
  ``window_spectrograms``      ``p['get_spec']`` of every window (:105-108), as ``get_spec_batch`` launches
  ``window_latents``           the batch-1 latent means of ``model.get_latent(DataLoader(SimpleDataset(specs)))``
  ``install``                  points ``ava.plotting.shotgun_movie.shotgun_movie_DC`` here

Deviations from the reference, on purpose:

* ``method='re_umap'`` raises ``NotImplementedError``: umap is not a dependency, and the reference module never
  imports it either.
* The second ffmpeg command is the one intended: the reference's ``'...{} -strict ' + '-2 {}'.format(...)`` formats
  only the last literal and leaves ``{}`` in argv.  Both commands are passed as argument lists.
* Without ``ffmpeg`` on PATH a warning is issued and the JPEG frames are kept; the reference raises
  ``FileNotFoundError``.
* For ``'spectrogram_correlation'`` a query whose correlations are all NaN (a silent window) gets index 0 (see
  ``ava_amd.neighbors``); sklearn returns an arbitrary row.

``dc`` is any object with ``request(field)`` and ``model_filename`` (``ava.data.data_container.DataContainer``).
"""
import os
import subprocess
import warnings

import numpy as np
import torch

from .neighbors import nearest
from .spec import DeviceAudio, _read_wav, get_spec_batch

__all__ = ["shotgun_movie_embedding", "shotgun_movie_DC", "window_onsets", "window_spectrograms", "window_latents",
           "ffmpeg_commands", "install", "METHODS"]

METHODS = ['latent_nn', 're_umap', 'spectrogram_correlation']
SPEC_CHUNK = 256                     # windows per get_spec_batch launch


def window_onsets(n_samples, fs, window_length, fps=30, shoulder=0.01):
    """Onsets (seconds) of the movie's windows: shotgun_movie.py:101-111 with the same float accumulation."""
    dt = 1 / fps
    onset = shoulder
    onsets = []
    while onset + window_length < n_samples / fs - shoulder:
        onsets.append(onset)
        onset += dt
    return np.array(onsets, dtype=np.float64)


def window_spectrograms(audio, fs, onsets, p, shoulder=0.01, chunk=SPEC_CHUNK):
    """``p['get_spec'](onset - shoulder, offset + shoulder, audio, p, fs=fs, target_times=linspace(onset, offset, T))``
    of every window (shotgun_movie.py:104-108), on the device: the fp32 tensor ``[n, F, T]``.  ``audio`` is a 1-D
    array or a ``DeviceAudio`` holding the one recording."""
    dev_audio = audio if isinstance(audio, DeviceAudio) else DeviceAudio([np.asarray(audio)])
    onsets = np.asarray(onsets, dtype=np.float64).reshape(-1)
    if len(onsets) == 0:
        raise ValueError("no windows")
    T = p['num_time_bins']
    out = []
    for s in range(0, len(onsets), chunk):
        onset = onsets[s:s + chunk]
        offset = onset + p['window_length']
        target_times = np.linspace(onset, offset, T, axis=-1)
        out.append(get_spec_batch(dev_audio, np.zeros(len(onset), dtype=np.int32), onset - shoulder, offset + shoulder,
                                  p, fs, target_times))
    return out[0] if len(out) == 1 else torch.cat(out)


def window_latents(model_filename, specs):
    """Latent means (float64 ``[n, z]``) of ``specs`` as the reference computes them (shotgun_movie.py:114-120): a VAE
    with the checkpoint's ``z_dim`` (as ``DataContainer._make_latent_means`` builds it), loaded from
    ``model_filename`` and left in its current (train) mode, encodes every window as a batch of one."""
    from .vae import VAE
    map_loc = 'cuda' if torch.cuda.is_available() else 'cpu'
    z_dim = torch.load(model_filename, map_location=map_loc)['z_dim']
    model = VAE(z_dim=z_dim)
    model.load_state(model_filename)
    specs = specs if torch.is_tensor(specs) else torch.from_numpy(np.ascontiguousarray(specs, dtype=np.float32))
    specs = specs.to(device=model.device, dtype=torch.float32)
    latent = torch.empty(len(specs), z_dim, device=model.device)
    with torch.no_grad():
        for i in range(len(specs)):
            mu, _, _ = model.encode(specs[i:i + 1])
            latent[i] = mu[0]
    return latent.cpu().numpy().astype(np.float64)


def shotgun_movie_embedding(dc, audio_file, p, method='spectrogram_correlation', fps=30, shoulder=0.01,
                            chunk_rows=None):
    """The compute half of ``shotgun_movie_DC`` (shotgun_movie.py:88-155): ``(new_embed, original_embed, indices,
    onsets)`` -- the embedding of every window, the embedding it is drawn on, the index of each window's nearest
    syllable and the window onsets in seconds.  ``chunk_rows`` is handed to ``neighbors.nearest``."""
    assert dc.model_filename is not None
    assert method in METHODS
    if method == 're_umap':
        raise NotImplementedError("method 're_umap' needs umap, which this package does not depend on")
    fs, audio = _read_wav(audio_file)
    assert fs == p['fs'], "found fs=" + str(fs) + ", expected " + str(p['fs'])
    onsets = window_onsets(len(audio), fs, p['window_length'], fps, shoulder)
    assert len(onsets) > 0
    specs = window_spectrograms(audio, fs, onsets, p, shoulder)
    if method == 'latent_nn':
        latent = window_latents(dc.model_filename, specs)
        original_embed = dc.request('latent_mean_umap')
        original_latent = dc.request('latent_means')
        indices, _ = nearest(latent, original_latent, 'euclidean', chunk_rows)
        new_embed = np.zeros((len(latent), 2))
        new_embed[:] = np.asarray(original_embed)[indices]
    else:
        original_specs = dc.request('specs')
        print("Finding nearest neighbors:")
        indices, _ = nearest(specs.reshape(len(specs), -1), original_specs, 'correlation', chunk_rows)
        print("\tDone.")
        original_embed = dc.request('latent_mean_umap')
        new_embed = np.asarray(original_embed)[indices]
    return new_embed, original_embed, indices, onsets


def ffmpeg_commands(fps, output_dir, audio_file, mp4_fn='out.mp4'):
    """The two ffmpeg argument lists shotgun_movie.py:182-190 means to run: frames -> temp.mp4, then temp.mp4 plus the
    audio -> ``output_dir/mp4_fn``."""
    img_fns = os.path.join(output_dir, 'viz-%05d.jpg')
    video_fn = os.path.join(output_dir, mp4_fn)
    return [['ffmpeg', '-y', '-r', str(fps), '-i', img_fns, 'temp.mp4'],
            ['ffmpeg', '-y', '-r', str(fps), '-i', 'temp.mp4', '-i', audio_file, '-c:a', 'aac', '-strict', '-2',
             video_fn]]


def shotgun_movie_DC(dc, audio_file, p, method='spectrogram_correlation', output_dir='temp', fps=30, shoulder=0.01,
                     c='b', alpha=0.2, s=0.9, marker_c='r', marker_s=50.0, marker_marker='*', transform_fn=None,
                     load_transform=False, save_transform=False, mp4_fn='out.mp4'):
    """Drop-in for ``ava.plotting.shotgun_movie.shotgun_movie_DC`` (same arguments): one JPEG per window in
    ``output_dir`` and the movie made from them by ffmpeg.  ``transform_fn``, ``load_transform`` and
    ``save_transform`` only concern ``'re_umap'``, which is not supported."""
    import matplotlib
    matplotlib.use('agg', force=False)
    import matplotlib.pyplot as plt
    plt.switch_backend('agg')
    assert dc.model_filename is not None
    assert method in METHODS
    if os.path.exists(output_dir):
        for fn in os.listdir(output_dir):
            if len(fn) > 4 and fn[-4:] == '.jpg':
                os.remove(os.path.join(output_dir, fn))
    new_embed, original_embed, _, _ = shotgun_movie_embedding(dc, audio_file, p, method=method, fps=fps,
                                                              shoulder=shoulder)
    # Calculate x and y limits (shotgun_movie.py:156-164).
    xmin = np.min(original_embed[:, 0])
    ymin = np.min(original_embed[:, 1])
    xmax = np.max(original_embed[:, 0])
    ymax = np.max(original_embed[:, 1])
    x_pad = 0.05 * (xmax - xmin)
    y_pad = 0.05 * (ymax - ymin)
    xmin, xmax = xmin - x_pad, xmax + x_pad
    ymin, ymax = ymin - y_pad, ymax + y_pad
    # Save images (:165-180).
    print("Saving images:")
    if not os.path.exists(output_dir):
        os.mkdir(output_dir)
    for i in range(len(new_embed)):
        plt.scatter(original_embed[:, 0], original_embed[:, 1], c=[c] * len(original_embed), alpha=alpha, s=s)
        plt.scatter([new_embed[i, 0]], [new_embed[i, 1]], s=marker_s, marker=marker_marker, c=marker_c)
        plt.xlim(xmin, xmax)
        plt.ylim(ymin, ymax)
        plt.gca().set_aspect('equal')
        plt.axis('off')
        plt.savefig(os.path.join(output_dir, f"viz-{i:05d}.jpg"))
        plt.close('all')
    print("\tDone.")
    # Make video (:181-190).
    for cmd in ffmpeg_commands(fps, output_dir, audio_file, mp4_fn):
        try:
            process = subprocess.Popen(cmd, stdout=subprocess.PIPE)
        except FileNotFoundError:
            warnings.warn("ffmpeg was not found on PATH: the frames are kept in %s, no movie was made" % output_dir)
            return
        process.communicate()


def install(module=None):
    """Point ``ava.plotting.shotgun_movie.shotgun_movie_DC`` at this module (call after importing the reference
    package; its ``ava.plotting`` needs umap and numba, so a module object may be passed instead)."""
    if module is None:
        import ava.plotting.shotgun_movie as module
    module.shotgun_movie_DC = shotgun_movie_DC
    return module
