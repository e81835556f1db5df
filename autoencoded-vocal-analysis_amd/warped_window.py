"""Time-warped shotgun windows of song motifs on the device.

Mirror of the reference's third training mode (examples/finch_warp_mwe.py):

  ``DeviceWarpedWindowDataset``       ava/models/window_vae_dataset.py:358-701  ``WarpedWindowDataset``
  ``get_warped_window_data_loaders``  ava/models/window_vae_dataset.py:297-354
  ``get_specs_and_amplitude_traces``  ava/models/utils.py:337-418               the inputs of the warp fit
  ``template_duration``               the ``template_dur`` of the same function, from the file lengths alone
  ``install``                         points the reference module's class and loader function here

The reference's ``__getitem__`` calls ``get_spec(0.0, template_dur, audio[file], ..., target_times=...)`` for every
window: it transforms the whole motif and interpolates ``num_time_bins`` columns out of it.  Here every motif is
transformed ONCE into a cache in HBM (``files x touched bins x frames x 8`` bytes of fp64 log-magnitudes,
``csrc/warp_spec.hip``), and a batch is one interpolation launch out of that cache under each window's own target times.
The cache is built by the kernels of ``spec.get_spec_batch`` and read by the very interpolation functions that path
uses, so a window is bit-identical to ``get_spec_batch(audio, file, 0.0, template_dur, ..., target_times)``.

On the host stay: the window draw (``np.random`` in the reference's call order, so that a seeded batch is the
reference's batch), the inverse warp (``scipy.interpolate.interp1d`` on ``n x T`` doubles), the knots file, and the
optional warp fit, which is ``affinewarp.PiecewiseWarping.fit`` exactly as the reference calls it when ``affinewarp``
can be imported (``ImportError`` otherwise; ``warp_type='null'`` and ``load_warp=True`` need no fit).  ``fit='device'``
fits the reference's own shift-and-slope warp (``ava/preprocessing/warping.py``) on the device instead
(``ava_amd.warp_fit``, row f12) and needs no affinewarp; with ``warp_params['n_knots'] > 0`` it fits that module's
piecewise-linear warp of ``n_knots + 2`` knots per file (row f14).

Not mirrored: ``write_hdf5_files`` (``h5py`` is no dependency of this package).  Limits as ``spec.get_spec_batch``:
``nperseg`` in 64..2048, at most 512 target times per window (``NotImplementedError``); the fit inputs need ``nperseg``
a power of two.  There is no CPU fallback.
"""
import ctypes
import os
import warnings

import numpy as np
import torch

from . import _lib
from . import segment as _seg
from .spec import (EPSILON as SPEC_EPSILON, DeviceAudio, DeviceWindowLoader, _check_stft_shape, _index_list,
                   _is_wav_file, _quantile_index, _read_wav, _stft_constants, _upload, _workspace, target_freqs_of)

__all__ = ["EPSILON", "DEFAULT_WARP_PARAMS", "DeviceWarpedWindowDataset", "get_warped_window_data_loaders",
           "get_specs_and_amplitude_traces", "template_duration", "install"]

EPSILON = 1e-9                       # window_vae_dataset.py:36, models/utils.py
DEFAULT_WARP_PARAMS = {              # window_vae_dataset.py:28-33
    'n_knots': 0,
    'warp_reg_scale': 1e-2,
    'smoothness_reg_scale': 1e-1,
    'l2_reg_scale': 1e-7,
}


def _get_wavs_from_dir(d):
    """models/utils.py:433-436"""
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if _is_wav_file(f)]


def template_duration(lengths, fs, p):
    """``template_dur`` of ``_get_specs_and_amplitude_traces`` (models/utils.py:401-407) for files of these lengths:
    the smallest frame count of scipy.signal.stft over the files times its time step."""
    nperseg, noverlap = int(p['nperseg']), int(p['noverlap'])
    lengths = np.asarray(lengths, dtype=np.int64)
    assert len(lengths) > 0                                                         # models/utils.py:400
    if (lengths < nperseg).any():
        raise ValueError("a motif file has fewer than nperseg = %d samples" % nperseg)
    num_time_bins = int(_seg.frame_count(lengths, nperseg, noverlap).min())
    return num_time_bins * _seg.frame_step(fs, nperseg, noverlap)


def get_specs_and_amplitude_traces(all_audio, fs, spec_params, device="cuda"):
    """``_get_specs_and_amplitude_traces`` (models/utils.py:371-418): ``(specs [files, frames, bins], amps
    [files, frames, 1], template_dur)``, with the band spectrogram of every file and its per-frame sums computed on the
    device in fp64 and returned in the dtype the reference holds them in (float32 for int16 / float32 audio).
    ``all_audio``: a list of 1-D arrays or a ``DeviceAudio``."""
    p = spec_params
    nperseg, noverlap = int(p['nperseg']), int(p['noverlap'])
    _seg._check_shape(nperseg, noverlap)
    audio = all_audio if isinstance(all_audio, DeviceAudio) else DeviceAudio(list(all_audio), device)
    template_dur = template_duration(audio.lengths, fs, p)
    f = np.fft.rfftfreq(nperseg, 1 / fs)
    i1, i2 = int(np.searchsorted(f, p['min_freq'])), int(np.searchsorted(f, p['max_freq']))    # models/utils.py:360-361
    if i2 <= i1:
        raise ValueError("empty frequency band [%s, %s)" % (p['min_freq'], p['max_freq']))
    divisor = p['spec_max_val'] - p['spec_min_val'] + EPSILON                      # models/utils.py:366
    T, frame_off = _seg._frame_offsets(audio.lengths, nperseg, noverlap)
    frames, dev = int(frame_off[-1]), audio.device
    lib = _lib.load()
    window, scale = _stft_constants(nperseg, dev)
    fo = torch.from_numpy(frame_off).to(dev)
    spec = torch.empty((i2 - i1, frames), dtype=torch.float64, device=dev)
    fsum = torch.empty(frames, dtype=torch.float64, device=dev)
    rc = lib.ava_warp_band_spec(audio.samples.data_ptr(), audio.code, audio.file_off.data_ptr(), audio.file_len.data_ptr(),
                                fo.data_ptr(), len(audio), frames, nperseg, noverlap, window.data_ptr(), scale, i1, i2,
                                float(p['spec_min_val']), float(divisor), spec.data_ptr(), fsum.data_ptr(),
                                _lib.stream())
    _lib.check(rc, "ava_warp_band_spec")
    dtype = _seg.trace_dtype(audio.dtype)
    spec, fsum = spec.cpu().numpy(), fsum.cpu().numpy()
    return _stack_specs_and_amps(spec, fsum, frame_off, dtype) + (template_dur,)


def _stack_specs_and_amps(spec, fsum, frame_off, dtype):
    """models/utils.py:399-417 on the band spectrogram [bins, all frames] and the band sums [all frames] of all files"""
    min_time_bins = int(np.diff(frame_off).min())
    specs = np.stack([spec[:, frame_off[i]:frame_off[i] + min_time_bins].T for i in range(len(frame_off) - 1)])
    amps = []
    for i in range(len(frame_off) - 1):
        amp_trace = fsum[frame_off[i]:frame_off[i] + min_time_bins].astype(dtype).reshape(-1, 1)
        amp_trace -= np.min(amp_trace)
        amp_trace /= np.max(amp_trace) + EPSILON
        amps.append(amp_trace)
    return np.ascontiguousarray(specs.astype(dtype)), np.stack(amps)


class DeviceWarpedWindowDataset:
    """``WarpedWindowDataset`` (window_vae_dataset.py:358-701) with the audio and the log-spectrogram of every motif
    resident in HBM.  Same constructor arguments plus ``device`` and ``fit`` (``'affinewarp'``: the reference's fit;
    ``'device'``: ``ava_amd.warp_fit.align_specs``, ``warp_params['n_knots'] + 1`` linear segments per file) (``transform`` is accepted and ignored:
    the items already are fp32 device tensors); ``from_arrays`` builds one from in-memory recordings and knots.

    ``__getitem__(index, seed=None)``: for a list ``index`` one device tensor ``[len(index), F, T]`` (the reference
    returns a list of arrays), for an int ``[F, T]``.  With a ``seed`` the windows are the ones the reference draws."""

    def __init__(self, audio_filenames, p, transform=None, dataset_length=2048, load_warp=False, save_warp=True,
                 start_q=-0.1, stop_q=1.1, warp_fn=None, warp_params={}, warp_type='spectrogram', device="cuda",
                 fit='affinewarp'):
        assert type(p) == type({})                                                   # :402
        assert warp_type in ['amplitude', 'spectrogram', 'null']                     # :403
        assert fit in ['affinewarp', 'device']
        self.audio_filenames = sorted(audio_filenames)                               # :404
        audio = [_read_wav(fn)[1] for fn in self.audio_filenames]                    # :407
        fs = _read_wav(self.audio_filenames[0])[0]                                   # :408: the first SORTED name
        self.transform = transform
        self._setup(audio, fs, p, dataset_length, start_q, stop_q, warp_fn, warp_params, device)
        self._compute_warp(load_warp=load_warp, save_warp=save_warp, warp_type=warp_type, fit=fit)
        self._finish()

    @classmethod
    def from_arrays(cls, audio, fs, p, x_knots=None, y_knots=None, template_dur=None, dataset_length=2048, start_q=-0.1,
                    stop_q=1.1, warp_params={}, device="cuda"):
        """A dataset over in-memory motifs.  Without knots: the null warp.  ``template_dur`` defaults to the
        reference's (``template_duration``)."""
        assert type(p) == type({})
        self = cls.__new__(cls)
        self.audio_filenames = ["<array %d>" % i for i in range(len(audio))]
        self.transform = None
        self._setup(list(audio), fs, p, dataset_length, start_q, stop_q, None, warp_params, device)
        if (x_knots is None) != (y_knots is None):
            raise ValueError("give both x_knots and y_knots, or neither")
        if x_knots is None:
            x_knots = np.zeros((len(audio), 2))
            x_knots[:, 1] = 1.0
            y_knots = np.copy(x_knots)
        self.x_knots = np.asarray(x_knots, dtype=np.float64)
        self.y_knots = np.asarray(y_knots, dtype=np.float64)
        self.template_dur = template_duration(self._lengths, fs, p) if template_dur is None else template_dur
        self._finish()
        return self

    def _setup(self, audio, fs, p, dataset_length, start_q, stop_q, warp_fn, warp_params, device):
        self._host_audio = [np.ascontiguousarray(a) for a in audio]
        self._lengths = np.array([len(a) for a in self._host_audio], dtype=np.int64)
        self.fs = fs
        self.dataset_length = dataset_length
        self.p = p
        self.start_q = start_q
        self.stop_q = stop_q
        self.warp_fn = warp_fn
        self.warp_params = {**DEFAULT_WARP_PARAMS, **warp_params}                    # :415
        self.device = torch.device(device)
        self._audio = None
        self._cache = None

    def _finish(self):
        if self.x_knots.shape != self.y_knots.shape or self.x_knots.ndim != 2 or len(self.x_knots) != len(self._lengths):
            raise ValueError("expected x_knots and y_knots of shape [files, knots]")
        if not (np.diff(self.y_knots, axis=1) > 0).all():       # the reference's interp1d divides by zero here
            raise ValueError("y_knots must be strictly increasing for every file")
        _check_stft_shape(self.p, self.p['num_time_bins'])
        self.window_frac = self.p['window_length'] / self.template_dur               # :418
        self._target_freqs = target_freqs_of(self.p)

    def __len__(self):
        """NOTE: length is arbitrary (window_vae_dataset.py:421-423)"""
        return self.dataset_length

    # ---- the warp (host) ----------------------------------------------------------------------------------------------

    @property
    def audio(self):
        """the motifs as a ``DeviceAudio`` (uploaded on first use)"""
        if self._audio is None:
            self._audio = DeviceAudio(self._host_audio, self.device)
        return self._audio

    def _compute_warp(self, load_warp=False, save_warp=True, warp_type='spectrogram', fit='affinewarp'):
        """window_vae_dataset.py:480-586.  ``fit='device'``: where the reference fits affinewarp's ``PiecewiseWarping``,
        fit the warp of ``ava_amd.warp_fit`` with ``n_knots + 2`` knots instead (with ``n_knots: 0`` shift and slope, the
        same family of warps; above that a piecewise-linear warp, but on fixed template knots and under that module's
        penalties, not affinewarp's)."""
        if save_warp:
            assert self.warp_fn is not None, "``warp_fn`` must be specified to save warps!"
        if warp_type == 'null':
            knots = np.zeros((len(self._lengths), 2))
            knots[:, 1] = 1.0
            self.x_knots = knots
            self.y_knots = np.copy(knots)
            self.template_dur = template_duration(self._lengths, self.fs, self.p)
            print("Made null warp.")
            if save_warp:
                print("Saving warp to:", self.warp_fn)
                to_save = {
                    'x_knots': self.x_knots,
                    'y_knots': self.y_knots,
                    'template_dur': self.template_dur,
                    'audio_filenames': self.audio_filenames,
                    'warp_params': self.warp_params,
                }
                np.save(self.warp_fn, to_save)
            return
        if load_warp:
            if self.warp_fn is None:
                warnings.warn("Tried to load warps, but ``warp_fns`` is None.", UserWarning)
            else:
                try:
                    data = np.load(self.warp_fn, allow_pickle=True).item()
                    self.x_knots = data['x_knots']
                    self.y_knots = data['y_knots']
                    self.template_dur = data['template_dur']
                    temp_fns = data['audio_filenames']
                    assert np.all(temp_fns[:-1] <= temp_fns[1:]), "Filenames in " + self.warp_fn + " are not sorted!"
                    assert len(temp_fns) >= len(self.audio_filenames)
                    if len(temp_fns) == len(self.audio_filenames):
                        assert np.array_equal(temp_fns, self.audio_filenames), \
                            "Input filenames do not match saved filenames!"
                    else:
                        unique_fns = np.unique(self.audio_filenames)
                        assert len(self.audio_filenames) == len(unique_fns)
                        perm = np.zeros(len(self.audio_filenames), dtype='int')
                        for i in range(len(self.audio_filenames)):
                            assert self.audio_filenames[i] in temp_fns, \
                                "Could not find filename " + self.audio_filenames[i] + " in saved warps!"
                            perm[i] = temp_fns.index(self.audio_filenames[i])
                        self.x_knots = self.x_knots[perm]
                        self.y_knots = self.y_knots[perm]
                    if type(self.audio_filenames) == type(np.array([])):
                        self.audio_filenames = self.audio_filenames.tolist()
                    self.warp_params = data['warp_params']
                    return
                except IOError:
                    warnings.warn("Can't load warps from: " + str(self.warp_fn), UserWarning)
        if fit == 'device':
            return self._fit_on_device(warp_type, save_warp)
        try:
            from affinewarp import PiecewiseWarping
        except ImportError as e:
            raise ImportError("fitting a time warp needs the affinewarp package; without it use load_warp=True with "
                              "a saved knots file (warp_fn) or warp_type='null'") from e
        specs, amps, template_dur = get_specs_and_amplitude_traces(self.audio, self.fs, self.p)
        self.template_dur = template_dur
        model = PiecewiseWarping(**self.warp_params)
        if warp_type == 'amplitude':
            print("Computing amplitude warp:", amps.shape)
            model.fit(amps, iterations=50, warp_iterations=200)
        elif warp_type == 'spectrogram':
            print("Computing spectrogram warp:", specs.shape)
            model.fit(specs, iterations=50, warp_iterations=200)
        else:
            raise NotImplementedError
        self.x_knots = model.x_knots
        self.y_knots = model.y_knots
        if save_warp:
            print("Saving warp to:", self.warp_fn)
            to_save = {
                'x_knots': self.x_knots,
                'y_knots': self.y_knots,
                'template_dur': self.template_dur,
                'audio_filenames': self.audio_filenames,
                'amplitude_traces': amps,
                'warp_params': self.warp_params,
            }
            np.save(self.warp_fn, to_save)

    def _fit_on_device(self, warp_type, save_warp):
        """The fit of ``fit='device'``: ``warp_fit.align_specs`` on the spectrograms (``warp_type='spectrogram'``) or the
        amplitude traces (``'amplitude'``) of ``get_specs_and_amplitude_traces`` as ``[files, bins, frames]``, under the
        schedule ``warp_params['shift_lambdas']`` / ``['slope_lambdas']`` (default: ``warp_fit.DEFAULT_*_LAMBDAS``);
        with ``warp_params['n_knots']`` inner knots: ``[files, n_knots + 2]`` knots, for ``n_knots: 0`` the shift and
        slope as two knots per file.  ``warp_reg_scale``, ``smoothness_reg_scale`` and ``l2_reg_scale`` are not read.
        The saved dict has the reference's keys."""
        from . import warp_fit
        shift_λs, slope_λs = warp_fit.check_schedule(self.warp_params.get('shift_lambdas', warp_fit.DEFAULT_SHIFT_LAMBDAS),
                                                     self.warp_params.get('slope_lambdas', warp_fit.DEFAULT_SLOPE_LAMBDAS))
        specs, amps, template_dur = get_specs_and_amplitude_traces(self.audio, self.fs, self.p)
        self.template_dur = template_dur
        if warp_type == 'amplitude':
            print("Computing amplitude warp:", amps.shape)
            fit_input = amps
        elif warp_type == 'spectrogram':
            print("Computing spectrogram warp:", specs.shape)
            fit_input = specs
        else:
            raise NotImplementedError
        _, fitted = warp_fit.align_specs(np.ascontiguousarray(fit_input.transpose(0, 2, 1)), shift_λs, slope_λs,
                                         verbose=False, n_knots=int(self.warp_params.get('n_knots', 0)))
        self.x_knots, self.y_knots = warp_fit.knots_from_warp_params(fitted, fit_input.shape[1])
        if save_warp:
            print("Saving warp to:", self.warp_fn)
            to_save = {
                'x_knots': self.x_knots,
                'y_knots': self.y_knots,
                'template_dur': self.template_dur,
                'audio_filenames': self.audio_filenames,
                'amplitude_traces': amps,
                'warp_params': self.warp_params,
            }
            np.save(self.warp_fn, to_save)

    def _get_unwarped_times(self, y_vals, index):
        """window_vae_dataset.py:461-477: warped (template) quantile times -> measured quantile times of file ``index``"""
        from scipy.interpolate import interp1d
        x_knots, y_knots = self.x_knots[index], self.y_knots[index]
        interp = interp1d(y_knots, x_knots, bounds_error=False, fill_value='extrapolate', assume_sorted=True)
        return interp(y_vals)

    def _target_times(self, file_index, start_t, stop_t, time_bins):
        t_vals = np.linspace(start_t, stop_t, time_bins)
        target_ts = self._get_unwarped_times(t_vals, file_index)
        target_ts *= self.template_dur
        return target_ts

    def _draw(self, n, seed=None):
        """``(file indices [n], target_times [n, T])`` of ``n`` windows: the reference's draw, call for call on
        ``np.random`` (window_vae_dataset.py:615-627, 637)"""
        T = self.p['num_time_bins']
        file_index, target_times = np.empty(n, dtype=np.int64), np.empty((n, T))
        np.random.seed(seed)
        for i in range(n):
            file_index[i] = np.random.randint(len(self._lengths))
            start_t = self.start_q + np.random.rand() * (self.stop_q - self.start_q - self.window_frac)
            stop_t = start_t + self.window_frac
            target_times[i] = self._target_times(file_index[i], start_t, stop_t, T)
        np.random.seed(None)
        return file_index, target_times

    # ---- the device ---------------------------------------------------------------------------------------------------

    def _cache_geometry(self):
        nperseg, noverlap = _check_stft_shape(self.p)
        tf = self._target_freqs
        return (len(self._lengths), float(self.template_dur), float(self.fs), nperseg, noverlap), (float(tf.min()), float(tf.max()))

    def build_cache(self):
        """Transform every motif once: the cache tensor (uint8, ``cache_bytes`` long).  Called on first use."""
        geo, band = self._cache_geometry()
        lib, audio = _lib.load(), self.audio
        nbytes = lib.ava_warp_cache_bytes(*geo, *band)
        wbytes = lib.ava_warp_cache_workspace_bytes(*geo)
        if nbytes == 0 or wbytes == 0:
            raise _lib.AvaHipError("ava_warp_cache_bytes: unsupported shape")
        window, scale = _stft_constants(geo[3], self.device)
        cache = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)       # padding included: two builds are equal bytes
        ws = _lib.workspace(wbytes, self.device, "warp cache")
        rc = lib.ava_warp_cache_build(audio.samples.data_ptr(), audio.code, audio.file_off.data_ptr(),
                                      audio.file_len.data_ptr(), *geo, window.data_ptr(), scale, *band, 1,
                                      cache.data_ptr(), cache.numel(), ws.data_ptr(), ws.numel(), _lib.stream())
        _lib.check(rc, "ava_warp_cache_build")
        self._cache = cache
        return cache

    @property
    def cache_bytes(self):
        """HBM footprint of the motif cache: about files x touched bins x frames x 8 bytes"""
        geo, band = self._cache_geometry()
        return int(_lib.load().ava_warp_cache_bytes(*geo, *band))

    def cache_rows(self, file):
        """The cached fp64 log-magnitudes ``[touched bins, frames]`` of one file (a view into the cache)"""
        if self._cache is None:
            self.build_cache()
        geo, band = self._cache_geometry()
        lay = (ctypes.c_int64 * 6)()
        _lib.check(_lib.load().ava_warp_cache_layout(*geo, *band, lay), "ava_warp_cache_layout")
        _, fstride, _, nb, _, off_logmag = lay
        files = geo[0]
        base = (-self._cache.data_ptr()) % 256                                       # the library aligns the buffer itself
        nframes = int(self._cache[base:base + 4 * files].view(torch.int32)[file])
        logmag = self._cache[base + off_logmag:base + off_logmag + 8 * files * nb * fstride].view(torch.float64)
        return logmag.view(files, nb, fstride)[file, :, :max(nframes, 0)]

    def windows(self, file_index, target_times):
        """The fp32 device batch ``[n, F, T]`` of the windows ``(file_index [n], target_times [n, T])``: one
        interpolation launch out of the cache.  Enqueued on the current stream; nothing synchronises."""
        file_index = np.ascontiguousarray(file_index, dtype=np.int32).reshape(-1)
        target_times = np.ascontiguousarray(target_times, dtype=np.float64)
        n, p, tf = file_index.shape[0], self.p, self._target_freqs
        F, T = tf.shape[0], target_times.shape[-1]
        if n == 0:
            raise ValueError("empty batch")
        if target_times.shape != (n, T):
            raise ValueError("inconsistent batch shapes")
        if file_index.min() < 0 or file_index.max() >= len(self._lengths):
            raise IndexError("file index out of range")
        _check_stft_shape(p, T)
        if self._cache is None:
            self.build_cache()
        geo, band = self._cache_geometry()
        lib, dev = _lib.load(), self.device
        normalize, q_lo, q_gamma = _quantile_index(p, F, T)
        (d_tf, d_tt), fidx = _upload(dev, [tf, target_times], file_index)
        ws = _workspace(dev, lib.ava_warp_windows_workspace_bytes(n, F, T, normalize))
        out = torch.empty((n, F, T), dtype=torch.float32, device=dev)
        rc = lib.ava_warp_windows(self._cache.data_ptr(), self._cache.numel(), *geo, *band, fidx.data_ptr(),
                                  d_tt.data_ptr(), n, d_tf.data_ptr(), F, T, float(p['spec_min_val']),
                                  float(p['spec_max_val']), float(-1 / SPEC_EPSILON), normalize, q_lo, q_gamma,
                                  out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream())
        _lib.check(rc, "ava_warp_windows")
        return out

    def __getitem__(self, index, seed=None):
        index, single_index = _index_list(index)
        file_index, target_times = self._draw(len(index), seed)
        specs = self.windows(file_index, target_times)
        return specs[0] if single_index else specs

    def _specific_times(self, query_filename, quantile):
        """``(file index, target_times)`` of ``get_specific_item`` (window_vae_dataset.py:659-666)"""
        file_index = self.audio_filenames.index(query_filename)
        start_t = self.start_q + quantile * (self.stop_q - self.start_q - self.window_frac)
        stop_t = start_t + self.window_frac
        return file_index, self._target_times(file_index, start_t, stop_t, self.p['num_time_bins'])

    def _whole_times(self, query_filename, time_bins):
        """``(file index, target_times)`` of ``get_whole_warped_spectrogram`` (window_vae_dataset.py:691-695)"""
        file_index = self.audio_filenames.index(query_filename)
        return file_index, self._target_times(file_index, self.start_q, self.stop_q, time_bins)

    def get_specific_item(self, query_filename, quantile):
        """window_vae_dataset.py:643-672: the window at ``quantile`` of one file, as a numpy array"""
        file_index, target_ts = self._specific_times(query_filename, quantile)
        return self.windows([file_index], target_ts[None, :])[0].cpu().numpy().astype(np.float64)

    def get_whole_warped_spectrogram(self, query_filename, time_bins=128):
        """window_vae_dataset.py:675-701: an entire warped motif, as a numpy array"""
        file_index, target_ts = self._whole_times(query_filename, time_bins)
        return self.windows([file_index], target_ts[None, :])[0].cpu().numpy().astype(np.float64)


def get_warped_window_data_loaders(audio_dirs, p, batch_size=64, num_workers=4, load_warp=False, warp_fn=None,
                                   warp_params={}, warp_type='spectrogram', device="cuda", fit='affinewarp'):
    """Mirror of window_vae_dataset.py:297-354: ``{'train': loader, 'test': loader}``, the same loader twice, over a
    ``DeviceWarpedWindowDataset`` of the wav files of ``audio_dirs``.  ``fit``: as the dataset's."""
    assert type(p) == type({})
    assert warp_type in ['amplitude', 'spectrogram', 'null']
    assert fit in ['affinewarp', 'device']
    audio_fns = []
    for audio_dir in audio_dirs:
        audio_fns += _get_wavs_from_dir(audio_dir)
    dataset = DeviceWarpedWindowDataset(audio_fns, p, load_warp=load_warp, warp_fn=warp_fn, warp_params=warp_params,
                                        warp_type=warp_type, device=device, fit=fit)
    dataloader = DeviceWindowLoader(dataset, batch_size=batch_size, shuffle=True, num_workers=num_workers)
    return {'train': dataloader, 'test': dataloader}


def install(module=None):
    """Point ``WarpedWindowDataset`` and ``get_warped_window_data_loaders`` of ``module`` (by default
    ``ava.models.window_vae_dataset``; the reference module imports affinewarp and h5py at import time, so a module
    object may be passed instead) at this module."""
    if module is None:
        import ava.models.window_vae_dataset as module
    module.WarpedWindowDataset = DeviceWarpedWindowDataset
    module.get_warped_window_data_loaders = get_warped_window_data_loaders
    return module
