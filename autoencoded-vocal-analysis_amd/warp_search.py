"""Searches over the parameters of the device warp fit.

The reference has two searches in ``ava/models/utils.py``: ``cross_validation_warp_parameter_search`` (:48-132), a
wrapper around ``affinewarp.crossval.paramsearch``, and ``anchor_point_warp_parameter_search`` (:135-308), which fits
``affinewarp.PiecewiseWarping`` models and scores them on hand-labelled anchor times.  affinewarp is no dependency here
and its model is not the one ``ava_amd.warp_fit`` fits, so the protocol below is this project's own; it keeps the shape of
the reference's functions and results, and answers the question the fit leaves open: which ``n_knots``,
``shift_lambdas`` and ``slope_lambdas`` to hand ``get_warped_window_data_loaders(..., fit='device')``.

  ``cross_validate``                          the search on an array ``[N, F, T]``
  ``cross_validation_warp_parameter_search``  the reference's signature around it: files in, plot out
  ``best_warp_params``                        the ``warp_params`` of the best sample of a search
  ``anchor_errors``                           the host arithmetic of the anchor score (models/utils.py:294-306)
  ``anchor_point_warp_parameter_search``      the reference's signature and return
  ``install``                                 points a reference module's two functions here

A setting is a knot count and two scales; its schedule is ``scale × base`` for the base schedule of the fit (``inf`` and
0 stay as they are).  Knot count ``-1`` is a shift-only fit: two knots, every ``slope_λ = inf``.  Cross-validation holds
out frequency bins: the fit sees the train bins of all motifs, and the warps it finds are scored on bins it never saw
by ``R² = 1 - SS_res / SS_tot``, ``SS_res`` the squared distance of every warped motif from the mean warped motif and
``SS_tot`` that of every unwarped motif from the bin's mean over motifs and columns.  Every fit of one knot count runs in
one ``warp_fit.align_specs_grouped`` call, and every template and every sum of squares comes from the grouped kernels
of ``csrc/warp_fit.hip``; there is no CPU fallback.
"""
import os
import warnings

import numpy as np
import torch

from . import warp_fit

__all__ = ["DEFAULT_SEARCH_PARAMS", "PARAM_NAMES", "sample_settings", "split_bins", "search_plan", "cross_validate",
           "cross_validation_warp_parameter_search", "best_warp_params", "anchor_errors",
           "anchor_point_warp_parameter_search", "install"]

DEFAULT_SEARCH_PARAMS = {            # models/utils.py:23-35 and, below the blank line, this module's own keys
    'samples_per_knot': 10,
    'n_valid_samples': 5,
    'n_train_folds': 3,
    'n_valid_folds': 1,
    'n_test_folds': 1,
    'knot_range': (-1, 2),
    'smoothness_range': (1e-1, 1e2),     # the four affinewarp keys are accepted and not read
    'warpreg_range': (1e-1, 1e2),
    'iter_range': (50, 51),
    'warp_iter_range': (50, 101),
    'outfile': None,

    'shift_range': (1e-1, 1e1),          # the scale of the shift_λ schedule, drawn log-uniformly
    'slope_range': (1e-1, 1e1),          # the scale of the slope_λ schedule
    'shift_lambdas': warp_fit.DEFAULT_SHIFT_LAMBDAS,
    'slope_lambdas': warp_fit.DEFAULT_SLOPE_LAMBDAS,
}

PARAM_NAMES = ['n_knots', 'shift_scale', 'slope_scale']         # the columns of param_history


def _schedule(knots, shift_scale, slope_scale, base_shift, base_slope):
    """``scale × base`` (``inf`` and 0 stay); knot count -1: every slope_λ is ``inf``"""
    with np.errstate(invalid='ignore'):
        shift = [float(v) if v == 0 or np.isinf(v) else float(shift_scale * v) for v in base_shift]
        slope = [float(v) if v == 0 or np.isinf(v) else float(slope_scale * v) for v in base_slope]
    if knots < 0:
        slope = [np.inf] * len(slope)
    return shift, slope


def sample_settings(search_params, rng):
    """The sampled settings of a search: for every knot count of ``range(*knot_range)`` in order, ``samples_per_knot``
    times one log-uniform draw from ``shift_range`` and then one from ``slope_range``.  Returns ``(knots [S] int,
    shift_scale [S], slope_scale [S], schedules)``, ``schedules[s] = (shift_λs, slope_λs)`` as lists of floats."""
    p = {**DEFAULT_SEARCH_PARAMS, **search_params}
    base_shift, base_slope = warp_fit.check_schedule(p['shift_lambdas'], p['slope_lambdas'])
    knots, a, b, schedules = [], [], [], []
    for k in range(*p['knot_range']):
        if k < -1:
            raise ValueError("knot counts start at -1 (a shift-only fit), got %d" % k)
        for _ in range(int(p['samples_per_knot'])):
            a.append(float(np.exp(rng.uniform(np.log(p['shift_range'][0]), np.log(p['shift_range'][1])))))
            b.append(float(np.exp(rng.uniform(np.log(p['slope_range'][0]), np.log(p['slope_range'][1])))))
            knots.append(k)
            schedules.append(_schedule(k, a[-1], b[-1], base_shift, base_slope))
    if not knots:
        raise ValueError("the search has no settings: knot_range %r, samples_per_knot %r"
                         % (p['knot_range'], p['samples_per_knot']))
    return np.array(knots, dtype=int), np.array(a), np.array(b), schedules


def split_bins(F, n_train_folds, n_valid_folds, n_test_folds, rng):
    """One split of the bins ``0 .. F-1``: a permutation cut by ``np.array_split`` into ``n_train + n_valid + n_test``
    folds, the first ``n_train`` of which are the train bins, the next ``n_valid`` the validation bins and the rest the
    test bins.  Returns three sorted int arrays.  ``ValueError`` when ``F`` is less than the number of folds."""
    folds = int(n_train_folds) + int(n_valid_folds) + int(n_test_folds)
    if min(int(n_train_folds), int(n_valid_folds), int(n_test_folds)) < 1:
        raise ValueError("every part of a split needs at least one fold")
    if F < folds:
        raise ValueError("%d bin(s) cannot be split into %d folds: cross-validation holds out frequency bins, so it needs "
                         "spectrograms; for amplitude traces use anchor_point_warp_parameter_search" % (F, folds))
    parts = np.array_split(rng.permutation(F), folds)
    a, b = int(n_train_folds), int(n_train_folds) + int(n_valid_folds)
    return tuple(np.sort(np.concatenate(parts[i:j])) for i, j in ((0, a), (a, b), (b, folds)))


def search_plan(F, search_params={}, seed=42):
    """Everything random about ``cross_validate``, from one ``RandomState(seed)``: first the settings
    (``sample_settings``), then for every sample in order its ``n_valid_samples`` splits (``split_bins``).  Returns
    ``(knots, shift_scale, slope_scale, schedules, splits)`` with ``splits[s][v] = (train, valid, test)``."""
    p = {**DEFAULT_SEARCH_PARAMS, **search_params}
    if F < int(p['n_train_folds']) + int(p['n_valid_folds']) + int(p['n_test_folds']):
        split_bins(F, p['n_train_folds'], p['n_valid_folds'], p['n_test_folds'], None)    # raises
    rng = np.random.RandomState(seed)
    knots, a, b, schedules = sample_settings(p, rng)
    splits = [[split_bins(F, p['n_train_folds'], p['n_valid_folds'], p['n_test_folds'], rng)
               for _ in range(int(p['n_valid_samples']))] for _ in range(len(knots))]
    return knots, a, b, schedules, splits


def score_candidates(wp):
    """the fitted warps of one group as candidates ``[rows, 1, W]`` of the loss kernels: the knots when the fit has
    them, otherwise ``(shift, log(slope))``"""
    if 'knots' in wp:
        return np.asarray(wp['knots'], dtype=np.float64)[:, None, :]
    return np.stack([np.asarray(wp['shifts'], np.float64), np.log(np.asarray(wp['slopes'], np.float64))], axis=1)[:, None, :]


def _score(specs, fits, bin_sets):
    """``R²`` of every fit on every one of its bin sets.  ``fits``: one ``warp_params`` dict (host arrays over all rows)
    per fit, all of one form; ``bin_sets[i]``: the bin lists fit ``i`` is scored on.  One plan whose groups are the
    (fit, bin set) pairs over all rows: the template under the fitted warps, ``SS_res`` from the grouped loss at the fitted
    parameters with both λ = 0, the raw template, its mean over columns and ``SS_tot`` from the raw grouped loss.  The
    per-row sums are added on the host, row 0 first.  Returns ``[len(fits)][len(bin_sets[i])]`` floats."""
    dev = specs.device
    N, _, T = specs.shape
    groups = [(np.arange(N, dtype=np.int32), np.asarray(b, dtype=np.int32)) for bs in bin_sets for b in bs]
    owner = [i for i, bs in enumerate(bin_sets) for _ in bs]
    plan = warp_fit.GroupPlan(specs, groups)
    cand = torch.from_numpy(np.ascontiguousarray(np.concatenate([score_candidates(fits[i]) for i in owner]))).to(dev)
    zero = torch.zeros(plan.G, dtype=torch.float64, device=dev)
    res = torch.empty((plan.V, 1), dtype=torch.float64, device=dev)
    if 'knots' in fits[0]:
        knots = torch.from_numpy(np.ascontiguousarray(np.concatenate([fits[i]['knots'] for i in owner]))).to(dev)
        plan.mean(knots=knots)
        plan.pl_loss(cand, zero, zero, False, res)
    else:
        params = np.concatenate([np.stack([fits[i]['shifts'], fits[i]['slopes']], axis=1) for i in owner])
        plan.mean(params=torch.from_numpy(np.ascontiguousarray(params)).to(dev))
        plan.ss_loss(cand, zero, zero, False, res)
    res = res.cpu().numpy()[:, 0]
    raw = plan.mean(out=torch.empty_like(plan.targets)).cpu().numpy()
    flat = np.empty_like(raw)
    for g in range(plan.G):                                  # the bin's mean over rows and columns, held along the row
        a, b = int(plan.bin_off[g]) * T, int(plan.bin_off[g + 1]) * T
        flat[a:b] = np.repeat(raw[a:b].reshape(-1, T).mean(axis=1), T)
    tot = plan.raw_loss(torch.empty(plan.V, dtype=torch.float64, device=dev), torch.from_numpy(flat).to(dev)).cpu().numpy()
    out, g = [], 0
    for bs in bin_sets:
        out.append([])
        for _ in bs:
            a, b = int(plan.row_off[g]), int(plan.row_off[g + 1])
            out[-1].append(1.0 - res[a:b].sum() / tot[a:b].sum())
            g += 1
    return out


def cross_validate(specs, search_params={}, seed=42, max_rows=None):
    """The cross-validated search over ``specs`` ``[N, F, T]`` (numpy or a device tensor, float32 or float64).  Reads the
    keys ``samples_per_knot``, ``n_valid_samples``, ``n_train_folds``, ``n_valid_folds``, ``n_test_folds``,
    ``knot_range``, ``shift_range``, ``slope_range``, ``shift_lambdas`` and ``slope_lambdas`` of
    ``{**DEFAULT_SEARCH_PARAMS, **search_params}``.  For every sampled setting and every one of its ``n_valid_samples``
    bin splits (``search_plan``) all motifs are fitted on the train bins, and the fitted warps are scored on the train,
    validation and test bins (module docstring).  Returns a dict: ``'knots'`` [S] int, ``'shift_scale'`` [S],
    ``'slope_scale'`` [S], ``'train_rsq'`` and ``'valid_rsq'`` [S, n_valid_samples], ``'test_rsq'`` [S] (the mean over
    the splits) and ``'schedules'``, a list of S ``(shift_λs, slope_λs)``.  The same seed gives the same dict.
    ``ValueError`` when ``F`` is less than the number of folds, as for amplitude traces.  ``max_rows`` is
    ``align_specs_grouped``'s."""
    specs, _ = warp_fit._specs_tensor(specs)
    N, F, T = specs.shape
    knots, a, b, schedules, splits = search_plan(F, search_params, seed)
    S, n_splits = len(knots), len(splits[0])
    rsq = np.zeros((3, S, n_splits))
    for k in sorted(set(knots.tolist())):
        n_knots = max(k, 0)
        if n_knots != 0:
            warp_fit._check_knots(T, n_knots + 2)
        idx = [s for s in range(S) if knots[s] == k]
        groups = [(None, splits[s][v][0]) for s in idx for v in range(n_splits)]
        shift = np.array([schedules[s][0] for s in idx for _ in range(n_splits)]).T
        slope = np.array([schedules[s][1] for s in idx for _ in range(n_splits)]).T
        fits = warp_fit.align_specs_grouped(specs, groups, shift, slope, n_knots=n_knots, max_rows=max_rows)
        fits = [{key: val.cpu().numpy() for key, val in wp.items()} for wp in fits]
        scores = _score(specs, fits, [splits[s][v] for s in idx for v in range(n_splits)])
        for i, (s, v) in enumerate((s, v) for s in idx for v in range(n_splits)):
            rsq[:, s, v] = scores[i]
    return {'knots': knots, 'shift_scale': a, 'slope_scale': b, 'train_rsq': rsq[0], 'valid_rsq': rsq[1],
            'test_rsq': rsq[2].mean(axis=1), 'schedules': schedules}


def best_warp_params(res):
    """The ``warp_params`` of the sample of ``cross_validate``'s result with the best median ``valid_rsq`` (the first
    of equals): ``{'n_knots', 'shift_lambdas', 'slope_lambdas'}``, ready for ``get_warped_window_data_loaders(...,
    warp_params=..., fit='device')``.  A shift-only sample has ``n_knots`` 0 and its all-``inf`` slope schedule."""
    best = int(np.argmax(np.median(np.asarray(res['valid_rsq'], dtype=np.float64), axis=1)))
    shift_λs, slope_λs = res['schedules'][best]
    return {'n_knots': max(int(res['knots'][best]), 0), 'shift_lambdas': list(shift_λs), 'slope_lambdas': list(slope_λs)}


def _read_files(audio_dirs, spec_params):
    """the wav files of the directories, in order, as ``get_specs_and_amplitude_traces`` returns them"""
    from scipy.io import wavfile
    from scipy.io.wavfile import WavFileWarning
    from . import warped_window as ww
    fns = [fn for d in audio_dirs for fn in ww._get_wavs_from_dir(d)]
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", category=WavFileWarning)
        audio = [wavfile.read(fn)[1] for fn in fns]
        fs = wavfile.read(fns[0])[0]
    return ww.get_specs_and_amplitude_traces(audio, fs, spec_params)


def _fit_layout(specs, amps, warp_type):
    """the search input as ``[files, bins, frames]``, the layout of ``warp_fit``"""
    to_warp = amps if warp_type == 'amplitude' else specs
    return np.ascontiguousarray(to_warp.transpose(0, 2, 1))


def cross_validation_warp_parameter_search(audio_dirs, spec_params, search_params={}, warp_type='spectrogram',
                                           verbose=True, make_plot=True, img_fn='temp.pdf'):
    """``cross_validation_warp_parameter_search`` (models/utils.py:48-132) around ``cross_validate``: the wav files of
    ``audio_dirs`` (all of one duration) become spectrograms and amplitude traces under ``spec_params``, the search
    runs on the kind ``warp_type`` names, and with ``make_plot`` the median train and validation scores and the test
    score of every sample are drawn against its knot count into ``img_fn``.  Returns ``cross_validate``'s dict.
    ``warp_type='amplitude'`` raises ``ValueError``: one bin cannot be split (use the anchor search)."""
    assert type(spec_params) == type({})
    assert warp_type in ['amplitude', 'spectrogram']
    search_params = {**DEFAULT_SEARCH_PARAMS, **search_params}
    if verbose:
        print("Collecting spectrograms...")
    specs, amps, _ = _read_files(audio_dirs, spec_params)
    if verbose:
        print("\tDone.")
        print("Running parameter search...")
    res = cross_validate(_fit_layout(specs, amps, warp_type), search_params)
    if verbose:
        print("\tDone.")
    if make_plot:
        import matplotlib.pyplot as plt
        plt.switch_backend('agg')
        knots = res['knots']
        plt.scatter(knots - 0.1, np.median(res['train_rsq'], axis=1), c='k', label='train', alpha=0.5)
        plt.scatter(knots, np.median(res['valid_rsq'], axis=1), c='b', label='validation', alpha=0.7)
        plt.scatter(knots + 0.1, res['test_rsq'], c='r', label='test', alpha=0.7)
        plt.ylabel("$R^2$")
        plt.xlabel("n_knots")
        plt.legend(loc='best')
        for side in ('top', 'right'):
            plt.gca().spines[side].set_visible(False)
        plt.savefig(img_fn)
        plt.close('all')
    return res


def anchor_errors(x_knots, y_knots, anchor_times, template_dur):
    """The anchor score of models/utils.py:294-306 for fitted knots: every file's anchor times (seconds,
    ``[files, anchors]``) are mapped from measured to template time through its knots (``interp1d`` of ``y_knots[i]``
    over ``x_knots[i]``, in quantiles of ``template_dur``, extrapolated beyond the outer knots); the score is the mean
    absolute deviation of the mapped times from their mean over files, corrected for the change of timescale by
    ``std(anchor_times) / std(mapped times)``, in milliseconds."""
    from scipy.interpolate import interp1d
    anchor_times = np.asarray(anchor_times, dtype=np.float64)
    mapped = np.zeros_like(anchor_times)
    for i in range(len(anchor_times)):
        to_template = interp1d(x_knots[i], y_knots[i], bounds_error=False, fill_value='extrapolate', assume_sorted=True)
        mapped[i] = to_template(anchor_times[i] / template_dur)
    mapped *= template_dur
    mae = np.mean(np.abs(np.mean(mapped, axis=0, keepdims=True) - mapped))
    return mae * 1e3 * np.std(anchor_times) / np.std(mapped)


def _get_txts_from_dir(d):
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if len(f) > 4 and f[-4:] == '.txt']


def anchor_point_warp_parameter_search(audio_dirs, anchor_dir, spec_params, search_params, num_iter=20, gridpoints=6,
                                       warp_type='amplitude', aw_iterations=25, aw_warp_iterations=100, verbose=True,
                                       make_plot=True, img_fn='temp.pdf'):
    """``anchor_point_warp_parameter_search`` (models/utils.py:135-276): ``num_iter`` settings are drawn with
    ``np.random.choice`` call for call as the reference draws them -- a knot count of ``arange(*knot_range)``, a
    ``shift_scale`` and a ``slope_scale`` of two ``geomspace`` grids of ``gridpoints`` points over ``shift_range`` and
    ``slope_range`` -- every setting is fitted to all files (those of ``audio_dirs``, then the annotated ones of
    ``anchor_dir``) on all bins, one ``align_specs_grouped`` call per distinct knot count, and scored by
    ``anchor_errors`` on the annotated files, which are the last rows of the fit.  (The reference reads the first
    rows' knots there, which are the annotated files' only when ``audio_dirs`` is empty.)  The annotation of
    ``name.wav`` is ``name.txt``: one row per anchor, the anchor time in the first of two columns.
    ``aw_iterations`` and ``aw_warp_iterations`` are accepted and not used.  Returns ``(param_history [num_iter, 3]
    int, loss_history [num_iter], support)``; ``param_history`` indexes ``support``."""
    assert type(spec_params) == type({})
    assert warp_type in ['amplitude', 'spectrogram']
    anchor_times = np.array([np.loadtxt(fn).reshape(-1, 2)[:, 0] for fn in _get_txts_from_dir(anchor_dir)])
    null_warp_mae = 1e3 * np.mean(np.abs(np.mean(anchor_times, axis=0, keepdims=True) - anchor_times))
    if verbose:
        print("Null warp MAE:", '{0:.3f}'.format(null_warp_mae), 'ms')
    for i in range(1, len(anchor_times)):
        assert len(anchor_times[0]) == len(anchor_times[i]), 'Unequal numbers of anchor times!'
    if verbose:
        print("Collecting spectrograms...")
    specs, amps, template_dur = _read_files(list(audio_dirs) + [anchor_dir], spec_params)     # annotated audio at the end
    to_warp = _fit_layout(specs, amps, warp_type)
    if verbose:
        print("\tDone.")
        print("Evaluating parameters...")
    search_params = {**DEFAULT_SEARCH_PARAMS, **search_params}
    knot_range = search_params['knot_range']
    support = [
        np.arange(*knot_range),
        np.geomspace(*search_params['shift_range'], num=gridpoints),
        np.geomspace(*search_params['slope_range'], num=gridpoints),
    ]
    param_ranges = [np.arange(knot_range[1] - knot_range[0]), np.arange(gridpoints), np.arange(gridpoints)]
    param_history = np.zeros((num_iter, len(PARAM_NAMES)), dtype='int')
    loss_history = np.zeros(num_iter)
    for i in range(num_iter):
        for j in range(len(PARAM_NAMES)):
            param_history[i, j] = np.random.choice(param_ranges[j])
    base_shift, base_slope = warp_fit.check_schedule(search_params['shift_lambdas'], search_params['slope_lambdas'])
    T, n_anchor = to_warp.shape[2], len(anchor_times)
    for k in sorted(set(support[0][param_history[:, 0]].tolist())):
        idx = [i for i in range(num_iter) if support[0][param_history[i, 0]] == k]
        schedules = [_schedule(k, support[1][param_history[i, 1]], support[2][param_history[i, 2]], base_shift, base_slope)
                     for i in idx]
        fits = warp_fit.align_specs_grouped(to_warp, [(None, None)] * len(idx), np.array([s[0] for s in schedules]).T,
                                            np.array([s[1] for s in schedules]).T, n_knots=max(int(k), 0))
        for i, wp in zip(idx, fits):
            x_knots, y_knots = warp_fit.knots_from_warp_params(wp, T)
            loss_history[i] = anchor_errors(x_knots[-n_anchor:], y_knots[-n_anchor:], anchor_times, template_dur)
    if verbose:
        for i in range(num_iter):
            print('\t' + str(param_history[i]), '{0:.3f}'.format(loss_history[i]), 'ms')
    if make_plot:
        import matplotlib.pyplot as plt
        plt.switch_backend('agg')
        _, axarr = plt.subplots(nrows=3)
        for i, (ax, key) in enumerate(zip(axarr, PARAM_NAMES)):
            x_vals = param_history[:, i] - 0.1 + 0.2 * np.random.rand(num_iter)
            ax.axhline(y=null_warp_mae, c='k', ls='--', alpha=0.5, lw=0.8)
            ax.scatter(x_vals, loss_history, c='k', alpha=0.5)
            ax.set_xlabel(key)
            ax.set_ylabel('MAE (ms)')
            for side in ('top', 'right'):
                ax.spines[side].set_visible(False)
            plt.sca(ax)
            plt.xticks(param_ranges[i], ['{0:.5f}'.format(j) for j in support[i]])
        plt.tight_layout()
        plt.savefig(img_fn)
        plt.close('all')
    return param_history, loss_history, support


def install(module):
    """Point ``cross_validation_warp_parameter_search`` and ``anchor_point_warp_parameter_search`` of ``module`` here.
    The module object is passed in: importing the reference's ``ava.models.utils`` needs affinewarp."""
    module.cross_validation_warp_parameter_search = cross_validation_warp_parameter_search
    module.anchor_point_warp_parameter_search = anchor_point_warp_parameter_search
    return module
