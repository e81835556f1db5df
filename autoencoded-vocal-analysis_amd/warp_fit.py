"""The time-warp fit on the device: shift and slope, piecewise linear (row f14).

Mirror of the reference's own replacement for affinewarp, ``ava/preprocessing/warping.py``:

  ``apply_warp``              warping.py:25-50
  ``align_specs``             warping.py:53-145    alternate a mean template with a per-spectrogram minimisation
  ``minimize_warp``           warping.py:121-131   the ``scipy.optimize.minimize(method='Powell')`` of every motif, batched
  ``warp_loss``               warping.py:148-163   both objectives, for a batch of candidates per motif
  ``knots_from_warp_params``  the fitted warps as the knots of ``DeviceWarpedWindowDataset``
  ``pl_warp_loss``, ``pl_minimize_warp``, ``align_specs(..., n_knots=)``   the piecewise-linear warp, no reference code
  ``align_specs_grouped``     many such fits over the same spectrograms in one launch sequence (row f17), for ``warp_search``
  ``install``                 points the reference module's two public functions here

Every number is made by the kernels of ``csrc/warp_fit.hip`` in fp64; there is no CPU fallback.  The functions take
numpy arrays or device tensors ``[N, F, T]`` of float32 or float64 and answer in kind (numpy in, numpy out) and in the
input's dtype: like the reference, ``align_specs`` keeps the warped spectrograms in the input's dtype and takes the next
iteration's mean template from those stored values.  ``T`` is at most ``ava_warpfit_max_t()`` = 512
(``NotImplementedError``); N and F are unbounded.

The search.  Powell is replaced by a deterministic derivative-free search made of batched loss evaluations.  Every round
evaluates, for all motifs in one launch, a grid of candidates centred on the motif's current best: ``2 GRID_KS + 1 = 7``
shifts in steps of ``hs`` times ``2 GRID_KL + 1 = 5`` log slopes in steps of ``hl``; with ``slope_λ = inf`` the grid is a
line of ``2 LINE_KS + 1 = 15`` shifts.  A slope step pivots the warp about the middle column (the shift moves along with
it), which keeps the two grid axes nearly independent directions of the objective.  The best candidate becomes the
next centre -- the centre is candidate 0 and wins ties, so the loss never rises -- and both steps halve.  The first
round spans ``shift ± T * SHIFT_SPAN`` (``T / 8`` columns) and ``log slope ± LOG_SLOPE_SPAN`` (0.25, slopes from 0.78
to 1.28) about ``x0``; the search ends when both steps are below ``XTOL = 1e-4``, the ``xtol`` Powell is called with
(16 rounds at T = 128).  Why the shift axis is the wide one: under linear interpolation the objective is piecewise
quadratic in the shift, with a kink wherever a position crosses a column -- at slope 1 all columns cross together, at
every whole shift -- so neighbouring cells can each hold a local minimum.  A grid that keeps only one cell on either
side of its best point when it halves (5 points) was seen to settle in the cell next to the one Powell found, 1.2e-4
above it in loss; 15 points keep 3.5 cells on either side, 7 points 1.5.  The number of rounds depends on ``T`` alone,
so nothing is read back: one ``align_specs`` iteration is enqueued without a host synchronisation.  The search always
returns a result: the reference's ``(None, None)`` on an optimiser failure has no counterpart here.

The piecewise-linear warp (``n_knots > 0``; what the reference's ``WarpedWindowDataset`` asks affinewarp for, which is no
dependency here).  A motif has ``K = n_knots + 2`` knots ``u[k]``: the source position, in time bins, that the template
column ``t_k = k (T - 1) / (K - 1)`` maps to.  Column ``j`` lies in segment ``k = min(j (K - 1) // (T - 1), K - 2)`` and
reads the source at ``p(j) = u_k + s_k (j - t_k)`` with ``s_k = (u_{k+1} - u_k) / (t_{k+1} - t_k)``; the objective is
``sum((interp(spec)(p) - target) ** 2) + shift_λ u_0 ** 2 + slope_λ mean_k(log(s_k) ** 2)``, ``+inf`` when some
``s_k <= 0``.  With ``K = 2`` that is the objective above at ``shift = u_0``, ``slope = s_0``.  ``K`` is at most
``ava_warpfit_max_knots()`` = 16 and ``T - 1 >= 2 (K - 1)`` (``ValueError``).  An iteration of ``align_specs`` searches in
two stages.  Stage A is the search above for (shift, log slope), carried from iteration to iteration as before; its result
gives the starting knots ``u_k = shift + slope t_k``: the knots of the iteration before are not kept, only the template
made from them is.  Stage B (``pl_minimize_warp``) is a coordinate search: rounds with
the knot step ``h`` halving from ``T * SHIFT_SPAN / (KNOT_KS (K - 1))`` until it is below ``XTOL``, every round sweeping
the knots ``k = 0 .. K - 1`` in order, every knot trying ``u_k + o h`` for ``o = 0, -1, +1, ... ± KNOT_KS`` in one
candidates, one loss and one argmin launch.  The first round reaches ``SHIFT_SPAN`` of a segment's length on either side
of a knot.  Candidate 0 is the centre and wins ties, and crossed knots lose to any finite loss, so a motif's loss never
rises and its knots stay in order.  An iteration with ``slope_λ = inf`` has no stage B: ``u_k = shift + t_k``.  The number of
launches depends on ``T`` and ``K`` alone: nothing is read back here either.
"""
import warnings

import numpy as np
import torch

from . import _lib

__all__ = ["WARNING_MSG", "XTOL", "GRID_KS", "GRID_KL", "LINE_KS", "SHIFT_SPAN", "LOG_SLOPE_SPAN", "DEFAULT_SHIFT_LAMBDAS",
           "DEFAULT_SLOPE_LAMBDAS", "KNOT_KS", "apply_warp", "align_specs", "minimize_warp", "warp_loss", "search_rounds",
           "check_schedule", "knots_from_warp_params", "install", "knot_columns", "knot_rounds", "pl_warp_loss",
           "pl_minimize_warp", "align_specs_grouped", "check_groups", "check_group_schedule", "GroupPlan"]

WARNING_MSG = "ava.preprocessing.warping is experimental and may change in " + \
    "a future version of AVA!"                 # warping.py:20-21

XTOL = 1e-4                # scipy's default xtol of method='Powell' (warping.py:130 passes no options)
GRID_KS, GRID_KL = 3, 2    # grid points on either side of the centre: shifts, log slopes
LINE_KS = 7                # the same for the line of shifts searched when slope_λ = inf
SHIFT_SPAN = 0.125         # half-span of the first round's shifts, as a fraction of T
LOG_SLOPE_SPAN = 0.25      # half-span of the first round's log slopes
KNOT_KS = 3                # candidates on either side of a knot in the piecewise-linear coordinate search

# the schedule fit='device' of DeviceWarpedWindowDataset uses when warp_params names none: shift-only first, then
# decreasing penalties down to the maximum-likelihood fit (the advice of the reference's docstring, warping.py:67-72)
DEFAULT_SHIFT_LAMBDAS = (1e-2, 1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 0.0, 0.0)
DEFAULT_SLOPE_LAMBDAS = (np.inf, np.inf, np.inf, 1e2, 1e1, 1.0, 0.0, 0.0)

_DTYPES = {torch.float32: 0, torch.float64: 1}


def _specs_tensor(specs):
    """``(contiguous device tensor [N, F, T], came as numpy)``"""
    is_numpy = not torch.is_tensor(specs)
    if is_numpy:
        specs = np.asarray(specs)
        if specs.dtype not in (np.float32, np.float64):
            raise TypeError("spectrograms must be float32 or float64, got %s" % specs.dtype)
        specs = torch.from_numpy(np.ascontiguousarray(specs)).to("cuda")
    elif specs.dtype not in _DTYPES:
        raise TypeError("spectrograms must be float32 or float64, got %s" % specs.dtype)
    if specs.dim() != 3 or specs.shape[0] < 1 or specs.shape[1] < 1:
        raise ValueError("expected spectrograms of shape [n_specs, freq_bins, time_bins]")
    T = specs.shape[2]
    if T < 2:
        raise ValueError("a warp needs at least two time bins")
    if T > _lib.load().ava_warpfit_max_t():
        raise NotImplementedError("at most %d time bins per spectrogram" % _lib.load().ava_warpfit_max_t())
    return specs.contiguous(), is_numpy


def _f64(a, dev, shape):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    t = t.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(t.shape)))
    return t


def _entry(stem, pl, *args):
    """Call the entry point ``ava_warpfit_<stem>``, the ``%s`` of ``stem`` standing for ``pl_`` with knots (``pl``) and for
    nothing with shift and slope; a failure names the entry point that was called.  ``pl`` is always said by the caller,
    never read off a tensor's last dimension: two knots and (shift, log slope) are both two wide."""
    name = "ava_warpfit_" + stem % ("pl_" if pl else "")
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _apply(specs, params, pl):
    """``specs`` [N, F, T] under ``params`` [N, 2] = (shift, slope) or, with ``pl``, under knots [N, K]; device tensors;
    enqueued, nothing synchronises"""
    N, F, T = specs.shape
    out = torch.empty_like(specs)
    k = (params.shape[1],) if pl else ()
    _entry("%sapply", pl, specs.data_ptr(), _DTYPES[specs.dtype], N, F, T, params.data_ptr(), *k, out.data_ptr(), _lib.stream())
    return out


def knot_columns(T, K):
    """the template columns ``t_k = k (T - 1) / (K - 1)`` of ``K`` knots: ``[K]`` float64"""
    return np.arange(K) * (T - 1) / (K - 1)


def _check_knots(T, K):
    """``ValueError`` unless ``K`` knots fit ``T`` time bins; raised before any launch"""
    cap = _lib.load().ava_warpfit_max_knots()
    if K < 2 or K > cap:
        raise ValueError("a warp has 2 to %d knots (n_knots = 0 to %d), got %d" % (cap, cap - 2, K))
    if T - 1 < 2 * (K - 1):
        raise ValueError("%d knots need at least %d time bins, got %d" % (K, 2 * (K - 1) + 1, T))


def _knots_tensor(knots, dev, N, T):
    t = knots if torch.is_tensor(knots) else torch.from_numpy(np.ascontiguousarray(np.asarray(knots, dtype=np.float64)))
    if t.dim() != 2 or t.shape[0] != N:
        raise ValueError("expected knots of shape [n_specs, n_knots + 2], got %s" % (tuple(t.shape),))
    _check_knots(T, t.shape[1])
    return t.to(device=dev, dtype=torch.float64).contiguous()


def apply_warp(specs, warp_params):
    """``apply_warp`` (warping.py:25-50): ``warped[n, f, j] = interp1d(specs[n, f])(shifts[n] + slopes[n] * j)`` with the
    end columns held outside the spectrogram.  ``warp_params`` maps ``'shifts'`` and ``'slopes'`` to ``[n_specs]``
    arrays or tensors.  With a key ``'knots'`` (``[n_specs, K]``, what ``align_specs(..., n_knots=K - 2)`` returns) the
    positions are the piecewise-linear ``p(j)`` of the module docstring instead, and the other two keys are not read.
    Same shape, dtype and kind (numpy array or device tensor) as ``specs``."""
    specs, is_numpy = _specs_tensor(specs)
    N = specs.shape[0]
    if 'knots' in warp_params:
        out = _apply(specs, _knots_tensor(warp_params['knots'], specs.device, N, specs.shape[2]), True)
        return out.cpu().numpy() if is_numpy else out
    params = torch.stack([_f64(warp_params['shifts'], specs.device, (N,)),
                          _f64(warp_params['slopes'], specs.device, (N,))], dim=1).contiguous()
    out = _apply(specs, params, False)
    return out.cpu().numpy() if is_numpy else out


class _Problem:
    """One plain fit problem as the searches see it: ``specs`` [N, F, T] against one ``target`` [F, T] (device tensors),
    with what a ``GroupPlan`` offers them: the row count ``V``, ``T`` and ``loss``.  Its λ are host floats."""

    def __init__(self, specs, target):
        self.specs, self.target = specs, target
        self.V, self.T = specs.shape[0], specs.shape[2]

    def loss(self, pl, cand, shift_λ, slope_λ, fixed, loss):
        """``ava_warpfit_loss`` of ``cand`` [N, C, 2] or, with ``pl``, ``ava_warpfit_pl_loss`` of ``cand`` [N, C, K] into
        ``loss`` [N, C]; the entry points read ``fixed`` off ``slope_λ = inf`` themselves"""
        N, F, T = self.specs.shape
        k = (cand.shape[2],) if pl else ()
        _entry("%sloss", pl, self.specs.data_ptr(), _DTYPES[self.specs.dtype], N, F, T, self.target.data_ptr(), cand.data_ptr(),
               cand.shape[1], *k, shift_λ, slope_λ, loss.data_ptr(), _lib.stream())
        return loss


def _warp_loss(specs, target, candidates, shift_λ, slope_λ, pl):
    specs, is_numpy = _specs_tensor(specs)
    N, F, T = specs.shape
    target = _f64(target, specs.device, (F, T))
    cand = candidates if torch.is_tensor(candidates) else torch.from_numpy(np.asarray(candidates, dtype=np.float64))
    if cand.dim() != 3 or cand.shape[0] != N or cand.shape[1] < 1 or (not pl and cand.shape[2] != 2):
        raise ValueError("expected candidates of shape [n_specs, n_candidates, %s]" % ("n_knots + 2" if pl else "2"))
    if pl:
        _check_knots(T, cand.shape[2])
    cand = cand.to(device=specs.device, dtype=torch.float64).contiguous()
    shift_λ, slope_λ = _check_lambdas(shift_λ, slope_λ)
    loss = torch.empty((N, cand.shape[1]), dtype=torch.float64, device=specs.device)
    _Problem(specs, target).loss(pl, cand, shift_λ, slope_λ, slope_λ == np.inf, loss)
    return loss.cpu().numpy() if is_numpy else loss


def warp_loss(specs, target, candidates, shift_λ, slope_λ):
    """The objectives of warping.py:148-163 for a batch of candidates: ``loss[n, c] = sum((interp(specs[n])(shift +
    exp(log_slope) * arange(T)) - target) ** 2) + shift_λ * shift ** 2 + slope_λ * log_slope ** 2`` for ``candidates``
    ``[N, C, 2]`` = (shift, log_slope).  With ``slope_λ = inf`` the slope is 1 and the slope term is dropped
    (``_get_shift_objective``).  Sums run in a fixed order: two calls give the same bits.  Returns ``[N, C]`` float64
    (numpy for numpy ``specs``)."""
    return _warp_loss(specs, target, candidates, shift_λ, slope_λ, False)


def pl_warp_loss(specs, target, candidates, shift_λ, slope_λ):
    """The piecewise-linear objective of the module docstring for ``candidates`` ``[N, C, K]``, ``K`` knots each:
    ``[N, C]`` float64, ``+inf`` where knots cross.  With ``slope_λ = inf`` every slope is 1 (``p(j) = u_0 + j``), the
    slope term is dropped and crossed knots go unnoticed.  Same sums, in the same order, as ``warp_loss``."""
    return _warp_loss(specs, target, candidates, shift_λ, slope_λ, True)


def _check_lambdas(shift_λ, slope_λ):
    shift_λ, slope_λ = float(shift_λ), float(slope_λ)
    if not np.isfinite(shift_λ) or shift_λ < 0:
        raise ValueError("shift_λ must be finite and not negative (only slope_λ may be inf), got %r" % shift_λ)
    if np.isnan(slope_λ) or slope_λ < 0:
        raise ValueError("slope_λ must be inf or not negative, got %r" % slope_λ)
    return shift_λ, slope_λ


def check_schedule(shift_λs, slope_λs):
    """The two λ sequences of ``align_specs`` as lists of floats: equally long, not empty, every ``shift_λ`` finite and
    not negative, every ``slope_λ`` not negative or ``inf`` (a shift-only iteration).  ``ValueError`` otherwise."""
    shift_λs, slope_λs = list(shift_λs), list(slope_λs)
    if len(shift_λs) != len(slope_λs):
        raise ValueError("shift_λs and slope_λs must have one entry per iteration each: %d and %d entries"
                         % (len(shift_λs), len(slope_λs)))
    if len(shift_λs) == 0:
        raise ValueError("an empty schedule fits nothing")
    pairs = [_check_lambdas(a, b) for a, b in zip(shift_λs, slope_λs)]
    return [a for a, _ in pairs], [b for _, b in pairs]


def search_rounds(T, fixed_slope):
    """``(ks, kl, [(hs, hl), ...])``: the grid half-widths and the grid steps of every round of ``minimize_warp`` for
    ``T`` time bins.  The steps halve each round from ``T * SHIFT_SPAN / ks`` and ``LOG_SLOPE_SPAN / kl`` until both
    (with ``fixed_slope``: the shift step) are below ``XTOL``."""
    ks, kl = (LINE_KS, 0) if fixed_slope else (GRID_KS, GRID_KL)
    hs, hl = T * SHIFT_SPAN / ks, LOG_SLOPE_SPAN / max(kl, 1)
    rounds = []
    while hs >= XTOL or (not fixed_slope and hl >= XTOL):
        rounds.append((hs, hl))
        hs, hl = hs / 2, hl / 2
    return ks, kl, rounds


def _minimize(prob, x, shift_λ, slope_λ, fixed, best_loss):
    """the search of ``minimize_warp`` over the rows of ``prob``, a ``_Problem`` (λ: floats) or a ``GroupPlan`` (λ: device
    [G]); ``x`` [V, 2] and ``best_loss`` [V] are updated in place"""
    V, T = prob.V, prob.T
    ks, kl, rounds = search_rounds(T, fixed)
    C = (2 * ks + 1) * (2 * kl + 1)
    dev, st = x.device, _lib.stream()
    cand = torch.empty((V, C, 2), dtype=torch.float64, device=dev)
    loss = torch.empty((V, C), dtype=torch.float64, device=dev)
    best = torch.empty(V, dtype=torch.int32, device=dev)
    for hs, hl in rounds:
        _entry("%scandidates", False, x.data_ptr(), V, T, ks, kl, hs, hl, cand.data_ptr(), st)
        prob.loss(False, cand, shift_λ, slope_λ, fixed, loss)
        _entry("%sargmin", False, loss.data_ptr(), cand.data_ptr(), V, C, best.data_ptr(), x.data_ptr(), best_loss.data_ptr(), st)


def minimize_warp(specs, target, x0, shift_λ, slope_λ):
    """The per-motif minimisation ``align_specs`` calls (warping.py:121-131), for all motifs at once: ``(x [N, 2],
    loss [N])`` with ``x`` = (shift, log_slope) minimising ``warp_loss(specs, target, ., shift_λ, slope_λ)`` from
    ``x0`` [N, 2], by the grid search of the module docstring (first round ``shift ± T / 8``, ``log slope ± 0.25``
    about ``x0``, halving to ``XTOL = 1e-4``).  With ``slope_λ = inf`` only the shift is searched and ``x[:, 1]`` is
    ``x0[:, 1]`` (the objective ignores it).  The loss returned is never above the loss at ``x0``.  Unlike Powell the
    search cannot fail: it always returns a result."""
    specs, is_numpy = _specs_tensor(specs)
    N, F, T = specs.shape
    target = _f64(target, specs.device, (F, T))
    x = _f64(x0, specs.device, (N, 2)).clone()
    shift_λ, slope_λ = _check_lambdas(shift_λ, slope_λ)
    best_loss = torch.empty(N, dtype=torch.float64, device=specs.device)
    _minimize(_Problem(specs, target), x, shift_λ, slope_λ, slope_λ == np.inf, best_loss)
    return (x.cpu().numpy(), best_loss.cpu().numpy()) if is_numpy else (x, best_loss)


def knot_rounds(T, K):
    """the knot steps of every round of ``pl_minimize_warp`` for ``T`` time bins and ``K`` knots: halving from
    ``T * SHIFT_SPAN / (KNOT_KS (K - 1))`` until below ``XTOL``"""
    h, rounds = T * SHIFT_SPAN / (KNOT_KS * (K - 1)), []
    while h >= XTOL:
        rounds.append(h)
        h = h / 2
    return rounds


def _minimize_pl(prob, u, shift_λ, slope_λ, fixed, best_loss):
    """stage B over the rows of ``prob`` (as in ``_minimize``); ``u`` [V, K] and ``best_loss`` [V] are updated in place.
    ``fixed``: a line search of one shift common to all knots, after which ``u_k = u_0 + t_k``."""
    V, T, K = prob.V, prob.T, u.shape[1]
    ks = LINE_KS if fixed else KNOT_KS
    steps = [(-1, hs) for hs, _ in search_rounds(T, True)[2]] if fixed else \
        [(k, h) for h in knot_rounds(T, K) for k in range(K)]
    C = 2 * ks + 1
    dev, st = u.device, _lib.stream()
    cand = torch.empty((V, C, K), dtype=torch.float64, device=dev)
    loss = torch.empty((V, C), dtype=torch.float64, device=dev)
    best = torch.empty(V, dtype=torch.int32, device=dev)
    for axis, h in steps:
        _entry("%scandidates", True, u.data_ptr(), V, K, axis, ks, h, cand.data_ptr(), st)
        prob.loss(True, cand, shift_λ, slope_λ, fixed, loss)
        _entry("%sargmin", True, loss.data_ptr(), cand.data_ptr(), V, C, K, best.data_ptr(), u.data_ptr(), best_loss.data_ptr(), st)
    if fixed:
        u.copy_(u[:, :1] + torch.from_numpy(knot_columns(T, K)).to(dev))


def pl_minimize_warp(specs, target, u0, shift_λ, slope_λ):
    """Stage B of the module docstring for all motifs at once: ``(u [N, K], loss [N])`` from the knots ``u0`` [N, K]
    by the coordinate search over single knots.  The loss returned is never above ``pl_warp_loss`` at ``u0``, and
    knots that start in order stay in order.  With ``slope_λ = inf`` one shift common to all knots is searched
    instead (a line of ``2 LINE_KS + 1`` shifts, as ``minimize_warp`` does) and ``u_k = u_0 + t_k`` is returned."""
    specs, is_numpy = _specs_tensor(specs)
    N, F, T = specs.shape
    target = _f64(target, specs.device, (F, T))
    u = _knots_tensor(u0, specs.device, N, T).clone()
    shift_λ, slope_λ = _check_lambdas(shift_λ, slope_λ)
    best_loss = torch.empty(N, dtype=torch.float64, device=specs.device)
    _minimize_pl(_Problem(specs, target), u, shift_λ, slope_λ, slope_λ == np.inf, best_loss)
    return (u.cpu().numpy(), best_loss.cpu().numpy()) if is_numpy else (u, best_loss)


def align_specs(specs, shift_λs, slope_λs, verbose=True, *, n_knots=0):
    """``align_specs`` (warping.py:53-145): align the spectrograms ``[n_specs, freq_bins, time_bins]`` by per-spectrogram
    shifts and slopes, alternating the mean warped spectrogram as the target with ``minimize_warp`` under
    ``shift_λs[i]``, ``slope_λs[i]`` (``slope_λ = inf``: a shift-only iteration, after which the log slope is 0), for
    ``min(len(shift_λs), len(slope_λs))`` iterations.  Returns ``(warped_specs, warp_params)``: the warped spectrograms
    in the shape, dtype and kind of ``specs``, and ``{'shifts': [n_specs], 'slopes': [n_specs]}`` in time bins, such that
    ``apply_warp(specs, warp_params)`` is ``warped_specs``.  Warns that the module is experimental, as the reference
    does.  The iterations are enqueued back to back; the ``verbose`` lines (the last spectrogram's loss per iteration,
    warping.py:141-143) are printed once all of them are.  There is no ``(None, None)`` return.

    ``n_knots > 0`` (no counterpart in the reference): a piecewise-linear warp of ``n_knots + 2`` knots per spectrogram,
    every iteration fitting stage A and then stage B of the module docstring.  Stage B does not warm-start: every
    iteration rebuilds the knots from stage A's line ``shift + slope t_k`` and the previous iteration's knots reach it
    only through the mean template.  ``warp_params`` then also holds
    ``'knots'`` ``[n_specs, n_knots + 2]`` in time bins, which ``apply_warp`` uses; ``'shifts'`` and ``'slopes'`` are
    stage A's last values."""
    warnings.warn(WARNING_MSG)
    specs, is_numpy = _specs_tensor(specs)
    N, F, T = specs.shape
    n_knots = int(n_knots)
    if n_knots != 0:
        _check_knots(T, n_knots + 2)
    dev = specs.device
    total_iterations = min(len(shift_λs), len(slope_λs))
    schedule = [_check_lambdas(shift_λs[i], slope_λs[i]) for i in range(total_iterations)]
    warped = specs.clone()
    x = torch.zeros((N, 2), dtype=torch.float64, device=dev)
    params = torch.stack([x[:, 0], torch.exp(x[:, 1])], dim=1)
    if n_knots != 0:
        t_k = torch.from_numpy(knot_columns(T, n_knots + 2)).to(dev)
        knots = (params[:, :1] + params[:, 1:] * t_k).contiguous()
    prob = _Problem(specs, torch.empty((F, T), dtype=torch.float64, device=dev))
    best_loss = torch.empty(N, dtype=torch.float64, device=dev)
    last_losses = torch.zeros(max(total_iterations, 1), dtype=torch.float64, device=dev)
    for warp_iter, (shift_λ, slope_λ) in enumerate(schedule):
        fixed = slope_λ == np.inf
        _lib.check(_lib.load().ava_warpfit_mean(warped.data_ptr(), _DTYPES[warped.dtype], N, F, T, prob.target.data_ptr(),
                                                _lib.stream()), "ava_warpfit_mean")
        _minimize(prob, x, shift_λ, slope_λ, fixed, best_loss)
        if fixed:
            x[:, 1] = 0.0                                   # slope = 1, log slope = 0 (warping.py:132-133)
        params = torch.stack([x[:, 0], torch.exp(x[:, 1])], dim=1)
        if n_knots == 0:
            warped = _apply(specs, params, False)
        else:
            knots = (params[:, :1] + params[:, 1:] * t_k).contiguous()     # stage A's line: u_k = shift + slope t_k
            if not fixed:
                _minimize_pl(prob, knots, shift_λ, slope_λ, False, best_loss)
            warped = _apply(specs, knots, True)
        last_losses[warp_iter] = best_loss[-1]
    if verbose:
        for warp_iter, loss in enumerate(last_losses[:total_iterations].cpu().numpy()):
            print("Iteration {}, loss={}".format(warp_iter, round(float(loss), 3)))
    warp_params = {'shifts': params[:, 0].contiguous(), 'slopes': params[:, 1].contiguous()}
    if n_knots != 0:
        warp_params['knots'] = knots
    if is_numpy:
        return warped.cpu().numpy(), {k: v.cpu().numpy() for k, v in warp_params.items()}
    return warped, warp_params


# ---- grouped fits (row f17): many fit problems over the same spectrograms in one launch sequence ---------------------------

def check_group_schedule(shift_λs, slope_λs, n_groups):
    """The schedules of ``align_specs_grouped`` as float64 arrays ``[iterations, n_groups]``: the conditions of
    ``check_schedule`` for every group, and within an iteration either every ``slope_λ`` is ``inf`` or none is (the
    shift objective is one flag of a launch).  ``ValueError`` otherwise."""
    a, b = np.asarray(shift_λs, dtype=np.float64), np.asarray(slope_λs, dtype=np.float64)
    if a.ndim != 2 or a.shape != b.shape or a.shape[1] != n_groups:
        raise ValueError("shift_λs and slope_λs must both be [iterations][%d groups], got %s and %s"
                         % (n_groups, a.shape, b.shape))
    if a.shape[0] == 0:
        raise ValueError("an empty schedule fits nothing")
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError("every shift_λ must be finite and not negative (only slope_λ may be inf)")
    if np.isnan(b).any() or (b < 0).any():
        raise ValueError("every slope_λ must be inf or not negative")
    inf = np.isinf(b)
    if (inf.any(axis=1) != inf.all(axis=1)).any():
        raise ValueError("within an iteration slope_λ = inf (a shift-only iteration) must hold for every group or for none")
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _index_list(idx, size, what):
    """a sorted index list without repeats inside ``range(size)`` as int32; ``None``: all"""
    if idx is None:
        return np.arange(size, dtype=np.int32)
    a = np.asarray(idx)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("a group's %s must be a non-empty 1-D index list" % what)
    if a.dtype.kind not in 'iu':
        raise ValueError("a group's %s must be integers, got %s" % (what, a.dtype))
    if a.min() < 0 or a.max() >= size:
        raise ValueError("a group's %s must lie in [0, %d)" % (what, size))
    if (np.diff(a.astype(np.int64)) <= 0).any():
        raise ValueError("a group's %s must be sorted and without repeats" % what)
    return a.astype(np.int32)


def check_groups(groups, N, F):
    """``[(rows, bins), ...]`` as int32 index arrays: every list sorted, without repeats, not empty and in range
    (``None``: all rows / all bins).  ``ValueError`` otherwise, before anything is launched."""
    groups = list(groups)
    if len(groups) == 0:
        raise ValueError("no groups to fit")
    out = []
    for g in groups:
        if g is None:
            g = (None, None)
        if len(g) != 2:
            raise ValueError("a group is a pair (rows, bins)")
        out.append((_index_list(g[0], N, "rows"), _index_list(g[1], F, "bins")))
    return out


class GroupPlan:
    """The device-side plan of a list of checked groups over ``specs`` [N, F, T] (a contiguous device tensor): the int32
    arrays of include/ava_hip.h, the grouped template and the grouped losses.  Nothing here synchronises."""

    def __init__(self, specs, groups):
        self.specs = specs
        self.N, self.F, self.T = specs.shape
        self.G = len(groups)
        rows = [g[0] for g in groups]
        bins = [g[1] for g in groups]
        self.row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        self.bin_off = np.concatenate([[0], np.cumsum([len(b) for b in bins])]).astype(np.int64)
        self.V, self.max_bins = int(self.row_off[-1]), int(max(len(b) for b in bins))
        if self.V > 2 ** 31 - 1 or int(self.bin_off[-1]) * self.T > 2 ** 31 - 1:
            raise ValueError("too many virtual rows or target cells for one plan: use max_rows")
        dev = specs.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.row_src = up(np.concatenate(rows))
        self.row_group_host = np.repeat(np.arange(self.G), np.diff(self.row_off))
        self.row_group = up(self.row_group_host)
        self.d_row_off, self.d_bin_off, self.bins = up(self.row_off), up(self.bin_off), up(np.concatenate(bins))
        self.targets = torch.empty(int(self.bin_off[-1]) * self.T, dtype=torch.float64, device=dev)

    def _head(self):
        s = self.specs
        return (s.data_ptr(), _DTYPES[s.dtype], self.N, self.F, self.T, self.row_src.data_ptr())

    def mean(self, params=None, knots=None, out=None):
        """the grouped template into ``out`` (default: the plan's own targets) under ``params`` [V, 2] = (shift, slope),
        under ``knots`` [V, K], or of the unwarped rows when both are ``None``"""
        out = self.targets if out is None else out
        tail = (self.d_row_off.data_ptr(), self.d_bin_off.data_ptr(), self.bins.data_ptr(), self.G, self.max_bins)
        if knots is not None:
            warp = (knots.data_ptr(), knots.shape[1], 0)
        else:
            warp = (None if params is None else params.data_ptr(), int(params is None))
        _entry("group_%smean", knots is not None, *self._head(), *tail, *warp, out.data_ptr(), _lib.stream())
        return out

    def loss(self, pl, cand, shift_λ, slope_λ, fixed, loss, targets=None, raw=False):
        """``ava_warpfit_group_loss`` of ``cand`` [V, C, 2] = (shift, log slope) or, with ``pl``,
        ``ava_warpfit_group_pl_loss`` of ``cand`` [V, C, K] into ``loss`` [V, C] against ``targets`` (default: the plan's
        own); λ: device [G].  ``raw``: no warp, no candidates, no λ, ``loss`` [V]."""
        targets = self.targets if targets is None else targets
        ptr = lambda t: None if t is None else t.data_ptr()
        k = (cand.shape[2],) if pl else ()
        _entry("group_%sloss", pl, *self._head(), self.row_group.data_ptr(), self.d_bin_off.data_ptr(), self.bins.data_ptr(),
               self.V, targets.data_ptr(), ptr(cand), 1 if cand is None else cand.shape[1], *k, ptr(shift_λ), ptr(slope_λ),
               int(bool(fixed)), int(bool(raw)), loss.data_ptr(), _lib.stream())
        return loss

    def ss_loss(self, cand, shift_λ, slope_λ, fixed, loss, targets=None):
        """``loss`` of ``cand`` [V, C, 2] = (shift, log slope)"""
        return self.loss(False, cand, shift_λ, slope_λ, fixed, loss, targets)

    def pl_loss(self, cand, shift_λ, slope_λ, fixed, loss, targets=None):
        """``loss`` of ``cand`` [V, C, K]"""
        return self.loss(True, cand, shift_λ, slope_λ, fixed, loss, targets)

    def raw_loss(self, loss, targets=None):
        """per virtual row the sum of squared differences of the unwarped row from its group's target, into ``loss`` [V]"""
        return self.loss(False, None, None, None, False, loss, targets, raw=True)


def _fit_plan(plan, shift_λs, slope_λs, n_knots):
    """the iterations of ``align_specs`` over the virtual rows of ``plan``; ``shift_λs``, ``slope_λs``: numpy
    [iterations, G].  Returns device tensors ``(params [V, 2] = (shift, slope), knots [V, K] or None)``."""
    dev, V, T = plan.specs.device, plan.V, plan.T
    d_shift, d_slope = torch.from_numpy(shift_λs).to(dev), torch.from_numpy(slope_λs).to(dev)
    x = torch.zeros((V, 2), dtype=torch.float64, device=dev)
    params = torch.stack([x[:, 0], torch.exp(x[:, 1])], dim=1)
    knots = None
    if n_knots != 0:
        t_k = torch.from_numpy(knot_columns(T, n_knots + 2)).to(dev)
    best_loss = torch.empty(V, dtype=torch.float64, device=dev)
    for it in range(len(shift_λs)):
        fixed = bool(np.isinf(slope_λs[it, 0]))
        if it == 0:
            plan.mean()                                     # the unwarped rows: an identity warp is not bit-exact
        elif n_knots == 0:
            plan.mean(params=params)
        else:
            plan.mean(knots=knots)
        _minimize(plan, x, d_shift[it], d_slope[it], fixed, best_loss)
        if fixed:
            x[:, 1] = 0.0
        params = torch.stack([x[:, 0], torch.exp(x[:, 1])], dim=1).contiguous()
        if n_knots != 0:
            knots = (params[:, :1] + params[:, 1:] * t_k).contiguous()
            if not fixed:
                _minimize_pl(plan, knots, d_shift[it], d_slope[it], False, best_loss)
    return params, knots


def align_specs_grouped(specs, groups, shift_λs, slope_λs, n_knots=0, max_rows=None):
    """Many ``align_specs`` fits over the same spectrograms ``[N, F, T]`` in one launch sequence (row f17).  ``groups``
    is a list of ``(rows, bins)``: sorted index lists without repeats (``None``: all) naming the motifs and the
    frequency bins of one fit problem; ``shift_λs`` and ``slope_λs`` are ``[iterations][len(groups)]``, and within an
    iteration ``slope_λ = inf`` holds for every group or for none.  Returns one dict per group, ``{'shifts', 'slopes'}``
    and with ``n_knots > 0`` also ``'knots'``, numpy for numpy ``specs`` and device tensors otherwise: bit for bit the
    ``warp_params`` that ``align_specs(specs[rows][:, bins], shift_λs[:, g], slope_λs[:, g], n_knots=n_knots)`` returns.
    The spectrograms are read where they lie: no gathered copy is made and no warped spectrogram is stored; every
    iteration's templates come from ``ava_warpfit_group_mean``.  All groups advance together, a launch covering
    every (motif, group) pair -- ``V = sum(len(rows))`` virtual rows -- and nothing is read back inside the loop.
    ``max_rows`` bounds ``V`` per launch sequence by running whole groups in chunks (a group larger than ``max_rows``
    runs alone); the result does not depend on it.  ``ValueError`` before any launch for empty, unsorted, repeated or
    out-of-range indices, a schedule of the wrong shape or with a mixed ``inf`` pattern, and unsupported ``n_knots``."""
    specs, is_numpy = _specs_tensor(specs)
    N, F, T = specs.shape
    n_knots = int(n_knots)
    if n_knots != 0:
        _check_knots(T, n_knots + 2)
    groups = check_groups(groups, N, F)
    shift_λs, slope_λs = check_group_schedule(shift_λs, slope_λs, len(groups))
    if max_rows is not None and int(max_rows) < 1:
        raise ValueError("max_rows must be positive")
    chunks, start, count = [], 0, 0
    for g, (rows, _) in enumerate(groups):
        if g > start and max_rows is not None and count + len(rows) > int(max_rows):
            chunks.append((start, g))
            start, count = g, 0
        count += len(rows)
    chunks.append((start, len(groups)))
    out = []
    for a, b in chunks:
        plan = GroupPlan(specs, groups[a:b])
        params, knots = _fit_plan(plan, np.ascontiguousarray(shift_λs[:, a:b]), np.ascontiguousarray(slope_λs[:, a:b]), n_knots)
        for g in range(b - a):
            lo, hi = int(plan.row_off[g]), int(plan.row_off[g + 1])
            wp = {'shifts': params[lo:hi, 0].contiguous(), 'slopes': params[lo:hi, 1].contiguous()}
            if knots is not None:
                wp['knots'] = knots[lo:hi].contiguous()
            out.append(wp)
    if is_numpy:
        return [{k: v.cpu().numpy() for k, v in wp.items()} for wp in out]
    return out


def knots_from_warp_params(warp_params, num_time_bins):
    """The fitted warps as knots of ``DeviceWarpedWindowDataset``: ``(x_knots [N, 2], y_knots [N, 2])`` in quantiles of
    ``template_dur``.  Time bin ``j`` of the fit inputs is the STFT frame at ``j * frame_step`` seconds, i.e. at
    quantile ``j / num_time_bins`` of ``template_dur = num_time_bins * frame_step``; ``warped(j) = spec(shift + slope *
    j)`` therefore maps the template quantile ``y`` to the measured quantile ``x = shift / T + slope * y``:
    ``y_knots = [0, 1]``, ``x_knots = [shift / T, shift / T + slope]``.  With a key ``'knots'`` (``[N, K]`` in time bins,
    strictly increasing) the other two are not read: ``x_knots = knots / T``, ``y_knots = knot_columns(T, K) / T``
    (``[N, K]`` each); the dataset extrapolates the outer segments beyond the outer knots."""
    T = float(num_time_bins)
    if 'knots' in warp_params:
        u = np.asarray(_host(warp_params['knots']), dtype=np.float64)
        if u.ndim != 2 or u.shape[1] < 2:
            raise ValueError("'knots' must be [n_specs, n_knots + 2]")
        if not (np.diff(u, axis=1) > 0).all():
            raise ValueError("knots must be strictly increasing")
        return u / T, np.tile(knot_columns(int(num_time_bins), u.shape[1]) / T, (len(u), 1))
    shifts = np.asarray(_host(warp_params['shifts']), dtype=np.float64).reshape(-1)
    slopes = np.asarray(_host(warp_params['slopes']), dtype=np.float64).reshape(-1)
    if shifts.shape != slopes.shape:
        raise ValueError("'shifts' and 'slopes' must have one entry per spectrogram each")
    if not (slopes > 0).all():
        raise ValueError("slopes must be positive")
    x_knots = np.stack([shifts / T, shifts / T + slopes], axis=1)
    y_knots = np.tile([0.0, 1.0], (len(shifts), 1))
    return x_knots, y_knots


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else a


def install(module=None):
    """Point ``align_specs`` and ``apply_warp`` of ``module`` (by default ``ava.preprocessing.warping``, imported after
    the reference package) at this module."""
    if module is None:
        import ava.preprocessing.warping as module
    module.align_specs = align_specs
    module.apply_warp = apply_warp
    return module
