"""The integer-shift time-warp fit on the device.

The reference's ``segment_sylls_from_songs`` (ava/segmenting/template_segmentation.py:455-627) aligns the amplitude traces
of all song renditions with ``affinewarp.ShiftWarping(maxlag=0.2, smoothness_reg_scale=10.0).fit(..., iterations=50)``.
affinewarp is no dependency here.  ``ShiftWarping`` below has that class's surface (``fit``, ``shifts``, ``template``,
``transform``, ``predict``, ``loss_hist``) over this project's own model.  It is NOT affinewarp's code or arithmetic; it
shares the sign convention the reference relies on (lines 552, 602-603): template column ``t`` lies at raw column
``t + shift_k``.

The model.  Data is ``x [K, F, T]`` (float32 or float64; all arithmetic is fp64; ``F = 1`` for amplitude traces),
``L = int(maxlag * T)``, the shifts ``s_k`` are integers in ``[-L, L]`` and start at 0.  One iteration:

  1. Template.  ``m̄[f, t] = sum_k x[k, f, clip(t + s_k, 0, T-1)] / K``; then, for every ``f``, ``A m[f, :] = m̄[f, :]``
     with ``A = (1 + l2 / K) I + λ D₂ᵀD₂`` (T x T, symmetric, pentadiagonal; ``D₂``: the ``(T-2) x T`` second differences
     ``(1, -2, 1)``; ``λ = smoothness_reg_scale``, affinewarp's per-trial scaling with ``K`` divided out; ``l2 = 1e-7``).
  2. Loss.  ``loss[k, c] = sum_{f,t} (x[k, f, clip(t + lag_c, 0, T-1)] - m[f, t]) ** 2 / (F T)`` for the lags
     ``lag_c = 0, -1, +1, -2, +2, ..., -L, +L``: candidate 0 is "no shift".
  3. Shifts.  ``s_k = lag_{argmin_c loss[k, c]}``; the lowest ``c`` wins ties (a constant trace keeps shift 0), NaN
     never wins.

Both half-steps minimise ``J = sum_k sum (aligned_k - m) ** 2 + K λ |D₂ m|² + l2 |m|²`` over their own variables, so
neither can raise it.  The shifts are not re-centred: every iteration searches absolute lags, nothing drifts, and a
common offset of all shifts is immaterial to the caller, who picks quantiles on the aligned picture.  The number of
launches depends on ``(T, L, iterations)`` alone and nothing is read back inside ``fit``; once the shifts repeat, later
iterations reproduce them.

Every number is made by the kernels of ``csrc/shift_fit.hip``; there is no CPU fallback.  ``T`` is at least 3
(``ValueError``) and at most ``ava_shiftfit_max_t()`` = 2048 (``NotImplementedError``).  Numpy in gives numpy out,
device tensors in give device tensors out.
"""
import numpy as np
import torch

from . import _lib

__all__ = ["L2_REG_SCALE", "lag_order", "shift_loss", "shift_template", "ShiftWarping"]

L2_REG_SCALE = 1e-7

_DTYPES = {torch.float32: 0, torch.float64: 1}


def lag_order(L):
    """the lags in candidate order: ``[0, -1, +1, -2, +2, ..., -L, +L]``, int64 ``[2 L + 1]``"""
    L = int(L)
    if L < 0:
        raise ValueError("L must not be negative, got %d" % L)
    c = np.arange(2 * L + 1, dtype=np.int64)
    return np.where(c & 1, -((c + 1) >> 1), c >> 1)


def _data_tensor(x):
    """``(contiguous device tensor [K, F, T], came as numpy)``; every shape check, before any launch"""
    is_numpy = not torch.is_tensor(x)
    if is_numpy:
        x = np.asarray(x)
        if x.dtype not in (np.float32, np.float64):
            raise TypeError("data must be float32 or float64, got %s" % x.dtype)
        if x.ndim != 3:
            raise ValueError("expected data of rank 3, got rank %d" % x.ndim)
    elif x.dtype not in _DTYPES:
        raise TypeError("data must be float32 or float64, got %s" % x.dtype)
    elif x.dim() != 3:
        raise ValueError("expected data of rank 3, got rank %d" % x.dim())
    K, F, T = x.shape
    if K < 1 or F < 1:
        raise ValueError("expected at least one trial and one feature, got shape %s" % (tuple(x.shape),))
    if T < 3:
        raise ValueError("a shift fit needs at least three time bins, got %d" % T)
    cap = _lib.load().ava_shiftfit_max_t()
    if T > cap:
        raise NotImplementedError("at most %d time bins per trial, got %d" % (cap, T))
    if F * T >= 2 ** 30:
        raise NotImplementedError("at most 2^30 values per trial")
    if is_numpy:
        x = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    return x.contiguous(), is_numpy


def _check_L(L, T):
    L = int(L)
    if L < 0 or L > T - 1:
        raise ValueError("L must lie in [0, T - 1] = [0, %d], got %d" % (T - 1, L))
    return L


def _check_reg(smoothness_reg_scale, l2_reg_scale):
    lam, l2 = float(smoothness_reg_scale), float(l2_reg_scale)
    if not np.isfinite(lam) or lam < 0 or not np.isfinite(l2) or l2 < 0:
        raise ValueError("smoothness_reg_scale and l2_reg_scale must be finite and not negative")
    return lam, l2


def _loss(x, template, L, loss):
    K, F, T = x.shape
    rc = _lib.load().ava_shiftfit_loss(x.data_ptr(), _DTYPES[x.dtype], K, F, T, template.data_ptr(), L, loss.data_ptr(),
                                       _lib.stream())
    _lib.check(rc, "ava_shiftfit_loss")


def _template(x, shifts, lam, l2, mbar, template, ws):
    K, F, T = x.shape
    rc = _lib.load().ava_shiftfit_template(x.data_ptr(), _DTYPES[x.dtype], K, F, T, shifts.data_ptr(), lam, l2,
                                           _lib.ptr(mbar), template.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream())
    _lib.check(rc, "ava_shiftfit_template")


def _workspace(x):
    K, F, T = x.shape
    return _lib.workspace(_lib.load().ava_shiftfit_workspace_bytes(K, F, T), x.device, "[%d, %d, %d]" % (K, F, T))


def _apply(x, shifts):
    K, F, T = x.shape
    out = torch.empty_like(x)
    rc = _lib.load().ava_shiftfit_apply(x.data_ptr(), _DTYPES[x.dtype], K, F, T, shifts.data_ptr(), out.data_ptr(),
                                        _lib.stream())
    _lib.check(rc, "ava_shiftfit_apply")
    return out


def _shifts_tensor(shifts, dev, K):
    t = shifts if torch.is_tensor(shifts) else torch.from_numpy(np.ascontiguousarray(np.asarray(shifts)))
    if t.dim() != 1 or t.shape[0] != K:
        raise ValueError("expected %d shifts, got shape %s" % (K, tuple(t.shape)))
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("shifts must be integers")
    return t.to(device=dev, dtype=torch.int32).contiguous()


def shift_loss(x, template, L):
    """Step 2 of the module docstring: ``loss [K, 2 L + 1]`` float64 of ``x [K, F, T]`` against ``template [F, T]`` for
    the lags ``lag_order(L)``.  Sums run in a fixed order: two calls give the same bits.  Numpy for numpy ``x``."""
    x, is_numpy = _data_tensor(x)
    K, F, T = x.shape
    L = _check_L(L, T)
    tm = template if torch.is_tensor(template) else torch.from_numpy(np.asarray(template, dtype=np.float64))
    if tuple(tm.shape) != (F, T):
        raise ValueError("expected a template of shape %s, got %s" % ((F, T), tuple(tm.shape)))
    tm = tm.to(device=x.device, dtype=torch.float64).contiguous()
    loss = torch.empty((K, 2 * L + 1), dtype=torch.float64, device=x.device)
    _loss(x, tm, L, loss)
    return loss.cpu().numpy() if is_numpy else loss


def shift_template(x, shifts, smoothness_reg_scale, l2_reg_scale=L2_REG_SCALE, return_mean=False):
    """Step 1 of the module docstring: the smoothed template ``m [F, T]`` float64 of ``x [K, F, T]`` under the integer
    ``shifts [K]``; with ``return_mean`` ``(m, m̄)``.  Numpy for numpy ``x``."""
    x, is_numpy = _data_tensor(x)
    K, F, T = x.shape
    lam, l2 = _check_reg(smoothness_reg_scale, l2_reg_scale)
    s = _shifts_tensor(shifts, x.device, K)
    mbar = torch.empty((F, T), dtype=torch.float64, device=x.device)
    m = torch.empty_like(mbar)
    _template(x, s, lam, l2, mbar, m, _workspace(x))
    if is_numpy:
        m, mbar = m.cpu().numpy(), mbar.cpu().numpy()
    return (m, mbar) if return_mean else m


class ShiftWarping:
    """The surface of ``affinewarp.ShiftWarping`` the reference uses, over the model of the module docstring.

    ``fit(data, iterations=20)`` takes affinewarp's ``[K, T, N]`` layout (trials, time bins, features).  Afterwards
    ``shifts`` is a numpy int array ``[K]``, ``template`` is ``[T, N]`` (the template the last shifts were chosen
    against) and ``loss_hist`` the list of ``J / (K T N)`` after every iteration, read back once after the last one.
    ``transform(data)`` aligns data of ``K`` trials (``aligned[k, t] = data[k, clip(t + shift_k)]``, exact copies);
    ``predict()`` is the template shifted back onto every trial, ``[K, T, N]``: what the reference plots as 'Shifted'."""

    def __init__(self, maxlag=0.5, smoothness_reg_scale=0.0, l2_reg_scale=L2_REG_SCALE):
        maxlag = float(maxlag)
        if not 0 <= maxlag < 1:
            raise ValueError("maxlag must lie in [0, 1), got %r" % maxlag)
        self.maxlag = maxlag
        self.smoothness_reg_scale, self.l2_reg_scale = _check_reg(smoothness_reg_scale, l2_reg_scale)
        self.shifts = None
        self.template = None
        self.loss_hist = []
        self._shifts = None

    @staticmethod
    def _kft(data):
        """affinewarp's ``[K, T, N]`` as the kernels' ``[K, N, T]``"""
        if torch.is_tensor(data):
            if data.dim() != 3:
                raise ValueError("expected data of shape [trials, time bins, features], got rank %d" % data.dim())
            return data.transpose(1, 2)
        data = np.asarray(data)
        if data.ndim != 3:
            raise ValueError("expected data of shape [trials, time bins, features], got rank %d" % data.ndim)
        return data.transpose(0, 2, 1)

    def fit(self, data, iterations=20, verbose=False):
        iterations = int(iterations)
        if iterations < 1:
            raise ValueError("at least one iteration")
        x, is_numpy = _data_tensor(self._kft(data))
        K, F, T = x.shape
        L = int(self.maxlag * T)
        lam, l2 = self.smoothness_reg_scale, self.l2_reg_scale
        lib, dev, st = _lib.load(), x.device, _lib.stream()
        shifts = torch.zeros(K, dtype=torch.int32, device=dev)
        m = torch.empty((F, T), dtype=torch.float64, device=dev)
        loss = torch.empty((K, 2 * L + 1), dtype=torch.float64, device=dev)
        best = torch.empty(K, dtype=torch.float64, device=dev)
        hist = torch.empty(iterations, dtype=torch.float64, device=dev)
        ws = _workspace(x)
        for it in range(iterations):
            _template(x, shifts, lam, l2, None, m, ws)
            _loss(x, m, L, loss)
            _lib.check(lib.ava_shiftfit_argmin(loss.data_ptr(), K, L, shifts.data_ptr(), best.data_ptr(), st),
                       "ava_shiftfit_argmin")
            # J / (K T N): the data term is the sum of the chosen losses, the penalties are a few [F, T] operations
            d2 = m[:, 2:] - 2.0 * m[:, 1:-1] + m[:, :-2]
            hist[it] = best.sum() / K + (lam * (d2 * d2).sum() + (l2 / K) * (m * m).sum()) / (F * T)
        self.loss_hist = [float(v) for v in hist.cpu().numpy()]
        self._shifts = shifts
        self.shifts = shifts.cpu().numpy().astype(np.int64)
        self.template = m.t().contiguous()
        if is_numpy:
            self.template = self.template.cpu().numpy()
        if verbose:
            for it, v in enumerate(self.loss_hist):
                print("Iteration {}, loss={}".format(it, v))
        return self

    def _fitted(self):
        if self._shifts is None:
            raise ValueError("fit() has not been called")

    def transform(self, data):
        self._fitted()
        x, is_numpy = _data_tensor(self._kft(data))
        if x.shape[0] != self._shifts.shape[0]:
            raise ValueError("expected %d trials, got %d" % (self._shifts.shape[0], x.shape[0]))
        out = _apply(x, self._shifts.to(x.device)).transpose(1, 2).contiguous()
        return out.cpu().numpy() if is_numpy else out

    def predict(self):
        self._fitted()
        is_numpy = not torch.is_tensor(self.template)
        m = torch.from_numpy(self.template).to(self._shifts.device) if is_numpy else self.template
        K = self._shifts.shape[0]
        tiled = m.t().unsqueeze(0).expand(K, -1, -1).contiguous()
        out = _apply(tiled, -self._shifts).transpose(1, 2).contiguous()   # raw column t shows template column t - shift
        return out.cpu().numpy() if is_numpy else out
