"""The host prelude that the analysis modules share: rows arrive as numpy arrays or tensors, on the host or the device,
of any dtype, and leave as contiguous float32 / float64 device tensors.  Shapes, limits and error messages differ from
module to module and stay with them; the ABI side (dtype codes, workspaces, the device) is in ``_lib``.
"""
import numpy as np
import torch


def native(X):
    """``X`` as a numpy array or a tensor: float32 and float64 as they are, every other dtype as float64"""
    if torch.is_tensor(X):
        return X if X.dtype in (torch.float32, torch.float64) else X.to(torch.float64)
    X = np.asarray(X)
    return X if X.dtype in (np.float32, np.float64) else X.astype(np.float64)


def is_finite(X):
    return bool((torch.isfinite(X) if torch.is_tensor(X) else np.isfinite(X)).all())


def has_nan(X):
    return bool((torch.isnan(X) if torch.is_tensor(X) else np.isnan(X)).any())


def upload(X, dev, dtype=None):
    """a contiguous tensor on ``dev``, cast to ``dtype`` if one is given: of a host array through ``ascontiguousarray``,
    of a tensor by moving it"""
    t = X if torch.is_tensor(X) else torch.from_numpy(np.ascontiguousarray(X))
    return t.to(device=dev, dtype=dtype).contiguous()
