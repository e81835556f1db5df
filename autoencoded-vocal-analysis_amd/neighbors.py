"""Exact 1-nearest-neighbour search on the device.

The two searches of the reference's ``shotgun_movie_DC`` (``ava/plotting/shotgun_movie.py``):

  ``metric='correlation'``  ``NearestNeighbors(n_neighbors=1, metric='correlation')`` over spectrograms (:148-158),
                            i.e. scipy's fp64 ``cdist(..., 'correlation')`` and an argmin per query
  ``metric='euclidean'``    ``np.argmin([euclidean(latent[i], j) for j in original_latent])`` (:126-133)

Both run in ``csrc/neighbors.hip`` (fp64 throughout).  Equal distances resolve to the lowest reference index.
Correlation: a zero-variance row gives NaN distances (as in scipy), NaN loses to any number, and a query whose
distances are all NaN gets index 0 and distance NaN -- sklearn's ``argpartition`` returns an arbitrary row there.
Euclidean: the first NaN wins, as ``np.argmin`` returns it.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from ._rows import native, upload       # by name: ``_rows`` here is this module's reshaping function

__all__ = ["nearest", "METRICS", "MAX_DIM", "DEFAULT_CHUNK_BYTES"]

METRICS = {'correlation': 0, 'euclidean': 1}
MAX_DIM = 65536
DEFAULT_CHUNK_BYTES = 1 << 30        # host references uploaded per launch when chunk_rows is not given


def _device():
    return _lib.device("nearest-neighbour")


def _rows(x, d, what):
    """``x`` as ``[n, d]`` (numpy array or device tensor, float32 / float64 kept, other dtypes as float64); ``d=None``
    takes the row length from ``x`` itself: a 1-D ``x`` is one row, otherwise ``reshape(-1, prod(shape[1:]))``."""
    if torch.is_tensor(x) and x.device.type != "cuda":
        x = x.detach().numpy()
    x = native(x.detach() if torch.is_tensor(x) else x)
    shape = tuple(x.shape)
    n_el = int(np.prod(shape, dtype=np.int64))
    if d is None:
        if len(shape) == 0:
            raise ValueError("%s must have at least one dimension" % what)
        d = shape[-1] if len(shape) == 1 else int(np.prod(shape[1:], dtype=np.int64))
    if d < 1 or n_el == 0 or n_el % d:
        raise ValueError("%s of shape %s cannot be reshaped to [-1, %d]" % (what, shape, d))
    return x.reshape(-1, d)


def nearest(queries, refs, metric='correlation', chunk_rows=None):
    """Index and distance of the nearest row of ``refs`` for every row of ``queries``: ``(idx int64 [nq],
    dist float64 [nq])`` as numpy arrays.

    ``queries`` / ``refs``: numpy arrays or device tensors, 2-D or reshapeable to ``[n, d]`` (``reshape(-1, dim)``
    as the reference does; ``d`` is the queries' row length).  float32 and float64 inputs are read as they are.
    Host references go to the device in chunks of at most ``chunk_rows`` rows (default: 1 GiB of rows), device
    references in one launch unless ``chunk_rows`` says otherwise; the chunks are combined on the device under the
    same order (an earlier chunk wins ties), so the result does not depend on ``chunk_rows``."""
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    q = _rows(queries, None, "queries")
    nq, d = int(q.shape[0]), int(q.shape[1])
    r = _rows(refs, d, "refs")
    nr = int(r.shape[0])
    if d > MAX_DIM:
        raise ValueError("row length %d exceeds %d" % (d, MAX_DIM))
    if nq >= 2 ** 31 or nr >= 2 ** 31:
        raise ValueError("at most 2**31 - 1 rows per operand")
    if chunk_rows is None:
        chunk_rows = nr if torch.is_tensor(r) else max(1, DEFAULT_CHUNK_BYTES // (d * r.dtype.itemsize))
    elif int(chunk_rows) != chunk_rows or chunk_rows < 1:
        raise ValueError("chunk_rows must be a positive integer")
    chunk_rows = min(int(chunk_rows), nr)
    code = METRICS[metric]
    lib = _lib.load()
    nbytes = lib.ava_nn_workspace_bytes(nq, chunk_rows, d, code)
    if nbytes == 0:                                     # refused here, before the device is asked for
        raise ValueError("unsupported shape: %d queries, %d references of length %d" % (nq, chunk_rows, d))
    dev = _device()
    qd = upload(q, dev)
    ws = _lib.workspace(nbytes, dev, "nearest")
    best_idx = torch.empty(nq, dtype=torch.int64, device=dev)
    best_dist = torch.empty(nq, dtype=torch.float64, device=dev)
    idx = torch.empty_like(best_idx) if chunk_rows < nr else best_idx
    dist = torch.empty_like(best_dist) if chunk_rows < nr else best_dist
    st = _lib.stream()
    for start in range(0, nr, chunk_rows):
        rd = upload(r[start:start + chunk_rows], dev)
        n = int(rd.shape[0])
        oi, od = (best_idx, best_dist) if start == 0 else (idx, dist)
        _lib.check(lib.ava_nn_argmin(qd.data_ptr(), _lib.dtype_code(qd), nq, rd.data_ptr(), _lib.dtype_code(rd), n, d,
                                     code, oi.data_ptr(), od.data_ptr(), ws.data_ptr(), nbytes, st), "ava_nn_argmin")
        if start:
            _lib.check(lib.ava_nn_merge(best_idx.data_ptr(), best_dist.data_ptr(), idx.data_ptr(), dist.data_ptr(), nq,
                                        start, code, st), "ava_nn_merge")
    return best_idx.cpu().numpy(), best_dist.cpu().numpy()
