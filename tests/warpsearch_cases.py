"""Shared cases of the grouped warp fits and the warp parameter searches, for
tests/test_cpu_warpsearch.py and tests/test_gpu_warpsearch.py.  Inputs come from ``synthetic.u01`` and the planted recipe
of tests/warppl_cases.py; the anchor score is restated here in plain numpy from its definition."""
import numpy as np

import warppl_cases as PC
from ava_amd import synthetic as syn

# ---- the grouped kernels: N = 5, F = 9, T = 130, C = 19, K = 4 ---------------------------------------------------------
# a lane owns three columns (T = 130 > 128), the bins run over the 4 staged rows, C runs over and off a block of 8
KERNEL_SHAPE = dict(N=5, F=9, T=130, C=19, K=4)
# one row and one bin; a bin list that straddles a staging pass (5 bins: 4 + 1); everything
KERNEL_GROUPS = [([3], [6]), ([0, 2, 4], [1, 3, 4, 5, 8]), (None, None)]
KERNEL_SHIFT_LAMBDAS = [0.01, 0.3, 0.0]              # one per group
KERNEL_SLOPE_LAMBDAS = [0.5, 0.0, 2.0]
# T and K at their caps
CAP_SHAPE = dict(N=3, F=2, T=512, C=9, K=16)
CAP_GROUPS = [([1], [1]), ([0, 2], None)]
# the template alone: more rows than one row set of 16 (two full sets and 5 rows), more bins than the 128 one sweep of a
# 32-workgroup column covers, columns over one 64-column tile and off the second
MEAN_SHAPE = dict(N=37, F=131, T=70, K=5)
MEAN_GROUPS = [(None, None), (list(range(1, 37, 2)), list(range(0, 131, 3))), ([36], [130])]

# ---- align_specs_grouped on the planted motifs of warppl_cases (N = 6, F = 3, T = 97) ------------------------------------
ALIGN_GROUPS = [(None, None), ([0, 2, 3, 5], [0, 2]), ([1, 4], [1])]
ALIGN_SCALES = [(1.0, 1.0), (3.0, 0.25), (0.2, 5.0)]   # (shift, slope) scale of PC.SHIFT_LAMBDAS / PC.SLOPE_LAMBDAS per group

# ---- cross_validate: the planted recipe with F = 10 bins, which the 3 / 1 / 1 folds split 6 / 2 / 2 --------------------
CV_RECIPE = dict(PC.PLANTED, F=10, salt=1501)
CV_PARAMS = dict(samples_per_knot=1, n_valid_samples=2, knot_range=(-1, 2),
                 shift_lambdas=[1e-2, 1e-2, 1e-3, 0.0], slope_lambdas=[np.inf, 1.0, 0.1, 0.0])
CV_SEED = 7


def gather(specs, rows, bins):
    """``specs[rows][:, bins]``, contiguous; ``None``: all"""
    rows = np.arange(specs.shape[0]) if rows is None else np.asarray(rows)
    bins = np.arange(specs.shape[1]) if bins is None else np.asarray(bins)
    return np.ascontiguousarray(specs[rows][:, bins])


def group_sizes(groups, N, F):
    return [(N if r is None else len(r), F if b is None else len(b)) for r, b in groups]


def scaled(base, scale):
    """``scale × base``, ``inf`` and 0 as they are"""
    return [v if v == 0 or np.isinf(v) else scale * v for v in base]


def hashed_params(V, C, T, salt):
    """(shift, log slope) candidates [V, C, 2]: shifts up to 0.3 T either way, so that positions leave the grid"""
    u = syn.u01(V * C * 2, salt).reshape(V, C, 2)
    return np.stack([(2 * u[..., 0] - 1) * 0.3 * T, (2 * u[..., 1] - 1) * 0.3], axis=-1)


def hashed_knots(V, C, T, K, salt):
    """ordered knots [V, C, K]: every knot within 0.3 segments of its column, the whole warp shifted by up to 0.3 T"""
    seg = (T - 1) / (K - 1)
    move = (2 * syn.u01(V * C * K, salt).reshape(V, C, K) - 1) * 0.3 * seg
    shift = (2 * syn.u01(V * C, salt + 1).reshape(V, C, 1) - 1) * 0.3 * T
    return PC.knot_columns(T, K) + move + shift


def anchor_errors(x_knots, y_knots, anchor_times, template_dur):
    """The anchor score from its definition: file i's anchor time a (seconds) has the quantile q = a / template_dur, which
    the piecewise-linear map through (x_knots[i], y_knots[i]) -- its outer segments continued beyond the outer knots --
    takes to a template quantile; back in seconds, the score is the mean absolute deviation of the mapped times from
    their mean over files, times std(anchor times) / std(mapped times), in milliseconds."""
    a = np.asarray(anchor_times, dtype=np.float64)
    mapped = np.zeros_like(a)
    for i in range(len(a)):
        x, y = np.asarray(x_knots[i], np.float64), np.asarray(y_knots[i], np.float64)
        q = a[i] / template_dur
        k = np.clip(np.searchsorted(x, q, side='right') - 1, 0, len(x) - 2)
        mapped[i] = (y[k] + (q - x[k]) * (y[k + 1] - y[k]) / (x[k + 1] - x[k])) * template_dur
    mae = np.abs(mapped - mapped.mean(axis=0, keepdims=True)).mean()
    return 1e3 * mae * a.std() / mapped.std()
