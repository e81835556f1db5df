"""Cases and the numpy fp64 restatement for ava_amd.tsne (exact t-SNE, row f19).

Inputs come from ava_amd.synthetic's hash streams, so the same arrays are produced anywhere.  The restatement follows
scikit-learn 1.7's exact path step by step (``_t_sne.py``: ``_joint_probabilities``, ``_kl_divergence``,
``_gradient_descent``, ``TSNE._tsne``; ``_utils.pyx``: ``_binary_search_perplexity``) with this package's deviations:
direct-difference squared distances and fp64 positions.  It is the oracle of the GPU tests; tests/test_cpu_tsne.py
holds it against sklearn's own functions through tests/golden/tsne.npz.

Two rules of the algorithm are discontinuous, so two implementations that differ in the last bits agree only away from
their thresholds.  ``check_search_margin`` and ``descent_reference`` assert, on the CPU, that the cases are."""
import functools

import numpy as np

from ava_amd import synthetic as syn

MACHINE_EPSILON = np.finfo(np.double).eps
EPSILON_DBL = float(np.float32(1e-8))               # C floats in _utils.pyx
PERPLEXITY_TOLERANCE = float(np.float32(1e-5))
SEARCH_MARGIN = 1e-9
GAIN_MARGIN = 1e-9


# ---- inputs ----------------------------------------------------------------------------------------------------------
def perplexity_for(n):
    return 2.0 if n == 5 else min(30.0, (n - 1) / 3.0)


def blobs(n, d, c, salt, dtype=np.float32, spread=4.0):
    """``c`` Gaussian blobs (centres ``spread`` N(0, 1), unit noise), labels ``i % c``: (rows [n, d], labels)"""
    centres = spread * syn.gauss(c * d, salt).reshape(c, d)
    labels = np.arange(n) % c
    X = centres[labels] + syn.gauss(n * d, salt + 1).reshape(n, d)
    return X.astype(dtype), labels


def duplicates(n=65, d=8, salt=9710):
    """exact copies of rows: zero distances off the diagonal"""
    X = syn.gauss(n * d, salt).reshape(n, d).astype(np.float32)
    X[[7, 33, 64]] = X[5]
    X[40:46] = X[40]
    return X


def outlier(n=65, d=8, salt=9720):
    """row 11 so far away that exp(-d^2) underflows for every neighbour at beta = 1: its search starts from
    sum_Pi == 0 (EPSILON_DBL), and its joint probabilities end at the eps clamp"""
    X = syn.gauss(n * d, salt).reshape(n, d).astype(np.float32)
    X[11] += 1000.0
    return X


# name -> (rows, perplexity); the shapes of the issue: tile tails, one tile, several tiles; d in {3, 32, 33}; both dtypes
P_CASES = {
    "n5": lambda: (blobs(5, 3, 2, 9601, np.float64)[0], perplexity_for(5)),
    "n63": lambda: (blobs(63, 3, 3, 9602, np.float32)[0], perplexity_for(63)),
    "n64": lambda: (blobs(64, 32, 3, 9603, np.float64)[0], perplexity_for(64)),
    "n65": lambda: (blobs(65, 33, 3, 9604, np.float32)[0], perplexity_for(65)),
    "n130": lambda: (blobs(130, 32, 4, 9605, np.float32)[0], perplexity_for(130)),
    "n300": lambda: (blobs(300, 33, 5, 9606, np.float64)[0], perplexity_for(300)),
    "duplicates": lambda: (duplicates(), perplexity_for(65)),
    "outlier": lambda: (outlier(), perplexity_for(65)),
}
GOLDEN_P_CASES = ["n5", "n63", "n130", "n300", "duplicates", "outlier"]
DESCENT_CASES = ["n5", "n65", "n130", "n300"]          # kl_gradient and descend run on these P
DESCENT_CHUNKS = {"n5": (None,), "n65": (None,), "n130": (1, 3), "n300": (1, 3)}


def run_blobs():
    """the whole-run euclidean case: 150 rows of 4 blobs in 5 dimensions, perplexity 30"""
    X, labels = blobs(150, 5, 4, 9650, np.float32)
    return X, labels, 30.0


def run_precomputed():
    """the whole-run precomputed case: the 40 x 40 euclidean distance matrix (not squared) of 4 blobs of 10 points in
    5 dimensions, perplexity 10 -- the shape of an MMD matrix of 40 conditions.  The centres sit on the corners of a
    square of side 6 in the first two dimensions, so every point's five nearest rows are of its own blob."""
    n, d = 40, 5
    centres = np.zeros((4, d))
    centres[[1, 3], 0] = 6.0
    centres[[2, 3], 1] = 6.0
    labels = np.arange(n) % 4
    X = centres[labels] + syn.gauss(n * d, 9660).reshape(n, d)
    return np.sqrt(sqdist(X)), labels, 10.0


RUN_CASES = {"blobs150": ("euclidean", run_blobs), "precomputed40": ("precomputed", run_precomputed)}
RUN_SEED = 42
RUN_STARTS = 8                  # perturbed restatement runs of the golden file
RUN_PERTURBATION = 1e-12


def random_init(n, seed=RUN_SEED):
    """sklearn's init='random' draw, widened to fp64"""
    return (1e-4 * np.random.RandomState(seed).standard_normal(size=(n, 2)).astype(np.float32)).astype(np.float64)


def spread_y(n, salt=9680):
    """a spread-out layout: positions of a few units"""
    return 3.0 * syn.gauss(2 * n, salt + n).reshape(n, 2)


def clamp_y(n, salt=9690):
    """``spread_y`` with point 2 at distance 1e8 (w / Z falls below eps there: Q's clamp) and points 3 and 4
    coincident"""
    Y = spread_y(n, salt)
    Y[2] = [1e8, -1e8]
    Y[4] = Y[3]
    return Y


# ---- 1. squared distances --------------------------------------------------------------------------------------------
def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    """a * b + c with one rounding (Dekker's exact product and Knuth's exact sum; the last addition rounds the exact
    sum of three parts, which differs from a true fma only at a double-rounding tie)"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    err = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    e2 = (p - (s - bb)) + (c - bb)
    return s + (e2 + err)


def sqdist(X):
    """[N, N] fp64: sum_k (x_k - y_k)^2 with one fma per k, k ascending (the order contract of csrc/sqdist_tile.h)"""
    X = np.asarray(X, dtype=np.float64)
    acc = np.zeros((len(X), len(X)))
    for k in range(X.shape[1]):
        df = X[:, None, k] - X[None, :, k]
        acc = fma(df, df, acc)
    return acc


def round_f32(D2):
    """sklearn's distances.astype(np.float32), kept as fp64"""
    return np.asarray(D2, dtype=np.float64).astype(np.float32).astype(np.float64)


def squared_distances(X, metric="euclidean"):
    if metric == "euclidean":
        return round_f32(sqdist(X))
    D = np.asarray(X, dtype=np.float64)
    return round_f32(D * D)


# ---- 2., 3. probabilities ---------------------------------------------------------------------------------------------
def conditional(D2, perplexity, return_margin=False):
    """_binary_search_perplexity on the full matrix: the conditional probabilities [N, N], and with ``return_margin``
    the smallest ``| |entropy_diff| - PERPLEXITY_TOLERANCE |`` over every step of every row"""
    D2 = np.asarray(D2, dtype=np.float64)
    n = len(D2)
    desired_entropy = float(np.log(np.float64(np.float32(perplexity))))       # `float desired_perplexity`
    C = np.zeros((n, n))
    margin = np.inf
    for i in range(n):
        d = D2[i]
        others = np.arange(n) != i
        beta, beta_min, beta_max = 1.0, -np.inf, np.inf
        for _ in range(100):
            p = np.where(others, np.exp(-d * beta), 0.0)
            sum_pi = p.sum()
            if sum_pi == 0.0:
                sum_pi = EPSILON_DBL
            p = p / sum_pi
            entropy = np.log(sum_pi) + beta * (d * p).sum()
            diff = entropy - desired_entropy
            margin = min(margin, abs(abs(diff) - PERPLEXITY_TOLERANCE))
            if abs(diff) <= PERPLEXITY_TOLERANCE:
                break
            if diff > 0.0:
                beta_min = beta
                beta = beta * 2.0 if beta_max == np.inf else (beta + beta_max) / 2.0
            else:
                beta_max = beta
                beta = beta / 2.0 if beta_min == -np.inf else (beta + beta_min) / 2.0
        C[i] = p
    return (C, margin) if return_margin else C


def joint(C):
    """_joint_probabilities after the search, as a square matrix with a zero diagonal"""
    P = C + C.T
    sum_p = max(P.sum(), MACHINE_EPSILON)
    P = np.maximum(P / sum_p, MACHINE_EPSILON)
    np.fill_diagonal(P, 0.0)
    return P


def joint_probabilities(D2, perplexity):
    return joint(conditional(D2, perplexity))


def check_search_margin(D2, perplexity):
    C, margin = conditional(D2, perplexity, return_margin=True)
    assert margin >= SEARCH_MARGIN, "a search step lies within %.1e of the stopping tolerance: re-salt" % margin
    return joint(C)


# ---- 4. descent ------------------------------------------------------------------------------------------------------
def kl_gradient(Y, P, exaggeration=1.0):
    """_kl_divergence with P scaled by the exaggeration, one degree of freedom: (kl, grad [N, 2])"""
    Y = np.asarray(Y, dtype=np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff ** 2).sum(2))
    off = ~np.eye(len(Y), dtype=bool)
    Z = w[off].sum()
    Q = np.maximum(w / Z, MACHINE_EPSILON)
    pe = exaggeration * P
    kl = float((pe * np.log(np.maximum(pe, MACHINE_EPSILON) / Q))[off].sum())
    grad = 4.0 * (((pe - Q) * w * off)[:, :, None] * diff).sum(1)
    return kl, grad


def descend(Y, update, gains, P, n_iters, momentum, lr, exaggeration, return_margin=False):
    """``n_iters`` iterations of _gradient_descent: new (Y, update, gains), the KL and the norm of grad * gains of the
    last one; with ``return_margin`` also the smallest |update grad| of those iterations relative to the largest (the
    iterations that start from update = 0 left out)"""
    Y, update, gains = (np.array(a, dtype=np.float64) for a in (Y, update, gains))
    kl = grad_norm = np.nan
    margin = np.inf
    for _ in range(n_iters):
        kl, grad = kl_gradient(Y, P, exaggeration)
        prod = update * grad
        if np.any(update != 0.0):
            margin = min(margin, float(np.abs(prod).min() / np.abs(prod).max()))
        inc = prod < 0.0
        gains = np.where(inc, gains + 0.2, gains * 0.8)
        gains = np.maximum(gains, 0.01)
        grad = grad * gains
        update = momentum * update - lr * grad
        Y = Y + update
        grad_norm = float(np.sqrt((grad ** 2).sum()))
    out = (Y, update, gains, kl, grad_norm)
    return out + (margin,) if return_margin else out


def run(P, Y0, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, early_exaggeration=12.0, lr=None):
    """TSNE._tsne on the restatement: (Y, kl_divergence, n_iter)"""
    n = len(P)
    lr = max(n / early_exaggeration / 4.0, 50.0) if lr is None else lr
    state = [np.array(Y0, dtype=np.float64), np.zeros((n, 2)), np.ones((n, 2))]

    def phase(it, last, nwp, momentum, exaggeration):
        error = best_error = np.finfo(float).max
        best_iter = i = it
        for i in range(it, last):
            state[0], state[1], state[2], error, grad_norm = descend(*state, P, 1, momentum, lr, exaggeration)
            if (i + 1) % 50 == 0:
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > nwp:
                    break
                if grad_norm <= min_grad_norm:
                    break
        return error, i

    kl, it = phase(0, 250, 250, 0.5, early_exaggeration)
    if it < 250 or max_iter - 250 > 0:
        kl, it = phase(it + 1, max_iter, n_iter_without_progress, 0.8, 1.0)
    return state[0], kl, it


def neighbour_label_fraction(Y, labels, k=5):
    """fraction of the (point, one of its k nearest others in Y) pairs that share a label"""
    Y = np.asarray(Y, dtype=np.float64)
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(D, np.inf)
    nb = np.argsort(D, axis=1, kind="stable")[:, :k]
    return float((labels[nb] == labels[:, None]).mean())


# ---- shared, read-only references ------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def p_case(name):
    """(rows, perplexity, D2 before the float32 rounding, D2, P); the search margin asserted"""
    X, perplexity = P_CASES[name]()
    raw = sqdist(X)
    D2 = round_f32(raw)
    P = check_search_margin(D2, perplexity)
    X, raw, D2, P = _frozen(X, raw, D2, P)
    return X, perplexity, raw, D2, P


@functools.lru_cache(maxsize=None)
def run_case(name):
    """(metric, input, labels, perplexity, D2, P) of a whole-run case"""
    metric, gen = RUN_CASES[name]
    X, labels, perplexity = gen()
    D2 = squared_distances(X, metric)
    P = check_search_margin(D2, perplexity)
    X, labels, D2, P = _frozen(X, labels, D2, P)
    return metric, X, labels, perplexity, D2, P


DESCENT_STATES = ("spread", "init")


def descent_start(name, state):
    """Y of a descent case: a spread-out layout or sklearn's 1e-4 init"""
    n = len(p_case(name)[0])
    return spread_y(n) if state == "spread" else random_init(n, 7)


def descent_lr(n):
    return max(n / 12.0 / 4.0, 50.0)


@functools.lru_cache(maxsize=None)
def descent_reference(name, state, momentum, exaggeration, n_iters):
    """the restatement's (Y, update, gains, kl, grad_norm) after ``n_iters`` iterations from ``descent_start`` with
    update = 0 and gains = 1; the gains margin asserted"""
    P = p_case(name)[4]
    n = len(P)
    out = descend(descent_start(name, state), np.zeros((n, 2)), np.ones((n, 2)), P, n_iters, momentum, descent_lr(n),
                  exaggeration, return_margin=True)
    assert out[5] >= GAIN_MARGIN, "an update * grad lies within %.1e (relative) of zero: re-salt" % out[5]
    _frozen(*out[:3])
    return out[:5]
