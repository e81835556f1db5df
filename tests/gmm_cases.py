"""Cases and the numpy fp64 restatement for ava_amd.mixture (Gaussian mixture models, row f20).

Inputs come from ava_amd.synthetic's hash streams and are float32-representable, so a float32 and a float64 copy mean
the same data.  The restatement follows scikit-learn 1.7's ``GaussianMixture`` step by step in this package's form:
direct differences ``x - mu`` in the E-step and in both covariance updates, ``nk = sum resp + 10 eps``, a max-shifted
logsumexp, normalised weights also at the start, the package's own Lloyd start (``kmeans``) and sklearn's stopping rule.
It is the oracle of the GPU tests; tests/test_cpu_gmm.py holds it against sklearn itself through tests/golden/gmm.npz.

The stopping rule and the label assignments are discontinuous, so two implementations that differ in the last bits
agree only away from their thresholds: ``fit`` and ``kmeans`` assert, on the CPU, that the cases are."""
import functools

import numpy as np
from scipy.linalg import solve_triangular

from ava_amd import synthetic as syn

EPS10 = 10.0 * np.finfo(np.float64).eps
LOG_2PI = float(np.log(2.0 * np.pi))
CHUNK = 2048                    # ava_gm_chunk_rows
STOP_MARGIN = 1e-9              # ||change| - tol| of every iteration of a fit case
KMEANS_MARGIN = 1e-9            # relative gap between the best and the second-best squared distance
KMEANS_MAX_ITER = 30
ILL_DEFINED = "ill-defined empirical covariance"


# ---- inputs ----------------------------------------------------------------------------------------------------------
def blobs(n, d, c, salt, dtype=np.float32, spread=4.0, offset=0.0):
    """``c`` Gaussian blobs (centres ``spread`` N(0, 1), unit noise), labels ``i % c``, rounded to float32"""
    centres = spread * syn.gauss(c * d, salt).reshape(c, d)
    labels = np.arange(n) % c
    X = centres[labels] + syn.gauss(n * d, salt + 1).reshape(n, d) + offset
    return X.astype(np.float32).astype(dtype)


# name -> (N, d, K, dtype): the row chunk (2048) - 1, + 0, + 1 and three chunks; the MFMA sample stage (16) - 1, + 0,
# + 1; N = K; d at and beside the 16-feature blocks and the kernels' 16 / 32 / 64 / 128 instantiations; K up to 17
STEP_CASES = {
    "n15_d1_k1": (15, 1, 1, np.float64),
    "n16_d2_k2": (16, 2, 2, np.float32),
    "n17_d2_k3": (17, 2, 3, np.float32),
    "n33_d5_k3": (33, 5, 3, np.float64),
    "n6_d5_k6": (6, 5, 6, np.float32),
    "n17_d16_k17": (17, 16, 17, np.float64),
    "n2047_d17_k3": (2047, 17, 3, np.float32),
    "n2048_d32_k6": (2048, 32, 6, np.float64),
    "n2049_d33_k2": (2049, 33, 2, np.float32),
    "n4100_d16_k17": (4100, 16, 17, np.float32),
    "n400_d64_k2": (400, 64, 2, np.float32),
    "n400_d65_k2": (400, 65, 2, np.float64),
    "n600_d128_k2": (600, 128, 2, np.float32),
}
COV_TYPES = ("full", "diag")


def step_rows(name):
    n, d, k, dtype = STEP_CASES[name]
    return blobs(n, d, max(k, 2) if n > k else k, 9800 + n + d, dtype)


def duplicates():
    """200 rows in 5 dimensions of 3 blobs, with runs of exact copies"""
    X = blobs(200, 5, 3, 9850)
    X[[7, 33, 64]] = X[5]
    X[40:52] = X[40]
    return X


def empty_cluster_rows():
    """(rows, seeds): 12 copies of one row and a blob 20 away; two of the three seeds are copies, so the second
    cluster is empty from the first assignment on (ties go to the lowest index) and keeps its centre"""
    X = np.concatenate([np.zeros((12, 3), dtype=np.float32), blobs(40, 3, 1, 9930) + np.float32(20.0)])
    return X, np.array([0, 1, 20])


def offset_rows():
    """rows 1e3 away from the origin: X P - mu P would cancel seven digits, the direct differences do not"""
    return blobs(300, 5, 3, 9860, offset=1000.0)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def log_det(pchol, cov_type):
    diag = np.diagonal(pchol, axis1=1, axis2=2) if cov_type == "full" else pchol
    return np.cumsum(np.log(diag), axis=1)[:, -1]


def e_step(X, weights, means, pchol, cov_type):
    """(log_prob_norm [N], log_resp [N, K], resp [N, K])"""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    k = len(weights)
    lp = np.empty((n, k))
    ld = log_det(pchol, cov_type)
    with np.errstate(divide="ignore"):
        lw = np.log(weights)
    for j in range(k):
        diff = X - means[j]
        y = diff @ pchol[j] if cov_type == "full" else diff * pchol[j]
        lp[:, j] = -0.5 * (d * LOG_2PI + np.sum(y * y, axis=1)) + (ld[j] + lw[j])
    m = lp.max(axis=1)
    lpn = np.log(np.exp(lp - m[:, None]).sum(axis=1)) + m
    log_resp = lp - lpn[:, None]
    return lpn, log_resp, np.exp(log_resp)


def precision_cholesky(cov, cov_type):
    if cov_type == "diag":
        if np.any(cov <= 0.0) or not np.isfinite(cov).all():
            raise ValueError(ILL_DEFINED)
        return 1.0 / np.sqrt(cov)
    out = np.empty_like(cov)
    for j, c in enumerate(cov):
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError(ILL_DEFINED)
        out[j] = solve_triangular(L, np.eye(len(c)), lower=True).T
    return out


def means_step(X, resp):
    X = np.asarray(X, dtype=np.float64)
    nk = resp.sum(axis=0) + EPS10
    means = (resp.T @ X) / nk[:, None]
    weights = nk / len(X)
    return nk, means, weights / weights.sum()


def m_step(X, resp, reg_covar, cov_type):
    """(weights, means, covariances, precisions_cholesky)"""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    nk, means, weights = means_step(X, resp)
    k = len(nk)
    cov = np.empty((k, d, d) if cov_type == "full" else (k, d))
    for j in range(k):
        diff = X - means[j]
        if cov_type == "full":
            c = (resp[:, j] * diff.T) @ diff / nk[j]
            c = np.tril(c) + np.tril(c, -1).T
            c.flat[:: d + 1] += reg_covar
            cov[j] = c
        else:
            cov[j] = (resp[:, j][:, None] * diff * diff).sum(axis=0) / nk[j] + reg_covar
    return weights, means, cov, precision_cholesky(cov, cov_type)


def onehot(labels, k):
    resp = np.zeros((len(labels), k))
    resp[np.arange(len(labels)), labels] = 1.0
    return resp


def seeds(n, k, random_state=42):
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    return rs.choice(n, size=k, replace=False)


def kmeans(X, seed_rows, check_margin=True):
    """the package's Lloyd start: (labels, number of assignments); asserts that no row is within KMEANS_MARGIN
    (relative) of a tie between its two nearest centres (``check_margin=False``: exact ties, which go to the lowest
    index on both sides, are the point of the case)"""
    X = np.asarray(X, dtype=np.float64)
    k = len(seed_rows)
    centres = X[seed_rows].copy()
    prev = np.full(len(X), -1)
    rounds = 0
    for _ in range(KMEANS_MAX_ITER):
        d2 = ((X[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)
        labels = d2.argmin(axis=1)
        if k > 1 and check_margin:
            two = np.partition(d2, 1, axis=1)[:, :2]
            assert np.all(two[:, 1] - two[:, 0] > KMEANS_MARGIN * (two[:, 1] + 1.0)), "a k-means case is near a tie"
        rounds += 1
        if np.array_equal(labels, prev):
            break
        prev = labels
        nk, means, _ = means_step(X, onehot(labels, k))
        centres = np.where(nk[:, None] > 0.5, means, centres)
    return labels, rounds


def start(X, k, cov_type, reg_covar=1e-6, init_params="random_from_data", random_state=42):
    """the parameters an unfitted model starts from, and the start's labels (one row per component for
    'random_from_data')"""
    rows = seeds(len(X), k, random_state)
    if init_params == "kmeans":
        labels = kmeans(X, rows)[0]
        resp = onehot(labels, k)
    else:
        labels = None
        resp = np.zeros((len(X), k))
        resp[rows, np.arange(k)] = 1.0
    return m_step(X, resp, reg_covar, cov_type), labels


def fit(X, params, cov_type, tol=1e-3, reg_covar=1e-6, max_iter=100, check_margin=True):
    """sklearn's EM loop from ``params`` = (weights, means, covariances, precisions_cholesky): a dict of the fitted
    attributes.  Asserts that no iteration is within STOP_MARGIN of the stopping threshold."""
    weights, means, cov, pchol = params
    lower_bound, bounds, converged = -np.inf, [], False
    for n_iter in range(1, max_iter + 1):
        prev = lower_bound
        lpn, log_resp, resp = e_step(X, weights, means, pchol, cov_type)
        weights, means, cov, pchol = m_step(X, resp, reg_covar, cov_type)
        lower_bound = lpn.mean()
        bounds.append(lower_bound)
        change = abs(lower_bound - prev)
        if check_margin and tol > 0:
            assert abs(change - tol) > STOP_MARGIN, "a fit case is near the stopping threshold"
        if change < tol:
            converged = True
            break
    return dict(weights=weights, means=means, covariances=cov, precisions_cholesky=pchol, converged=converged,
                n_iter=n_iter, lower_bound=lower_bound, lower_bounds=np.array(bounds))


def predict(X, fitted, cov_type, margin=1e-6, near_ties=0.0):
    """labels of the fitted model; asserts a posterior margin between the two best components.  ``near_ties`` > 0: at
    most that share of the rows may be within the margin, and the mask of the other rows is returned as well."""
    _, log_resp, _ = e_step(X, fitted["weights"], fitted["means"], fitted["precisions_cholesky"], cov_type)
    clear = np.ones(len(log_resp), dtype=bool)
    if log_resp.shape[1] > 1:
        two = -np.partition(-log_resp, 1, axis=1)[:, :2]
        clear = two[:, 0] - two[:, 1] > margin
        assert np.mean(~clear) <= near_ties, "a predict case is near a tie"
    return (log_resp.argmax(axis=1), clear) if near_ties > 0.0 else log_resp.argmax(axis=1)


def n_parameters(k, d, cov_type):
    return (k * d * (d + 1) // 2 if cov_type == "full" else k * d) + d * k + k - 1


# ---- fixtures shared by the CPU and the GPU tests ------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def step_case(name, cov_type):
    """(X, params after two EM iterations from the 'random_from_data' start, the E-step there)"""
    X = step_rows(name)
    k = STEP_CASES[name][2]
    params = start(X, k, cov_type)[0]
    for _ in range(2):
        params = m_step(X, e_step(X, *params[:2], params[3], cov_type)[2], 1e-6, cov_type)
    est = e_step(X, params[0], params[1], params[3], cov_type)
    return _frozen(X, *params, *est)


@functools.lru_cache(maxsize=None)
def empty_case(cov_type):
    """three components on two blobs, the third 1e3 away in every feature: its resp is exactly 0 in every row"""
    X = blobs(300, 5, 2, 9870)
    params = list(start(X, 3, cov_type)[0])
    means = params[1].copy()
    means[2] = means[0] + 1000.0
    weights = np.array([0.5, 0.3, 0.2])
    cov = np.ones((3, 5, 5)) * np.eye(5) if cov_type == "full" else np.ones((3, 5))
    pchol = precision_cholesky(cov, cov_type)
    est = e_step(X, weights, means, pchol, cov_type)
    assert np.all(est[2][:, 2] == 0.0)
    return _frozen(X, weights, means, cov, pchol, *est)


@functools.lru_cache(maxsize=None)
def small_weight_case(cov_type):
    """two overlapping components, one with weight 0.005"""
    X = blobs(300, 5, 1, 9880)
    means = np.stack([X[:150].astype(np.float64).mean(axis=0), X[150:].astype(np.float64).mean(axis=0) + 0.5])
    weights = np.array([0.995, 0.005])
    cov = np.ones((2, 5, 5)) * np.eye(5) if cov_type == "full" else np.ones((2, 5))
    cov = cov * np.array([1.0, 2.0]).reshape((2,) + (1,) * (cov.ndim - 1))
    pchol = precision_cholesky(cov, cov_type)
    est = e_step(X, weights, means, pchol, cov_type)
    return _frozen(X, weights, means, cov, pchol, *est)


MANY_CHUNKS = 64                # from this many chunks on the chunk-sum kernel takes 4 outputs per thread instead of 1
THRESHOLD_ROWS = ((MANY_CHUNKS - 1) * CHUNK, (MANY_CHUNKS - 1) * CHUNK + 1)


@functools.lru_cache(maxsize=None)
def threshold_case(n):
    """(X [n, 65], resp [n, 17]) on either side of that threshold: K d = 1105 outputs, so both forms of the kernel run
    several slices with a ragged last one; the responsibilities are normalised hash noise"""
    X = blobs(n, 65, 3, 9960)
    resp = syn.u01(n * 17, 9961).reshape(n, 17) + 1e-3
    return _frozen(X, resp / resp.sum(axis=1, keepdims=True))


# name -> (N, d, K, dtype) at the library's limits K <= 64, d <= 128: the fourth pass of the 'diag' E-step's component
# loop (K = 25); K d below, at and above one 256-output slice of the chunk-sum kernel with K = 64; eight feature blocks of
# which three are empty (d = 65) under 33 components; one below both limits with three chunks and a ragged last slice;
# the corner itself (32 slices, 3 x 64 covariance partials of 128 x 128) as float32 and as float64 rows
LIMIT_CASES = {
    "k25_d3": (600, 3, 25, np.float64),
    "k64_d1": (300, 1, 64, np.float32),
    "k64_d4": (2049, 4, 64, np.float32),
    "k33_d65": (2049, 65, 33, np.float64),
    "k63_d127": (4100, 127, 63, np.float32),
    "k64_d128": (4100, 128, 64, np.float32),
    "k64_d128_f64": (4100, 128, 64, np.float64),
}
# name -> (salt, spread of the blob centres): small spreads, so that the components overlap and the E-step is no one-hot
# exercise (tests/test_cpu_gmm.py holds the share of soft rows and the conditioning)
LIMIT_ROWS = {
    "k25_d3": (10100, 0.25),
    "k64_d1": (10110, 0.25),
    "k64_d4": (10120, 0.25),
    "k33_d65": (10130, 0.2),
    "k63_d127": (10140, 0.2),
    "k64_d128": (10150, 0.2),
    "k64_d128_f64": (10150, 0.2),
}
LIMIT_GOLDEN = ("k63_d127", "k64_d128")        # the device against sklearn's values (the CPU test takes every case)
LIMIT_QUANTITIES = ("m_weights", "m_means_k", "m_means_j", "m_var_k", "m_var_j", "m_log_det")


def limit_key(name, cov_type):
    """the key of a limit case in tests/golden/gmm.npz: the float64 copy of the corner shares the float32 one's"""
    return "limit_%s_%s_" % (name[:-4] if name.endswith("_f64") else name, cov_type)


def limit_reduced(weights, means, cov, pchol, cov_type):
    """what tests/golden/gmm.npz keeps of an M-step at the limits, where the covariances alone are 8 MB: the weights,
    log det P_k, and the sums over the features and over the components of the means and of the variances (the
    covariances' diagonals), in the order of LIMIT_QUANTITIES.  One wrong entry (k, j) moves the sums k and j."""
    var = np.diagonal(cov, axis1=1, axis2=2) if cov_type == "full" else cov
    return (weights, means.sum(axis=1), means.sum(axis=0), var.sum(axis=1), var.sum(axis=0), log_det(pchol, cov_type))


@functools.lru_cache(maxsize=None)
def limit_resp(name):
    """the M-step input of a limit case: normalised hash noise [N, K], every component owning a share of every row (at
    fitted responsibilities a component of the corner would own fewer rows than it has features)"""
    n, _, k, _ = LIMIT_CASES[name]
    resp = syn.u01(n * k, LIMIT_ROWS[name][0] + 4).reshape(n, k) + 1e-3
    return _frozen(resp / resp.sum(axis=1, keepdims=True))[0]


@functools.lru_cache(maxsize=None)
def limit_case(name, cov_type):
    """(X, weights, means, covariances, precisions_cholesky, the E-step there) with explicit parameters: blob-wise means,
    hash weights in [0.5, 1.5) / sum and covariances I + A A^T / 8 (A: d x 4 normals; 'diag': 1 + mean(A^2) / 2).
    Parameters fitted at these sizes overfit their own rows and leave a one-hot E-step; these do not."""
    n, d, k, dtype = LIMIT_CASES[name]
    salt, spread = LIMIT_ROWS[name]
    X = blobs(n, d, k, salt, dtype, spread=spread)
    X64 = X.astype(np.float64)
    means = np.stack([X64[j::k].mean(axis=0) for j in range(k)])
    weights = syn.u01(k, salt + 2) + 0.5
    weights = weights / weights.sum()
    A = syn.gauss(k * d * 4, salt + 3).reshape(k, d, 4)
    if cov_type == "full":
        cov = np.eye(d) + 0.5 * (A @ np.swapaxes(A, 1, 2)) / 4.0
    else:
        cov = 1.0 + 0.5 * (A * A).mean(axis=2)
    pchol = precision_cholesky(cov, cov_type)
    est = e_step(X, weights, means, pchol, cov_type)
    return _frozen(X, weights, means, cov, pchol, *est)


def limit_m_case(name, cov_type):
    """the limit case with the M-step's input (``limit_resp``) in the place of the E-step's responsibilities"""
    return limit_case(name, cov_type)[:7] + (limit_resp(name),)


SPECIAL_ROWS = {"duplicates": duplicates, "offset": offset_rows}


@functools.lru_cache(maxsize=None)
def special_case(name, cov_type):
    X = SPECIAL_ROWS[name]()
    params = start(X, 3, cov_type)[0]
    for _ in range(2):
        params = m_step(X, e_step(X, *params[:2], params[3], cov_type)[2], 1e-6, cov_type)
    est = e_step(X, params[0], params[1], params[3], cov_type)
    return _frozen(X, *params, *est)


# the fit at the limit of 64 components: 60 rows per blob in two chunks, K d = 320 outputs of the chunk sums (two slices,
# the second ragged).  Rows and salt are chosen on the CPU: the 64 seeds leave 20 blobs without one and put up to four
# into one blob; with these the k-means start ends after 17 assignments and its smallest cluster still has 15 rows for a
# 5 x 5 covariance (tests/test_cpu_gmm.py holds cond < 1e3 for the fitted covariances)
K64_ROWS, K64_SALT = 3840, 10250

# whole fits: name -> (rows, K)
FIT_ROWS = {
    "blobs300": lambda: (blobs(300, 5, 3, 9900), 3),
    "chunks2100": lambda: (blobs(2100, 17, 4, 9910), 4),
    "offset300": lambda: (offset_rows(), 3),
    "k64_d5": lambda: (blobs(K64_ROWS, 5, 64, K64_SALT), 64),
}
FIT_RUNS = (("tol0_1", 0.0, 1), ("tol0_20", 0.0, 20), ("tol0_100", 0.0, 100), ("tol1e-3", 1e-3, 100))
FIT_INITS = ("explicit", "random_from_data", "kmeans")
FIT_QUANTITIES = ("weights", "means", "covariances", "precisions_cholesky", "lower_bound")
# (rows, covariance type, init, run): every init and run on the small case; the first step after a 'random_from_data'
# start on rows far from the origin (variances = reg_covar: sklearn's 'diag' expansion is at its worst there); several
# chunks from an explicit and from the k-means start; the same at the limit of 64 components (two chunks)
FIT_CASES = [("blobs300", c, i, r[0]) for c in COV_TYPES for i in FIT_INITS for r in FIT_RUNS] + \
            [("offset300", c, "random_from_data", r) for c in COV_TYPES for r in ("tol0_1", "tol1e-3")] + \
            [("chunks2100", c, i, r) for c in COV_TYPES for i in ("explicit", "kmeans") for r in ("tol0_20", "tol1e-3")] + \
            [("k64_d5", c, i, r) for c in COV_TYPES for i in ("explicit", "kmeans") for r in ("tol0_20", "tol1e-3")]


def fit_id(case):
    return "-".join(case)


def explicit_init(X, k, cov_type):
    """the explicit ``*_init`` arrays of a fit case: blob-wise means of the first max(60, 4 K) rows, unit precisions"""
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[1]
    means = np.stack([X[j:max(60, 4 * k):k].mean(axis=0) for j in range(k)])
    weights = np.full(k, 1.0 / k)
    precisions = np.ones((k, d, d)) * np.eye(d) if cov_type == "full" else np.ones((k, d))
    return weights, means, precisions


@functools.lru_cache(maxsize=None)
def fit_start(name, cov_type, init):
    """(X, K, start parameters, start labels or None)"""
    X, k = FIT_ROWS[name]()
    if init == "explicit":
        w, mu, prec = explicit_init(X, k, cov_type)
        d = X.shape[1]
        cov = np.ones((k, d, d)) * np.eye(d) if cov_type == "full" else np.ones((k, d))
        return _frozen(X)[0], k, (w, mu, cov, precision_cholesky(cov, cov_type)), None
    params, labels = start(X, k, cov_type, init_params=init)
    return _frozen(X)[0], k, params, labels


@functools.lru_cache(maxsize=None)
def fit_case(name, cov_type, init, run):
    tol, max_iter = {r[0]: r[1:] for r in FIT_RUNS}[run]
    X, k, params, _ = fit_start(name, cov_type, init)
    return fit(X, params, cov_type, tol=tol, max_iter=max_iter)
