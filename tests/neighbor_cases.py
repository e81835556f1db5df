"""Cases of the nearest-neighbour tests (row f7) and an fp64 numpy restatement of both metrics.

``tests/golden/make_golden_neighbors.py`` writes ``neighbors.npz`` from these cases: sklearn's
``NearestNeighbors(n_neighbors=1, metric='correlation')`` for the correlation cases and the reference's latent_nn
expression ``np.argmin([euclidean(latent[i], j) for j in original_latent])`` run literally for the euclidean ones.
The inputs are regenerated from hash salts (``ava_amd.synthetic``), so the npz holds only the case parameters and the
outputs."""
import numpy as np

from ava_amd import synthetic as syn

# name -> (metric, nq, nr, d, dtype, salt, dup, flat); the euclidean cases are float64, as the latent means the reference
# searches are (scipy's euclidean computes in float32 for float32 rows)
#   dup:  reference rows r with r % 5 == 4 repeat row r - 3 (exact ties; the lower index must win)
#   flat: reference rows r with r % 9 == 7 are the constant 0.25 (zero variance: NaN correlation distances)
CASES = {
    "corr_q1_r1003_d4096_f32": ("correlation", 1, 1003, 4096, "float32", 310, 0, 0),
    "corr_q17_r63_d33_f64": ("correlation", 17, 63, 33, "float64", 320, 0, 0),
    "corr_q130_r1003_d16384_f32_dup": ("correlation", 130, 1003, 16384, "float32", 330, 1, 0),
    "corr_q17_r1_d2_f64": ("correlation", 17, 1, 2, "float64", 340, 0, 0),
    "corr_q130_r63_d4096_f64_dup_flat": ("correlation", 130, 63, 4096, "float64", 350, 1, 1),
    "corr_q17_r1003_d33_f32_flat": ("correlation", 17, 1003, 33, "float32", 360, 0, 1),
    "eucl_q1_r1003_d33_f64": ("euclidean", 1, 1003, 33, "float64", 410, 0, 0),
    "eucl_q17_r63_d2_f64": ("euclidean", 17, 63, 2, "float64", 420, 0, 0),
    "eucl_q130_r1003_d33_f64_dup": ("euclidean", 130, 1003, 33, "float64", 430, 1, 0),
    "eucl_q17_r63_d4096_f64": ("euclidean", 17, 63, 4096, "float64", 440, 0, 0),
}
METRIC_CODES = {"correlation": 0, "euclidean": 1}
DTYPE_CODES = {"float32": 0, "float64": 1}


def params_row(name):
    """the case parameters as the integer row the npz stores"""
    metric, nq, nr, d, dtype, salt, dup, flat = CASES[name]
    return np.array([METRIC_CODES[metric], nq, nr, d, DTYPE_CODES[dtype], salt, dup, flat], dtype=np.int64)


def _pick(n, n_from, salt):
    return np.minimum((syn.u01(n, salt) * n_from).astype(np.int64), n_from - 1)


def _rows(metric, n, d, salt):
    if metric == "correlation":
        # clipped log-spectrogram-like values, rescaled and shifted per row (the kernels centre each row)
        x = np.clip(1.4 * syn.u01(n * d, salt) - 0.4, 0.0, 1.0).reshape(n, d)
        return x * (0.5 + syn.u01(n, salt + 1))[:, None] + 2.0 * syn.u01(n, salt + 2)[:, None]
    return syn.gauss(n * d, salt).reshape(n, d)


def make_inputs(metric, nq, nr, d, dtype, salt, dup=0, flat=0):
    """(queries [nq, d], refs [nr, d]) in ``dtype``: every even query is a perturbed copy of a reference row"""
    refs = _rows(metric, nr, d, salt)
    if dup:
        r = np.arange(nr)
        sel = r[(r % 5 == 4) & (r >= 3)]
        refs[sel] = refs[sel - 3]
    if flat:
        refs[np.arange(nr) % 9 == 7] = 0.25
    queries = _rows(metric, nq, d, salt + 3)
    even = np.arange(0, nq, 2)
    src = _pick(len(even), nr, salt + 4)
    queries[even] = refs[src] + 0.3 * queries[even]          # never a zero-variance query
    return queries.astype(dtype), refs.astype(dtype)


def case_inputs(name):
    metric, nq, nr, d, dtype, salt, dup, flat = CASES[name]
    return make_inputs(metric, nq, nr, d, dtype, salt, dup, flat)


def distances(queries, refs, metric):
    """all distances [nq, nr] in fp64: scipy's correlation (centred cosine, cosine clipped to [-1, 1]) or euclidean"""
    Q = np.asarray(queries, dtype=np.float64)
    R = np.asarray(refs, dtype=np.float64)
    if metric == "correlation":
        Qc = Q - Q.mean(axis=1, keepdims=True)
        Rc = R - R.mean(axis=1, keepdims=True)
        den = np.sqrt(np.outer(np.einsum("ij,ij->i", Qc, Qc), np.einsum("ij,ij->i", Rc, Rc)))
        with np.errstate(invalid="ignore", divide="ignore"):
            c = (Qc @ Rc.T) / den
        return 1.0 - np.clip(c, -1.0, 1.0)
    out = np.empty((len(Q), len(R)))
    for i in range(len(Q)):
        out[i] = np.sqrt(np.einsum("ij,ij->i", R - Q[i], R - Q[i]))
    return out


def nearest_from_distances(D, metric):
    """(idx, dist) under the device's rules: lowest index on ties; correlation: NaN loses, all-NaN rows give
    (0, NaN); euclidean: the first NaN wins (np.argmin)"""
    if metric == "correlation":
        idx = np.argmin(np.where(np.isnan(D), np.inf, D), axis=1)
    else:
        idx = np.argmin(D, axis=1)
    return idx.astype(np.int64), D[np.arange(len(D)), idx]


def numpy_nearest(queries, refs, metric):
    """fp64 numpy restatement: (idx, dist, D)"""
    D = distances(queries, refs, metric)
    idx, dist = nearest_from_distances(D, metric)
    return idx, dist, D


def gap(D):
    """per row: second-best minus best distance over the non-NaN entries (inf with fewer than two)"""
    out = np.full(len(D), np.inf)
    for i, row in enumerate(D):
        s = np.sort(row[~np.isnan(row)])
        if len(s) >= 2:
            out[i] = s[1] - s[0]
    return out
