"""Cases of the nearest-neighbour tests (row f7) and an fp64 numpy restatement of both metrics.

``tests/golden/make_golden_neighbors.py`` writes ``neighbors.npz`` from these cases: sklearn's
``NearestNeighbors(n_neighbors=1, metric='correlation')`` for the correlation cases and the reference's latent_nn
expression ``np.argmin([euclidean(latent[i], j) for j in original_latent])`` run literally for the euclidean ones.
The inputs are regenerated from hash salts (``ava_amd.synthetic``), so the npz holds only the case parameters and the
outputs.

``EDGE_CASES`` (below) are the cases at the kernels' tile, stage and reduce edges; the restatement is their reference and
nothing of them is in the npz."""
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


# ---- edge cases: tile, stage and reduce edges of csrc/neighbors.hip --------------------------------------------------
# Nothing of these is stored in the golden: the restatement above is the reference.  TILE is the kernels' reference
# tile (NC_BR, SQD_T: one partial per query and tile), QTILE the query tile; nn_reduce_kernel folds 64 tiles per pass.
TILE = {"correlation": 128, "euclidean": 64}
QTILE = {"correlation": 128, "euclidean": 64}

# name -> (group, metric, builder, arguments); edge_case(name) builds it
EDGE_CASES = {}
NEAR_CONSTANT = "edge_corr_near_constant_d4096"


def _edge(name, group, metric, builder, *args):
    assert name not in EDGE_CASES and name not in CASES, name
    EDGE_CASES[name] = (group, metric, builder, args)


def _as(x, dtype):
    """``x`` rounded to ``dtype``, back in fp64: copies and mirrors are derived from the values as they are stored"""
    return np.asarray(x, dtype=dtype).astype(np.float64)


def _case(metric, queries, refs, dtype, **marks):
    """marks: ties [(query, low, high)] bit-identical references low < high that are the query's nearest; same [query]:
    bit-identical to a reference; mirror [query]: the centred mirror image of the one reference; winners: the planted
    reference of every query"""
    out = dict(metric=metric, q=np.ascontiguousarray(queries.astype(dtype)), r=np.ascontiguousarray(refs.astype(dtype)),
               ties=[], same=[], mirror=[], winners=None)
    out.update(marks)
    return out


def _near(metric, refs, src, salt, eps):
    """one query per entry of ``src``: that reference row plus ``eps`` times a row of its own"""
    return refs[np.asarray(src)] + eps * _rows(metric, len(src), refs.shape[1], salt)


def _build_tile(metric, nq, nr, d, dtype, salt):
    """query i is planted on reference (nr - 1 - 7 i) % nr: the last row, alone in a trailing tile, decides query 0"""
    refs = _as(_rows(metric, nr, d, salt), dtype)
    return _case(metric, _near(metric, refs, (nr - 1 - 7 * np.arange(nq)) % nr, salt + 3, 0.1), refs, dtype)


def position_permutation(n, tile):
    """p with p([0, tile)) = [0, tile) and p([tile, n)) = [tile, n), both by an odd multiplier: neighbouring queries
    get winners in different 16-row blocks and different halves of the tile"""
    i = np.arange(n)
    return np.where(i < tile, (37 * i + 11) % tile, tile + (37 * (i - tile) + 5) % (n - tile))


def _build_position(metric, n, d, dtype, salt):
    refs = _as(_rows(metric, n, d, salt), dtype)
    p = position_permutation(n, TILE[metric])
    return _case(metric, _near(metric, refs, p, salt + 3, 0.02), refs, dtype, winners=p)


def _build_tie(metric, nr, d, low, high, dtype, salt):
    """reference ``high`` repeats ``low``; three queries near that row and one bit-identical to it"""
    refs = _as(_rows(metric, nr, d, salt), dtype)
    refs[high] = refs[low]
    queries = _near(metric, refs, [low] * 4, salt + 3, 0.02)
    queries[3] = refs[low]
    return _case(metric, queries, refs, dtype, ties=[(i, low, high) for i in range(4)], same=[3],
                 winners=np.full(4, low))


def _build_reduce(metric, nr, rows, dup, spoil, dtype, salt):
    """five queries planted on the reference rows ``rows``; dup (low, high): row high repeats row low; spoil: rows made
    NaN in one element (euclidean: the first of them wins every query) or constant (correlation: they lose)"""
    d = 5 if metric == "correlation" else 3
    # normal rows under both metrics: with d = 5 the clipped pattern leaves rows of a single non-zero element, which
    # all correlate exactly
    refs = _as(_rows("euclidean", nr, d, salt), dtype)
    ties = []
    if dup is not None:
        refs[dup[1]] = refs[dup[0]]
        ties = [(i, dup[0], dup[1]) for i, row in enumerate(rows) if row == dup[0]]
    queries = _near("euclidean", refs, rows, salt + 3, 1e-3)
    winners = np.array(rows)
    for k, row in enumerate(spoil):
        if metric == "correlation":
            refs[row] = 0.25
        else:
            refs[row, k % d] = np.nan
    if spoil:
        ties = []
        winners = np.full(len(rows), min(spoil)) if metric == "euclidean" else None
    return _case(metric, queries, refs, dtype, ties=ties, winners=winners)


def _build_near_constant(nq, nr, d, salt):
    """rows 1e6 + 1e-3 (the usual clipped pattern): a large mean and a small variation"""
    q, r = make_inputs("correlation", nq, nr, d, "float64", salt)
    return _case("correlation", 1e6 + 1e-3 * q, 1e6 + 1e-3 * r, "float64")


def _build_same(metric, nq, nr, d, dtype, salt):
    """every query is bit-identical to a reference"""
    refs = _as(_rows(metric, nr, d, salt), dtype)
    src = (nr - 1 - 7 * np.arange(nq)) % nr
    return _case(metric, refs[src], refs, dtype, same=list(range(nq)), winners=src)


def _build_mirror(nq, d, dtype, salt):
    """one reference r; query 0 is 2 mean(r) - r, the others b - a (r - mean(r)) with a > 0: correlation -1 with r"""
    ref = _as(_rows("correlation", 1, d, salt), dtype)
    c = ref[0] - ref[0].mean()
    a = 0.5 + syn.u01(nq, salt + 3)
    b = ref[0].mean() + 2.0 * syn.u01(nq, salt + 4)
    a[0], b[0] = 1.0, ref[0].mean()
    return _case("correlation", b[:, None] - a[:, None] * c[None, :], ref, dtype, mirror=list(range(nq)),
                 winners=np.zeros(nq, dtype=np.int64))


def _build_nan_query(nq, nr, d, dtype, salt):
    """query 1 has one NaN element: all its correlation distances are NaN"""
    case = _build_tile("correlation", nq, nr, d, dtype, salt)
    case["q"][1, d // 3] = np.nan
    return case


def _register():
    E, C = "euclidean", "correlation"
    # tile edges: every listed nq, nr and d appears; the corners (65, 65, 33) and (129, 129, 17) in both dtypes
    for k, (nq, nr, d, dtype) in enumerate([
            (63, 63, 1, "float64"), (64, 64, 31, "float32"), (65, 65, 33, "float64"), (65, 65, 33, "float32"),
            (63, 64, 32, "float64"), (64, 65, 65, "float64"), (65, 63, 32, "float32"), (63, 65, 31, "float64"),
            (64, 63, 65, "float32"), (65, 64, 1, "float32"), (1, 65, 33, "float64"), (65, 1, 31, "float32")]):
        _edge("edge_eucl_q%d_r%d_d%d_%s" % (nq, nr, d, dtype[0] + dtype[-2:]), "tile", E, _build_tile, E, nq, nr, d,
              dtype, 1000 + 10 * k)
    for k, (nq, nr, d, dtype) in enumerate([
            (127, 127, 15, "float64"), (128, 128, 16, "float32"), (129, 129, 17, "float64"), (129, 129, 17, "float32"),
            (127, 128, 33, "float32"), (128, 129, 15, "float64"), (129, 127, 16, "float64"), (127, 129, 16, "float32"),
            (128, 127, 17, "float64"), (129, 128, 33, "float64"), (1, 129, 17, "float32"), (129, 1, 2, "float64")]):
        _edge("edge_corr_q%d_r%d_d%d_%s" % (nq, nr, d, dtype[0] + dtype[-2:]), "tile", C, _build_tile, C, nq, nr, d,
              dtype, 1200 + 10 * k)
    # d = 1 under correlation: every row has zero variance, every distance is NaN, every index 0
    _edge("edge_corr_d1_all_nan", "d1", C, _build_tile, C, 5, 130, 1, "float64", 1400)
    # every position of a tile decides
    _edge("edge_corr_position_257_d17", "position", C, _build_position, C, 257, 17, "float64", 1410)
    _edge("edge_eucl_position_129_d33", "position", E, _build_position, E, 129, 33, "float64", 1420)
    # planted ties
    _edge("edge_corr_tie_10_70_halves", "tie", C, _build_tie, C, 129, 17, 10, 70, "float64", 1430)
    _edge("edge_eucl_tie_3_19_thread", "tie", E, _build_tie, E, 65, 33, 3, 19, "float64", 1440)
    _edge("edge_eucl_tie_3_4_lanes", "tie", E, _build_tie, E, 65, 33, 3, 4, "float32", 1450)
    _edge("edge_corr_tie_10_198_tiles", "tie", C, _build_tie, C, 257, 17, 10, 198, "float32", 1460)
    _edge("edge_eucl_tie_5_69_tiles", "tie", E, _build_tie, E, 130, 33, 5, 69, "float64", 1470)
    # the reduce's second and third pass.  With 65 tiles the 65th holds the last row alone, so the winner in tile 64,
    # the winner in the last row and the duplicate of a row of tile 0 in tile 64 cannot share one run: the "dup" runs
    # plant the duplicate, the plain ones the winner.  With 129 tiles of 64 one run holds them all.
    e65 = [17, 63 * 64 + 40, 4096, 64 + 3, 32 * 64 + 63]                 # tile 0, tile 63, tile 64 = the last row
    e129 = [17, 63 * 64 + 40, 64 * 64 + 9, 8192, 29]                     # tile 0, 63, 64, the last row (tile 128)
    c65 = [17, 63 * 128 + 40, 8192, 128 + 3, 32 * 128 + 127]
    _edge("edge_eucl_reduce_r4097", "reduce", E, _build_reduce, E, 4097, e65, None, [], "float64", 1500)
    _edge("edge_eucl_reduce_r4097_dup", "reduce", E, _build_reduce, E, 4097, [17, 63 * 64 + 40, 29, 29, 29],
          (29, 4096), [], "float64", 1500)
    _edge("edge_eucl_reduce_r4097_nan", "reduce", E, _build_reduce, E, 4097, e65, None, [4096, 2 * 64 + 5], "float64",
          1500)
    _edge("edge_eucl_reduce_r4097_nan64", "reduce", E, _build_reduce, E, 4097, e65, None, [4096], "float64", 1500)
    _edge("edge_eucl_reduce_r8193", "reduce", E, _build_reduce, E, 8193, e129, (29, 64 * 64 + 50), [], "float32", 1510)
    _edge("edge_eucl_reduce_r8193_nan", "reduce", E, _build_reduce, E, 8193, e129, None, [64 * 64 + 7, 2 * 64 + 5],
          "float32", 1510)
    _edge("edge_corr_reduce_r8193", "reduce", C, _build_reduce, C, 8193, c65, None, [], "float64", 1520)
    _edge("edge_corr_reduce_r8193_dup", "reduce", C, _build_reduce, C, 8193, [17, 63 * 128 + 40, 29, 29, 29],
          (29, 8192), [], "float32", 1520)
    _edge("edge_corr_reduce_r8193_flat", "reduce", C, _build_reduce, C, 8193, c65, None, [8192, 2 * 128 + 5], "float64",
          1520)
    # near-constant rows
    _edge(NEAR_CONSTANT, "near_constant", C, _build_near_constant, 9, 130, 4096, 1600)
    # the clip
    _edge("edge_corr_same_d33_f64", "clip", C, _build_same, C, 9, 130, 33, "float64", 1610)
    _edge("edge_corr_same_d4096_f32", "clip", C, _build_same, C, 9, 130, 4096, "float32", 1620)
    _edge("edge_eucl_same_d33_f64", "clip", E, _build_same, E, 9, 130, 33, "float64", 1630)
    _edge("edge_corr_mirror_d17_f64", "clip", C, _build_mirror, 9, 17, "float64", 1640)
    _edge("edge_corr_mirror_d4096_f32", "clip", C, _build_mirror, 9, 4096, "float32", 1650)
    _edge("edge_corr_nan_query", "clip", C, _build_nan_query, 3, 130, 17, "float64", 1660)


_register()
_built = {}


def edge_case(name):
    """the case as a dict: group, metric, q, r, the marks of _case, and the restatement's D, idx, dist and gap.  Built
    once and shared: callers leave it unchanged."""
    if name not in _built:
        group, metric, builder, args = EDGE_CASES[name]
        case = builder(*args)
        assert case["metric"] == metric
        case["group"] = group
        case["idx"], case["dist"], case["D"] = numpy_nearest(case["q"], case["r"], metric)
        case["gap"] = gap(case["D"])
        for a in ("idx", "dist", "D", "gap"):           # q and r stay writable: torch.from_numpy takes them as they are
            case[a].setflags(write=False)
        _built[name] = case
    return _built[name]


def third_gap(D):
    """per row: third-best minus best distance over the non-NaN entries (inf with fewer than three)"""
    out = np.full(len(D), np.inf)
    for i, row in enumerate(D):
        s = np.sort(row[~np.isnan(row)])
        if len(s) >= 3:
            out[i] = s[2] - s[0]
    return out


def distances_longdouble(queries, refs):
    """the correlation formulas of distances() in np.longdouble (the inputs are exact there)"""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here"
    Q = np.asarray(queries, dtype=np.longdouble)
    R = np.asarray(refs, dtype=np.longdouble)
    Qc = Q - Q.mean(axis=1, keepdims=True)
    Rc = R - R.mean(axis=1, keepdims=True)
    den = np.sqrt(np.outer(np.einsum("ij,ij->i", Qc, Qc), np.einsum("ij,ij->i", Rc, Rc)))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (Qc @ Rc.T) / den
    return np.longdouble(1.0) - np.clip(c, np.longdouble(-1.0), np.longdouble(1.0))


def near_constant_floor():
    """(floor, DL): DL the longdouble distances of the near-constant case, floor = max |fp64 restatement - DL|, the
    error an fp64 evaluation of these formulas makes on these rows"""
    if "floor" not in _built:
        case = edge_case(NEAR_CONSTANT)
        DL = distances_longdouble(case["q"], case["r"])
        _built["floor"] = (float(np.max(np.abs(case["D"].astype(np.longdouble) - DL))), DL)
    return _built["floor"]


def nn_better(d1, i1, d2, i2, nan_wins):
    """nn_better of neighbors.hip: True when candidate (d1, i1) beats (d2, i2); an empty candidate (index < 0) loses
    to everything"""
    if i2 < 0:
        return i1 >= 0
    if i1 < 0:
        return False
    n1, n2 = bool(np.isnan(d1)), bool(np.isnan(d2))
    if n1 != n2:
        return n1 if nan_wins else n2
    if not n1 and d1 != d2:
        return bool(d1 < d2)
    return i1 < i2


def merge(best_idx, best_dist, idx, dist, offset, nan_wins):
    """nn_merge_kernel restated: (best_idx, best_dist) after the candidates (idx + offset, dist) met them"""
    out_i, out_d = np.array(best_idx, dtype=np.int64), np.array(best_dist, dtype=np.float64)
    for k in range(len(out_i)):
        if nn_better(dist[k], int(idx[k]) + offset, out_d[k], int(out_i[k]), nan_wins):
            out_i[k], out_d[k] = int(idx[k]) + offset, dist[k]
    return out_i, out_d
