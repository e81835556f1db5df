"""The numpy restatement of the definitions of ``ava_amd/embedding_quality.py`` / ``include/ava_embed_quality.h`` and the
deterministic cases of its tests and of ``tests/golden/make_golden_embed_quality.py``.

For n rows in two spaces the restatement forms the fp64 squared distances by direct differences with the features
ascending, orders every row's other rows by ``lexsort`` on (distance, index), and reads ranks, neighbour sets, penalties
and overlaps off that order.  numpy has no fused multiply-add, so a distance differs from the device's by the rounding
of its products, a relative 2^-53 per feature: the random cases keep consecutive sorted distances ``MIN_GAP`` apart
(``min_gap`` measures it), the tie cases have distances that both sides form exactly or bit for bit alike.
"""
import numpy as np

MIN_GAP = 1e-11           # least relative gap of consecutive sorted distances of a row, in the random cases

# (n, d, k, seed) of the golden file
GOLDEN_CASES = [(65, 3, 5, 0), (129, 33, 12, 1), (300, 32, 63, 2), (1500, 32, 30, 3), (2049, 8, 5, 4)]
GOLDEN_RANK_TABLES = 2    # the first cases store their rank tables too

# the kernel's edges: the 64-row tile, the 32-column stage
RANK_N = [63, 64, 65, 129, 257]
RANK_D = [1, 2, 31, 32, 33, 65]
RANK_M = [1, 5, 63]
COL_SPLITS = [1, 2, 7, 0]


def sqd(X):
    """[n, n] squared distances of the rows of X: direct differences, features ascending"""
    X = np.asarray(X, dtype=np.float64)
    acc = np.zeros((len(X), len(X)), dtype=np.float64)
    for j in range(X.shape[1]):
        df = X[:, j:j + 1] - X[None, :, j]
        acc += df * df
    return acc


def order(D2):
    """[n, n - 1]: every row's other rows by (distance, index)"""
    n = len(D2)
    out = np.empty((n, n - 1), dtype=np.int64)
    idx = np.arange(n)
    for i in range(n):
        o = np.lexsort((idx, D2[i]))
        out[i] = o[o != i]
    return out


def ranks_of(order_):
    """[n, n]: rank[i, j] = 1 + the place of j in row i's order; 0 on the diagonal"""
    n = len(order_)
    r = np.zeros((n, n), dtype=np.int64)
    r[np.arange(n)[:, None], order_] = np.arange(1, n)[None, :]
    return r


def brute_rank(D2, i, j):
    """the definition, pair by pair"""
    c = 1
    for l in range(len(D2)):
        if l != i and (D2[i, l] < D2[i, j] or (D2[i, l] == D2[i, j] and l < j)):
            c += 1
    return c


def min_gap(D2):
    """the least relative gap between consecutive sorted distances of any row (the row itself left out)"""
    n = len(D2)
    s = np.sort(D2 + np.diag(np.full(n, np.inf)), axis=1)[:, :n - 1]
    return float(np.min((s[:, 1:] - s[:, :-1]) / s[:, 1:]))


def target_ranks(X, tgt):
    """[n, m] int32: the rank in X of every target"""
    r = ranks_of(order(sqd(X)))
    return r[np.arange(len(r))[:, None], np.asarray(tgt)].astype(np.int32)


def penalties(rank, ks):
    """(pen [n, n_k] int64, totals [n_k] int64) of a rank table"""
    rank = np.asarray(rank, dtype=np.int64)
    pen = np.stack([np.maximum(rank[:, :k] - k, 0).sum(axis=1) for k in ks], axis=1)
    return pen, pen.sum(axis=0)


def overlaps(A, B, ks):
    """(overlap [n, n_k] int32, totals [n_k] int64) of two neighbour tables: matching slot pairs below k"""
    A, B = np.asarray(A), np.asarray(B)
    ov = np.stack([((A[:, :k, None] == B[:, None, :k]) & (A[:, :k, None] >= 0)).sum(axis=(1, 2)) for k in ks], axis=1)
    return ov.astype(np.int32), ov.sum(axis=0).astype(np.int64)


def scalar(t, n, k):
    """sklearn's expression, from the exact integer"""
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


class Pair:
    """everything the definitions give for rows in two spaces, up to neighbourhood size ``m``"""

    def __init__(self, X, Y, m):
        self.n, self.m = len(X), m
        self.ox, self.oy = order(sqd(X)), order(sqd(Y))
        self.nx, self.ny = self.ox[:, :m], self.oy[:, :m]             # N_m^X, N_m^Y in the order
        rx, ry = ranks_of(self.ox), ranks_of(self.oy)
        rows = np.arange(self.n)[:, None]
        self.rank_x = rx[rows, self.ny].astype(np.int32)              # ranks in X of the neighbours in Y
        self.rank_y = ry[rows, self.nx].astype(np.int32)

    def curve(self, ks):
        n = self.n
        pt, tt = penalties(self.rank_x, ks)
        pc, tc = penalties(self.rank_y, ks)
        ov, to = overlaps(self.nx, self.ny, ks)
        ks = np.asarray(ks)
        q = np.array([int(t) / (n * int(k)) for t, k in zip(to, ks)])
        return {"trustworthiness": np.array([scalar(int(t), n, int(k)) for t, k in zip(tt, ks)]),
                "continuity": np.array([scalar(int(t), n, int(k)) for t, k in zip(tc, ks)]),
                "preservation": q, "lcmc": q - ks / (n - 1.0),
                "penalty_t": tt, "penalty_c": tc, "pen_t": pt, "pen_c": pc, "overlap": ov}

    def local(self, k):
        c = self.curve([k])
        f = 2.0 / (k * (2.0 * self.n - 3.0 * k - 1.0))
        return {"trustworthiness": 1.0 - c["pen_t"][:, 0] * f, "continuity": 1.0 - c["pen_c"][:, 0] * f,
                "overlap": c["overlap"][:, 0]}


def golden_x(n, d, seed):
    """(the RandomState after X, X): the golden generator draws Y's noise from the same stream"""
    rs = np.random.RandomState(seed)
    return rs, rs.standard_normal((n, d))


def rows(n, d, seed):
    return np.random.RandomState(1000 + seed).standard_normal((n, d))


def far_targets(X, m):
    """targets that are no neighbours: slot 0 the farthest row, slot 1 (if any) a repeat of it, the rest rows spread
    over the whole order"""
    o = order(sqd(X))
    n = len(o)
    cols = np.linspace(n - 2, 0, m).round().astype(np.int64)
    t = o[:, cols]
    if m > 1:
        t[:, 1] = t[:, 0]
    return t


def twins(n, d, seed):
    """every row stored twice: row i and row n + i are equal"""
    X = rows(n, d, seed)
    return np.concatenate([X, X])


def grid():
    """the 75 points of a 5 x 5 x 3 integer grid, in a shuffled order: every distance is a small integer"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    return g[np.random.RandomState(7).permutation(len(g))].astype(np.float64)


def all_others(n):
    """[n, n - 1]: every other row as a target, ascending"""
    return np.array([[j for j in range(n) if j != i] for i in range(n)], dtype=np.int64)
