"""Cases and a numpy restatement for the spectral row (f27): graphs, their dense spectra, the operator in extended
precision, and thick-restart Lanczos with the null space locked from the components, the counter-based start vector and
the restart rule of ``ava_amd.spectral``, written out again in numpy (sums in numpy's order, so it agrees with the
device to rounding, not to the bit)."""
from fractions import Fraction

import numpy as np
import scipy.sparse
from scipy.sparse.csgraph import connected_components as _scipy_components

from ava_amd import synthetic as syn

BREAKDOWN = 1e-12
U = 2.0 ** -52
MIN_GAP = 1e-3

# (n, centres, std, seed): blobs in 8 dimensions whose 10-neighbour graph sklearn clusters with ARI 1.0
BLOB_CASES = [(96, 2, 1.0, 0), (300, 4, 1.0, 0), (600, 3, 2.5, 6)]
BLOB_K = 10
BLOB_DIM = 8
RINGS = (400, 10, 0)                       # n, k, seed
# (name, n_components) of the graphs whose sklearn SpectralEmbedding is in tests/golden/spectral.npz
EMBED_CASES = [("blobs0", 3), ("blobs1", 5), ("blobs2", 4), ("gauss", 3), ("wring", 3)]
WRING = (257, 1)                           # n, seed of the weighted ring with chords
GAUSS = (2000, 8, 10, 0)                   # n, d, k, seed


# ---- rows and graphs ---------------------------------------------------------------------------------------------------
def blobs(n, centres, std, seed, d=BLOB_DIM):
    """(X float64 [n, d], truth [n]): ``centres`` gaussian blobs of equal share, centres uniform in [-10, 10]"""
    rs = np.random.RandomState(1000 + seed)
    mu = rs.uniform(-10.0, 10.0, size=(centres, d))
    y = np.arange(n) % centres
    return mu[y] + std * rs.normal(size=(n, d)), y


def rings(n, seed):
    """(X float64 [n, 2], truth): two concentric rings of radii 1 and 3 with a little noise, interleaved"""
    rs = np.random.RandomState(2000 + seed)
    y = np.arange(n) % 2
    t = rs.uniform(0.0, 2.0 * np.pi, size=n)
    r = np.where(y == 0, 1.0, 3.0) + 0.05 * rs.normal(size=n)
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=1), y


def gauss_rows(n, d, seed):
    return np.random.RandomState(3000 + seed).normal(size=(n, d))


def knn_table(X, k):
    """[n, k] the k nearest rows of every row, itself first, by (squared distance, index)"""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty((len(X), k), dtype=np.int64)
    for a in range(0, len(X), 512):
        d2 = ((X[a:a + 512, None, :] - X[None, :, :]) ** 2).sum(-1)
        d2[np.arange(len(d2)), a + np.arange(len(d2))] = -1.0
        out[a:a + 512] = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return out


def knn_affinity(X, k):
    """sklearn's ``kneighbors_graph(include_self=True)`` followed by ``0.5 (C + C^T)``"""
    idx = knn_table(X, k)
    n = len(idx)
    C = scipy.sparse.csr_matrix((np.ones(idx.size), (np.repeat(np.arange(n), k), idx.ravel())), shape=(n, n))
    A = scipy.sparse.csr_matrix(0.5 * (C + C.T))
    A.sort_indices()
    return A


def case_rows(name):
    if name.startswith("blobs"):
        n, c, std, seed = BLOB_CASES[int(name[5:])]
        return blobs(n, c, std, seed)
    if name == "rings":
        return rings(RINGS[0], RINGS[2])
    if name == "gauss":
        return gauss_rows(GAUSS[0], GAUSS[1], GAUSS[3]), None
    raise KeyError(name)


_GRAPHS = {}


def case_graph(name):
    """the affinity graph of a named case, made once"""
    if name not in _GRAPHS and name == "wring":
        _GRAPHS[name] = weighted_ring(*WRING)
    if name not in _GRAPHS:
        X, _ = case_rows(name)
        k = RINGS[1] if name == "rings" else GAUSS[2] if name == "gauss" else BLOB_K
        _GRAPHS[name] = knn_affinity(X, k)
    return _GRAPHS[name]


def csr(n, rows, cols, vals):
    A = scipy.sparse.csr_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def symmetric(n, edges, w=None):
    """the symmetric graph of the edge list ``edges`` [(i, j)], weights ``w`` (default 1)"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(e)) if w is None else np.asarray(w, dtype=np.float64)
    return csr(n, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), np.concatenate([w, w]))


def path_graph(n):
    return symmetric(n, [(i, i + 1) for i in range(n - 1)])


def cliques_and_isolated(a, b, iso):
    """a clique of ``a`` rows, ``iso`` isolated rows, a clique of ``b`` rows"""
    e = [(i, j) for i in range(a) for j in range(i + 1, a)]
    e += [(a + iso + i, a + iso + j) for i in range(b) for j in range(i + 1, b)]
    return symmetric(a + iso + b, e)


def two_halves_last_edge(n):
    """two paths over the even and over the odd rows below n - 1, and row n - 1, which alone links them (to 0 and 1)"""
    e = [(i, i + 2) for i in range(n - 3)]
    return symmetric(n, e + [(n - 1, 0), (n - 1, 1)])


def weighted_ring(n, seed, chords=2):
    """a connected graph with random weights: a ring and ``chords n`` random chords"""
    rs = np.random.RandomState(4000 + seed)
    e = {(i, (i + 1) % n) if i < (i + 1) % n else ((i + 1) % n, i) for i in range(n)} if n > 2 else {(0, 1)}
    for _ in range(chords * n):
        i, j = sorted(rs.randint(0, n, size=2))
        if i != j:
            e.add((int(i), int(j)))
    e = sorted(e)
    return symmetric(n, e, rs.uniform(0.2, 1.0, size=len(e)))


def mixed_rows(n, seed):
    """n >= 800 rows; rows 0 .. 5 have 0, 1, 63, 64, 65 and 300 off-diagonal entries, every row up to 40 a stored
    diagonal, the others a few random links: symmetric, so later rows gain entries"""
    rs = np.random.RandomState(5000 + seed)
    e = set()
    base = 400                                      # targets of the long rows: rows beyond every short one
    for r, cnt in ((1, 1), (2, 63), (3, 64), (4, 65), (5, 300)):
        for j in rs.choice(n - base, size=cnt, replace=False):
            e.add((r, base + int(j)))
    for i in range(6, n - 1, 3):
        j = int(rs.randint(i + 1, n))
        e.add((i, j))
    e = sorted(e)
    A = symmetric(n, e, rs.uniform(0.1, 2.0, size=len(e))).tolil()
    for i in range(0, 40):
        A[i, i] = 0.75 + i
    A = scipy.sparse.csr_matrix(A)
    A.sort_indices()
    return A


# ---- definitions -------------------------------------------------------------------------------------------------------
def off_diagonal(A):
    A = scipy.sparse.csr_matrix(A, dtype=np.float64, copy=True)
    A.setdiag(0.0)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def components(A):
    """(c, labels): the components numbered in the order of their smallest row"""
    c, lab = _scipy_components(off_diagonal(A), directed=False)
    _, first = np.unique(lab, return_index=True)
    renumber = np.empty(c, dtype=np.int64)
    renumber[np.argsort(first)] = np.arange(c)
    return int(c), renumber[lab].astype(np.int32)


def row_terms(A):
    """per row the off-diagonal (columns, values)"""
    A = off_diagonal(A)
    return [(A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]) for i in range(A.shape[0])]


def degrees(A):
    """(deg, dd, bound): exact row sums rounded once, ``dd`` as scipy's laplacian sets it, and per row
    ``nnz 2^-52 sum |terms|``"""
    terms = row_terms(A)
    deg = np.array([float(sum((Fraction(float(a)) for a in v), Fraction(0))) for _, v in terms])
    bound = np.array([len(v) * U * np.abs(v).sum() for _, v in terms])
    return deg, np.where(deg == 0.0, 1.0, np.sqrt(np.where(deg == 0.0, 1.0, deg))), bound


def apply_exact(A, dd, x):
    """(y, bound): ``y[i] = (sum_j a_ij (x_j (1 / dd_j))) (1 / dd_i)`` with the factors in fp64 as the kernel forms them
    and the row sum exact, rounded once; bound as for the degrees, over the terms of y"""
    dinv = 1.0 / dd
    t = x * dinv
    y = np.zeros(len(x))
    bound = np.zeros(len(x))
    for i, (c, v) in enumerate(row_terms(A)):
        s = sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(v, t[c])), Fraction(0))
        y[i] = float(s) * dinv[i]
        bound[i] = len(v) * U * float(np.abs(v * t[c]).sum()) * dinv[i]
    return y, bound


def operator(A):
    """(M sparse, dd): ``D^-1/2 A D^-1/2`` without the diagonal"""
    A = off_diagonal(A)
    deg = np.asarray(A.sum(axis=1)).ravel()
    dd = np.where(deg == 0.0, 1.0, np.sqrt(np.where(deg == 0.0, 1.0, deg)))
    D = scipy.sparse.diags(1.0 / dd)
    return scipy.sparse.csr_matrix(D @ A @ D), dd


def laplacian(A):
    """(L_sym dense, dd): ``I - D^-1/2 A D^-1/2`` with a 0 on the diagonal of an isolated row, as scipy's ``laplacian``
    has it: a row without neighbours is a component of its own, with eigenvalue 0 and eigenvector ``e_i``"""
    M, dd = operator(A)
    isolated = np.diff(off_diagonal(A).indptr) == 0
    return np.diag(1.0 - isolated) - M.toarray(), dd


def dense_spectrum(A):
    """(lambda ascending, X columns, dd): ``numpy.linalg.eigh`` of ``L_sym``"""
    L, dd = laplacian(A)
    lam, X = np.linalg.eigh(L)
    return lam, X, dd


def residuals(A, lam, u):
    """``|L_sym x - lambda x|`` of the unit vectors ``x = u o dd`` in the columns of ``u``"""
    L, dd = laplacian(A)
    x = unit(u * dd[:, None])
    return np.linalg.norm(L @ x - x * np.asarray(lam)[None, :], axis=0)


def gaps(lam, c, k):
    """the least gap that the first ``k`` pairs of a spectrum with a ``c``-fold 0 rest on: between the last wanted
    eigenvalue and the next, and between distinct wanted eigenvalues outside the null space"""
    k = max(k, c)
    edges = lam[c - 1:k + 1] if k < len(lam) else lam[c - 1:k]
    return float(np.min(np.diff(edges))) if len(edges) > 1 else np.inf


def sign_flip(u):
    """sklearn's ``_deterministic_vector_sign_flip`` for vectors in columns"""
    big = np.argmax(np.abs(u), axis=0)
    return u * np.sign(u[big, np.arange(u.shape[1])])[None, :]


def unit(u):
    return u / np.linalg.norm(u, axis=0, keepdims=True)


def subspace_sine(Q, G):
    """the sine of the largest principal angle between span(G) and its projection on span(Q)"""
    Q, _ = np.linalg.qr(Q)
    G, _ = np.linalg.qr(G)
    return float(np.linalg.norm(G - Q @ (Q.T @ G), 2))


def is_permutation(a, b):
    """whether the contingency table of two labelings is a permutation matrix"""
    a, b = np.asarray(a), np.asarray(b)
    ka, kb = int(a.max()) + 1, int(b.max()) + 1
    if ka != kb:
        return False
    T = np.zeros((ka, kb), dtype=np.int64)
    np.add.at(T, (a, b), 1)
    return bool(((T > 0).sum(0) == 1).all() and ((T > 0).sum(1) == 1).all())


def check_eigenvalues(lam_got, lam_dense, n, tol):
    """``|lambda^ - lambda| <= |r|_2 <= tol`` for a symmetric matrix, and the rest is rounding"""
    bound = tol + 64 * n * U
    err = np.abs(np.asarray(lam_got) - lam_dense[:len(lam_got)])
    print("eigenvalue error %.3e, bound %.3e" % (err.max(), bound))
    assert err.max() <= bound


def check_embedding(name, k, lam_dense, c, u_all, golden_Y, tol):
    """``u_all`` [n, k + 1]: all pairs in sklearn's convention, none dropped; ``golden_Y`` [n, k]: sklearn's, the first
    dropped.  Davis-Kahan: a unit vector is within ``(tol + 1e-12) / gap`` of sklearn's after the sign rule; inside the
    null space of a disconnected graph sklearn's basis is arbitrary, so there the spanned subspace is compared."""
    bound = (tol + 1e-12) / gaps(lam_dense, c, k + 1)
    null_golden = min(c, k + 1) - 1                    # sklearn's columns that lie in the null space
    if null_golden > 0:
        sine = subspace_sine(u_all[:, :min(c, k + 1)], golden_Y[:, :null_golden])
        print("%s null space sine %.3e, bound %.3e" % (name, sine, bound))
        assert sine <= bound
    for col in range(null_golden, k):
        a = unit(sign_flip(u_all[:, col + 1:col + 2]))
        b = unit(sign_flip(golden_Y[:, col:col + 1]))
        err = float(np.linalg.norm(a - b))
        print("%s vector %d error %.3e, bound %.3e" % (name, col, err, bound))
        assert err <= bound


# ---- the solver, restated ----------------------------------------------------------------------------------------------
def start_vector(n, seed):
    return syn.u01(n, seed) - 0.5


def null_vectors(labels, dd, k):
    V = np.zeros((k, len(dd)))
    for c in range(k):
        V[c] = np.where(labels == c, dd, 0.0)
        V[c] /= np.linalg.norm(V[c])
    return V


def _orth_normalise(B, w):
    """two passes of classical Gram-Schmidt against the rows of B: (the summed coefficients, |w|, w / |w|)"""
    h = np.zeros(len(B))
    for _ in range(2):
        if len(B):
            g = B @ w
            w = w - B.T @ g
            h += g
    beta = float(np.linalg.norm(w))
    return h, beta, (w / beta if beta > BREAKDOWN else np.zeros_like(w))


def lanczos_steps(M, V, nlock, j0, j1, alpha, beta):
    """steps j0 .. j1 - 1 on the basis V [capacity, n] in place, as ``ava_sp_lanczos``"""
    for j in range(j0, j1):
        m = nlock + j + 1
        h, b, v = _orth_normalise(V[:m], M @ V[m - 1])
        alpha[j], beta[j], V[m] = h[m - 1], b, v


def projected_matrix(theta, s, alpha, beta, k, m):
    T = np.diag(np.concatenate([theta[:k], alpha[k:m]]))
    for i in range(k):
        T[k, i] = T[i, k] = s[i]
    for j in range(k, m - 1):
        T[j, j + 1] = T[j + 1, j] = beta[j]
    return T


class Solve:
    """thick-restart Lanczos for the ``n_components`` smallest pairs of ``L_sym``: ``lam`` ascending, ``x`` [k, n] unit
    eigenvectors (the null vectors of the components first), ``n_ops``, ``n_restarts``"""

    def __init__(self, A, n_components, tol=1e-10, ncv=None, seed=0, maxiter=5000):
        M, dd = operator(A)
        n = A.shape[0]
        c, labels = components(A)
        self.n_comp, self.labels, self.dd = c, labels, dd
        k_null = min(c, n_components)
        nwant = n_components - k_null
        self.n_ops = self.n_restarts = 0
        if nwant == 0:
            self.lam, self.x = np.zeros(k_null), null_vectors(labels, dd, k_null)
            return
        room = n - c
        ncv = max(64, 2 * nwant + 1) if ncv is None else ncv
        m = min(ncv, room)
        V = np.zeros((c + m + 1, n))
        V[:c] = null_vectors(labels, dd, c)
        _, _, V[c] = _orth_normalise(V[:c], start_vector(n, seed))
        alpha, beta = np.zeros(m), np.zeros(m)
        k, theta, s = 0, np.zeros(0), np.zeros(0)
        while True:
            lanczos_steps(M, V, c, k, m, alpha, beta)
            self.n_ops += m - k
            broke = np.nonzero(beta[k:m] <= BREAKDOWN)[0]
            exact = m == room or len(broke) > 0
            me = k + int(broke[0]) + 1 if len(broke) else m
            mu, S = np.linalg.eigh(projected_matrix(theta, s, alpha, beta, k, me))
            order = np.argsort(-mu, kind="stable")
            res = np.zeros(me) if exact else np.abs(beta[me - 1] * S[me - 1, order])
            if exact or (res[:nwant] <= tol).all():
                V[c:c + nwant] = S[:, order[:nwant]].T @ V[c:c + me]
                self.lam = np.concatenate([np.zeros(c), 1.0 - mu[order[:nwant]]])
                self.x = V[:c + nwant].copy()
                return
            if self.n_ops >= maxiter:
                raise RuntimeError("no convergence")
            kk = nwant + (me - nwant) // 2
            keep = order[:kk]
            last = V[c + me].copy()
            V[c:c + kk] = S[:, keep].T @ V[c:c + me]
            V[c + kk] = last
            theta, s, k = mu[keep], beta[me - 1] * S[me - 1, keep], kk
            self.n_restarts += 1

    def embedding(self, drop_first):
        """sklearn's convention: (eigenvalues, ``u = x / dd`` in columns, sign-fixed)"""
        first = 1 if drop_first else 0
        return self.lam[first:], sign_flip((self.x / self.dd[None, :]).T)[:, first:]


def lloyd(Y, k, iters=100):
    """a deterministic k-means for rows that form k tight groups: farthest-point seeding from row 0, then Lloyd"""
    Y = np.asarray(Y, dtype=np.float64)
    centres = [Y[0]]
    for _ in range(1, k):
        d2 = np.min(((Y[:, None, :] - np.asarray(centres)[None, :, :]) ** 2).sum(-1), axis=1)
        centres.append(Y[int(np.argmax(d2))])
    centres = np.asarray(centres)
    labels = None
    for _ in range(iters):
        new = np.argmin(((Y[:, None, :] - centres[None, :, :]) ** 2).sum(-1), axis=1)
        if labels is not None and (new == labels).all():
            break
        labels = new
        for c in range(k):
            if (labels == c).any():
                centres[c] = Y[labels == c].mean(0)
    return labels


def cluster_rows(name):
    """(X, truth, n_clusters) of a clustering case: the three blob cases and the rings"""
    X, y = case_rows(name)
    return X, y, int(y.max()) + 1


CLUSTER_CASES = ["blobs0", "blobs1", "blobs2", "rings"]
