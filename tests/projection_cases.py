"""Cases and the numpy restatement for ava_amd.projection (the UMAP / PCA projections of latent means).

Inputs come from ava_amd.synthetic's hash streams, so the same arrays are produced anywhere.  The restatement follows
the algorithm of the device path step by step (umap-learn 0.5 semantics with this package's deviations, and sklearn
1.7's covariance_eigh PCA); it is the oracle of the GPU tests.  Sums run in the device's order where the order shows
at the tolerances the tests use.
"""
import numpy as np
import scipy.sparse

from ava_amd import synthetic as syn

MAX_NEG = 16


# ---- inputs ----------------------------------------------------------------------------------------------------------
def blobs(n=1500, d=32, c=6, salt=9100):
    """``c`` Gaussian blobs (centres 4 N(0, 1), unit noise), labels ``i % c``: (float32 [n, d], labels)"""
    centres = 4.0 * syn.gauss(c * d, salt).reshape(c, d)
    labels = np.arange(n) % c
    X = centres[labels] + syn.gauss(n * d, salt + 1).reshape(n, d)
    return X.astype(np.float32), labels


def spiral(n=1500, d=32, salt=9200):
    """a noisy 3-D spiral embedded in ``d`` dimensions: (float32 [n, d], curve parameter t)"""
    t = np.sort(syn.u01(n, salt) * 4 * np.pi)
    Q = np.linalg.qr(syn.gauss(d * 3, salt + 1).reshape(d, 3))[0]
    X = np.stack([np.cos(t) * t, np.sin(t) * t, 2 * t], 1) @ Q.T + 0.1 * syn.gauss(n * d, salt + 2).reshape(n, d)
    return X.astype(np.float32), t


def duplicates(n=300, d=16, salt=9300):
    """rows with exact copies (ties in the kNN order, zero distances, rho = 0 rows)"""
    X = syn.gauss(n * d, salt).reshape(n, d).astype(np.float32)
    X[[7, 150, 299]] = X[5]
    X[40:60] = X[40]                                  # 20 equal rows: a row whose k - 1 nearest are all at 0
    return X


def gaussian(n, d, salt, dtype=np.float32):
    return syn.gauss(n * d, salt).reshape(n, d).astype(dtype)


# cases of the golden file: name -> (generator, kwargs, k); tie-free, so sklearn's kNN indices are unambiguous
GOLDEN_CASES = {
    "blobs": (blobs, dict(n=400, d=32, c=4, salt=9110), 20),
    "spiral": (spiral, dict(n=300, d=24, salt=9210), 15),
    "small_d": (gaussian, dict(n=500, d=3, salt=9410), 10),
}
# PCA golden cases: name -> (n, d, salt, dtype); the last two have n < 10 d (sklearn's 'full' solver)
PCA_CASES = {
    "latent_f64": (2000, 32, 9500, np.float64),
    "latent_f32": (1000, 32, 9510, np.float32),
    "wide_f64": (200, 32, 9520, np.float64),
    "tiny_f64": (12, 5, 9530, np.float64),
}
# PCA cases beyond the golden file (checked against ``pca`` alone): more than one 2048-row chunk of the Gram kernel,
# and D = 129 columns (5 x 5 tiles)
PCA_KERNEL_CASES = {
    "chunks_f64": (5000, 32, 9540, np.float64),
    "chunks_f32": (5000, 32, 9550, np.float32),
    "tiles_f64": (3000, 128, 9560, np.float64),
}


def golden_input(name):
    gen, kw, k = GOLDEN_CASES[name]
    X = gen(**kw)
    return (X[0] if isinstance(X, tuple) else X), k


def pca_input(name):
    n, d, salt, dtype = PCA_CASES[name] if name in PCA_CASES else PCA_KERNEL_CASES[name]
    scale = 1.0 + 3.0 * np.arange(d)                    # well separated variances
    return (syn.gauss(n * d, salt).reshape(n, d) * scale + 0.5).astype(dtype)


# ---- kNN, bandwidths, memberships --------------------------------------------------------------------------------------
def distances(X):
    """fp64 euclidean distance matrix, the squared differences summed in column order"""
    X = np.asarray(X, dtype=np.float64)
    acc = np.zeros((len(X), len(X)))
    for c in range(X.shape[1]):
        df = X[:, None, c] - X[None, :, c]
        acc += df * df
    return np.sqrt(acc)


def knn(X, k):
    """column 0 the row itself at 0, then the k - 1 nearest other rows by (distance, index)"""
    D = distances(X)
    n = len(D)
    np.fill_diagonal(D, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(n), D.shape), D), axis=1)[:, :k - 1]
    idx = np.concatenate([np.arange(n)[:, None], order], 1).astype(np.int64)
    dist = np.concatenate([np.zeros((n, 1)), np.take_along_axis(D, order, 1)], 1)
    return idx, dist


def smooth_knn(idx, dist, local_connectivity=1.0, n_iter=64):
    """smooth_knn_dist (bandwidth 1, tolerance 1e-5, floor 1e-3 x mean distance) and compute_membership_strengths"""
    n, k = dist.shape
    target = np.log2(k)
    mean_all = dist.mean()
    rho = np.zeros(n)
    sigma = np.zeros(n)
    for i in range(n):
        row = dist[i]
        nz = row[row > 0.0]
        if len(nz) >= local_connectivity:
            index = int(np.floor(local_connectivity))
            interp = local_connectivity - index
            if index > 0:
                rho[i] = nz[index - 1]
                if interp > 1e-5:
                    rho[i] += interp * (nz[index] - nz[index - 1])
            elif len(nz) > 0:                           # local_connectivity 0 admits a row with no nonzero distance
                rho[i] = interp * nz[0]
        elif len(nz) > 0:
            rho[i] = np.max(nz)
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(n_iter):
            psum = 0.0
            for j in range(1, k):
                d = row[j] - rho[i]
                psum += np.exp(-(d / mid)) if d > 0 else 1.0
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2 if hi == np.inf else (lo + hi) / 2.0
        floor = 1e-3 * (row.mean() if rho[i] > 0.0 else mean_all)
        sigma[i] = max(mid, floor)
    dd = dist - rho[:, None]
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        w = np.where((dd <= 0) | (sigma[:, None] == 0), 1.0, np.exp(-(dd / sigma[:, None])))
    w[idx == np.arange(n)[:, None]] = 0.0
    return sigma, rho, w


def psum(dist, rho, sigma):
    """the bandwidth search's sum for the final sigma of every row"""
    dd = dist[:, 1:] - rho[:, None]
    return np.where(dd > 0, np.exp(-(dd / sigma[:, None])), 1.0).sum(1)


def fuzzy_union_dense(idx, w, n, set_op_mix_ratio=1.0):
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), idx.shape[1]), idx.ravel()] = w.ravel()
    prod = A * A.T
    return set_op_mix_ratio * (A + A.T - prod) + (1.0 - set_op_mix_ratio) * prod


# ---- schedule, init, layout ------------------------------------------------------------------------------------------
def find_ab_params(spread=1.0, min_dist=0.1):
    from scipy.optimize import curve_fit
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    p, _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(p[0]), float(p[1])


def prune(G, n_epochs):
    """CSR graph with the weights below max / n_epochs removed"""
    G = scipy.sparse.csr_matrix(G, copy=True)
    G.data[G.data < G.data.max() / float(n_epochs)] = 0.0
    G.eliminate_zeros()
    G.sort_indices()
    return G


def layout(G, Y0, n_epochs, a, b, salt, epochs=None, gamma=1.0, learning_rate=1.0, negative_sample_rate=5,
           cap=False):
    """``epochs`` (default all) of the synchronous layout over the pruned CSR graph ``G`` from ``Y0``: each vertex
    sums, in CSR order, 2 alpha clip(g (y_v - y_j)) for every active edge followed by that edge's negative samples,
    all from the previous epoch's positions.  An edge that is due more than ``MAX_NEG`` negative samples in one epoch
    is an error, or, with ``cap``, draws ``MAX_NEG`` and advances its counter by as many, as the kernel does; then the
    result is ``(Y, flagged)``, ``flagged`` telling whether any edge was capped"""
    epochs = n_epochs if epochs is None else epochs
    n = G.shape[0]
    nnz = G.nnz
    head = np.repeat(np.arange(n), np.diff(G.indptr))
    tail = G.indices.astype(np.int64)
    w = G.data
    eps = np.full(nnz, -1.0)
    ns = n_epochs * (w / w.max())
    eps[ns > 0] = float(n_epochs) / ns[ns > 0]
    epn = eps / negative_sample_rate
    next_s, next_n = eps.copy(), epn.copy()
    Y = np.array(Y0, dtype=np.float64)
    flagged = False

    def clip(v):
        return np.clip(v, -4.0, 4.0)

    for ep in range(epochs):
        alpha = learning_rate if ep == 0 else learning_rate * (1.0 - (ep - 1) / n_epochs)
        act = next_s <= ep
        moves = np.zeros((nnz, 1 + MAX_NEG, 2))
        use = np.zeros((nnz, 1 + MAX_NEG), dtype=bool)
        diff = Y[head] - Y[tail]
        d2 = (diff ** 2).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(d2 > 0, -2.0 * a * b * np.power(d2, b - 1.0) / (a * np.power(d2, b) + 1.0), 0.0)
        moves[:, 0] = 2.0 * alpha * clip(g[:, None] * diff)
        use[:, 0] = act
        next_s[act] += eps[act]
        nneg = np.zeros(nnz, dtype=np.int64)
        nneg[act] = ((ep - next_n[act]) / epn[act]).astype(np.int64)
        if cap:
            flagged = flagged or bool(nneg.max(initial=0) > MAX_NEG)
            nneg = np.minimum(nneg, MAX_NEG)
        else:
            assert nneg.max(initial=0) <= MAX_NEG
        u = syn.u01(nnz * MAX_NEG, salt, start=ep * nnz * MAX_NEG).reshape(nnz, MAX_NEG)
        kk = np.minimum(np.floor(u * n).astype(np.int64), n - 1)
        ndiff = Y[head][:, None, :] - Y[kk]
        nd2 = (ndiff ** 2).sum(2)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = 2.0 * gamma * b / ((0.001 + nd2) * (a * np.power(nd2, b) + 1.0))
        ok = act[:, None] & (np.arange(MAX_NEG)[None, :] < nneg[:, None]) & (kk != head[:, None]) & (nd2 > 0) & (c > 0)
        moves[:, 1:] = np.where(ok[:, :, None], alpha * clip(c[:, :, None] * ndiff), 0.0)
        use[:, 1:] = ok
        next_n[act] += nneg[act] * epn[act]
        M = np.zeros((n, 2))
        np.add.at(M, np.repeat(head, 1 + MAX_NEG)[use.ravel()], moves.reshape(-1, 2)[use.ravel()])
        Y = Y + M
    return (Y, flagged) if cap else Y


LAYOUT_ISOLATED = [3, 17, 64, 129]        # one in each 64-vertex workgroup, the last vertex among them
LAYOUT_CLUSTER = list(range(20, 30))      # vertices that start at one position
LAYOUT_SALT = 9820                        # of the negative samples


def layout_edge_graph(n_epochs=12):
    """a small pruned graph with isolated vertices: the fuzzy graph of ``blobs(n=130, d=8, c=3)`` at k = 10 with the
    rows and columns of ``LAYOUT_ISOLATED`` emptied, pruned at ``n_epochs``"""
    X, _ = blobs(n=130, d=8, c=3, salt=9800)
    idx, dist = knn(X, 10)
    _, _, w = smooth_knn(idx, dist)
    A = fuzzy_union_dense(idx, w, len(X))
    A[LAYOUT_ISOLATED, :] = 0.0
    A[:, LAYOUT_ISOLATED] = 0.0
    return prune(scipy.sparse.csr_matrix(A), n_epochs)


def layout_edge_start(G, salt=9810):
    """``Y0`` (uniform in [0, 10)^2) for ``layout_edge_graph``: the vertices of ``LAYOUT_CLUSTER`` share one position
    (negative samples meet coincident points), and so do the two ends of the first edge of the largest weight (period
    1: active from epoch 1) that lies among the first 40 vertices outside the cluster; returns ``(Y0, (i, j))``"""
    n = G.shape[0]
    Y0 = 10.0 * syn.u01(2 * n, salt).reshape(n, 2)
    Y0[LAYOUT_CLUSTER] = Y0[LAYOUT_CLUSTER[0]]
    head = np.repeat(np.arange(n), np.diff(G.indptr))
    tail = G.indices
    top = (G.data == G.data.max()) & (head < tail) & (tail < 40)
    top &= ~np.isin(head, LAYOUT_CLUSTER) & ~np.isin(tail, LAYOUT_CLUSTER)
    e = int(np.flatnonzero(top)[0])
    i, j = int(head[e]), int(tail[e])
    Y0[j] = Y0[i]
    return Y0, (i, j)


def induced(G, m, n_epochs=12):
    """the subgraph of ``G`` induced by its first ``m`` vertices, pruned again (its largest weight may be smaller)"""
    return prune(scipy.sparse.csr_matrix(G)[:m][:, :m], n_epochs)


# ---- PCA -----------------------------------------------------------------------------------------------------------
def gram(X):
    """``(G, A)``: the (d + 1) x (d + 1) Gram matrix ``[X, 1]^T [X, 1]`` of the rows converted to fp64 (as the kernel
    reads them) and summed in ``np.longdouble``, and ``A = [|X|, 1]^T [|X|, 1]``, the scale of its rounding error"""
    X = np.asarray(X, dtype=np.float64)
    Z = np.concatenate([X, np.ones((len(X), 1))], 1).astype(np.longdouble)
    return Z.T @ Z, np.abs(Z).T @ np.abs(Z)


def gram_bound(n, absgram):
    """first-order bound on the error of an fp64 sum of ``n`` fused multiply-adds taken in any order: every partial sum
    is rounded once, so no term passes through more than ``n`` roundings of 2^-53 each (the 2 more are slack for the
    rounding of the restatement and of the bound themselves)"""
    return (n + 2) * 2.0 ** -53 * absgram


def pca(X, n_components=2):
    """sklearn 1.7 PCA(copy=False).fit_transform along the covariance_eigh path, in fp64"""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    mean = X.mean(0)
    C = X.T @ X - n * mean[:, None] * mean[None, :]
    C /= n - 1
    _, vecs = np.linalg.eigh(C)
    Vt = np.flip(vecs, axis=1).T
    Vt = Vt * np.sign(Vt[np.arange(d), np.argmax(np.abs(Vt), axis=1)])[:, None]
    V = Vt[:n_components]
    return X @ V.T - mean[None, :] @ V.T


# ---- quality -------------------------------------------------------------------------------------------------------
def trustworthiness(X, Y, n_neighbors=10):
    """sklearn.manifold.trustworthiness with the euclidean metric, in numpy"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    n = len(X)
    DX = distances(X)
    np.fill_diagonal(DX, np.inf)
    ind_X = np.argsort(DX, axis=1)
    DY = distances(Y)
    np.fill_diagonal(DY, np.inf)
    ind_Y = np.argsort(DY, axis=1)[:, :n_neighbors]
    inverted = np.zeros((n, n), dtype=np.int64)
    ordered = np.arange(n + 1)
    inverted[ordered[:-1, None], ind_X] = ordered[1:]
    ranks = inverted[ordered[:-1, None], ind_Y] - n_neighbors
    t = np.sum(ranks[ranks > 0])
    return 1.0 - t * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0)))


def knn_label_accuracy(Y, labels, k=5):
    """fraction of points whose k nearest others in ``Y`` carry the majority label equal to their own"""
    D = distances(Y)
    np.fill_diagonal(D, np.inf)
    nb = np.argsort(D, axis=1, kind="stable")[:, :k]
    votes = labels[nb]
    pred = np.array([np.bincount(v, minlength=labels.max() + 1).argmax() for v in votes])
    return float((pred == labels).mean())
