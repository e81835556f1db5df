"""Cases and numpy restatements for the out-of-sample half of ava_amd.projection (``TransformableUMAP.transform``) and
for ava_amd.refine_segments.

The restatements follow the device path step by step (umap-learn 0.5's ``transform`` with this package's deviations);
they are the oracle of tests/test_gpu_refine.py.  Everything shared with the fit comes from tests/projection_cases.py.
The synthetic recordings and segment files come from ava_amd.synthetic's hash streams, so tests/golden/refine.npz
(written by tests/golden/make_golden_refine.py) holds results only.
"""
import os

import numpy as np

import projection_cases as PC
from ava_amd import synthetic as syn

MAX_NEG = PC.MAX_NEG


# ---- query kNN, memberships, start positions ------------------------------------------------------------------------
def query_distances(Q, X):
    """fp64 euclidean distances [m, n], the squared differences summed in column order"""
    Q = np.asarray(Q, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    acc = np.zeros((len(Q), len(X)))
    for c in range(X.shape[1]):
        df = Q[:, None, c] - X[None, :, c]
        acc += df * df
    return np.sqrt(acc)


def knn_query(Q, X, k):
    """the k nearest rows of X of every row of Q by (distance, index); no row excluded"""
    D = query_distances(Q, X)
    order = np.lexsort((np.broadcast_to(np.arange(D.shape[1]), D.shape), D), axis=1)[:, :k]
    return order.astype(np.int64), np.take_along_axis(D, order, 1)


def smooth_knn_bipartite(idx, dist, local_connectivity=0.0):
    """``PC.smooth_knn`` without the zeroed own column.  ``PC.smooth_knn`` zeroes ``w`` where ``idx`` equals the row
    number; handing it indices that never do (-1) leaves every other step as it is."""
    return PC.smooth_knn(np.full(idx.shape, -1, dtype=np.int64), dist, local_connectivity)


def normalize_init(idx, w, E):
    """rows of ``w`` over their sum (left to right; a zero row stays zero) and the weighted mean of ``E[idx]`` in slot
    order: (wn, Y0)"""
    m, k = w.shape
    total = np.zeros(m)
    for s in range(k):
        total = total + w[:, s]
    wn = np.where(total[:, None] > 0, w / np.where(total > 0, total, 1.0)[:, None], 0.0)
    Y0 = np.zeros((m, 2))
    for s in range(k):
        Y0 = Y0 + wn[:, s, None] * E[idx[:, s]]
    return wn, Y0


def schedule(w, n_epochs, negative_sample_rate=5):
    """(eps, epn) [m, k]: -1 for the slots below ``w.max() / n_epochs``, else ``n_epochs / (n_epochs w / w.max())``"""
    eps = np.full(w.shape, -1.0)
    keep = ~(w < w.max() / float(n_epochs)) & (w != 0.0)
    ns = n_epochs * (w[keep] / w[keep].max()) if keep.any() else np.zeros(0)
    eps[keep] = float(n_epochs) / ns
    return eps, eps / negative_sample_rate


def transform_layout(Y0, E, idx, eps, epn, n_epochs, a, b, salt, epochs=None, gamma=1.0, learning_rate=1.0,
                     cap=False):
    """``epochs`` (default all) of the transform layout: row i walks its slots in order; a due slot pulls
    ``y_i`` towards ``E[idx[i, s]]`` by ``alpha clip(g (y_i - E[j]))`` (once), then pushes it from its negative samples
    one after the other, each from the updated ``y_i``.  Vectorised over the rows, serial over slots and samples, which
    is the order every row sees.  ``cap`` as in ``PC.layout``: the result is then ``(Y, flagged)``."""
    epochs = n_epochs if epochs is None else epochs
    m, k = idx.shape
    n = len(E)
    next_s = np.where(eps > 0, eps, np.inf)
    next_n = epn.copy()
    Y = np.array(Y0, dtype=np.float64)
    alpha0 = learning_rate / 4.0
    flagged = False

    def clip(v):
        return np.clip(v, -4.0, 4.0)

    for ep in range(epochs):
        alpha = alpha0 if ep == 0 else alpha0 * (1.0 - (ep - 1) / n_epochs)
        # counter ((ep m + i) k + s) 16 + p: this epoch's are one contiguous range
        u_ep = syn.u01(m * k * MAX_NEG, salt, start=ep * m * k * MAX_NEG).reshape(m, k, MAX_NEG)
        for s in range(k):
            act = next_s[:, s] <= ep
            if not act.any():
                continue
            diff = Y - E[idx[:, s]]
            d2 = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(d2 > 0, -2.0 * a * b * np.power(d2, b - 1.0) / (a * np.power(d2, b) + 1.0), 0.0)
            Y = np.where(act[:, None], Y + alpha * clip(g[:, None] * diff), Y)
            next_s[act, s] += eps[act, s]
            nneg = np.zeros(m, dtype=np.int64)
            nneg[act] = ((ep - next_n[act, s]) / epn[act, s]).astype(np.int64)
            if cap:
                flagged = flagged or bool(nneg.max(initial=0) > MAX_NEG)
                nneg = np.minimum(nneg, MAX_NEG)
            else:
                assert nneg.max(initial=0) <= MAX_NEG
            for p in range(int(nneg.max(initial=0))):
                kk = np.minimum(np.floor(u_ep[:, s, p] * n).astype(np.int64), n - 1)
                diff = Y - E[kk]
                d2 = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]
                with np.errstate(divide="ignore", invalid="ignore"):
                    c = 2.0 * gamma * b / ((0.001 + d2) * (a * np.power(d2, b) + 1.0))
                ok = act & (p < nneg) & (d2 > 0) & (c > 0)
                Y = np.where(ok[:, None], Y + alpha * clip(c[:, None] * diff), Y)
            next_n[act, s] += nneg[act] * epn[act, s]
    return (Y, flagged) if cap else Y


def transform(Xq, Xtrain, E, k, a, b, n_epochs=None, transform_seed=42, local_connectivity=1.0,
              negative_sample_rate=5, gamma=1.0, learning_rate=1.0):
    """the whole of ``TransformableUMAP.transform`` on float32 rows, in numpy: fp64 ``[m, 2]``"""
    Xq = np.asarray(Xq, dtype=np.float32)
    Xtrain = np.asarray(Xtrain, dtype=np.float32)
    E = np.asarray(E, dtype=np.float32).astype(np.float64)
    idx, dist = knn_query(Xq, Xtrain, k)
    _, _, w = smooth_knn_bipartite(idx, dist, max(0.0, local_connectivity - 1.0))
    _, Y0 = normalize_init(idx, w, E)
    m = len(Xq)
    n_epochs = (100 if m <= 10000 else 30) if n_epochs is None else int(n_epochs // 3)
    if n_epochs == 0:
        return Y0
    eps, epn = schedule(w, n_epochs, negative_sample_rate)
    salt = np.random.RandomState(transform_seed).randint(2 ** 31 - 1)
    return transform_layout(Y0, E, idx, eps, epn, n_epochs, a, b, salt, gamma=gamma, learning_rate=learning_rate)


# ---- kernel cases ------------------------------------------------------------------------------------------------------
KNN_CASE = dict(n=300, m=130, d=40, k=20)      # 5 reference tiles (last partial), 3 workgroups, 2 column stages


def knn_case(dtype=np.float32):
    c = KNN_CASE
    return PC.gaussian(c['m'], c['d'], 9910, dtype), PC.gaussian(c['n'], c['d'], 9900, dtype), c['k']


def copies_case(dtype=np.float32):
    """references with a block of 20 equal rows and queries that are exact copies of reference rows: (Q, X, rows the
    first 40 queries copy)"""
    X = PC.gaussian(300, 16, 9920, dtype)
    X[40:60] = X[40]
    src = np.concatenate([np.arange(0, 300, 15), np.arange(40, 60)])        # 20 spread rows, then the equal block
    Q = np.concatenate([X[src], PC.gaussian(30, 16, 9921, dtype)])
    return Q, X, src


def membership_case():
    """a query table with rows whose nearest reference is at distance 0 and rows (the copies of the equal block, row
    25 among them) whose k nearest all are: (idx, dist, E) at k = 20"""
    Q, X, _ = copies_case()
    idx, dist = knn_query(Q, X, 20)
    assert np.any(dist[:, 0] == 0) and np.all(dist[25] == 0) and np.any(dist[:, 0] > 0)
    E = 10.0 * syn.u01(2 * len(X), 9930).reshape(len(X), 2)
    return idx, dist, E


LAYOUT_SALT = 9950
LAYOUT_PRUNED_ROW = 77
LAYOUT_ON_POINT_ROW = 129


def layout_case(n_epochs=12, m=130, n=400, k=10):
    """a transform layout problem with no device fit behind it: hash-uniform training positions in [0, 10)^2,
    neighbours and weights from a query kNN of Gaussian rows.  Row ``LAYOUT_PRUNED_ROW`` has every weight below the
    pruning threshold; row ``LAYOUT_ON_POINT_ROW`` (in the last, partial 64-row group) has all its weight on slot 0
    and so starts exactly on a training point.  Returns (idx, w, E)."""
    X = PC.gaussian(n, 8, 9940)
    Q = PC.gaussian(m, 8, 9941)
    idx, dist = knn_query(Q, X, k)
    _, _, w = smooth_knn_bipartite(idx, dist, 0.0)
    w = w.copy()
    w[LAYOUT_PRUNED_ROW] = w.max() / (4.0 * n_epochs)
    w[LAYOUT_ON_POINT_ROW] = 0.0
    w[LAYOUT_ON_POINT_ROW, 0] = w.max()
    E = 10.0 * syn.u01(2 * n, 9942).reshape(n, 2)
    return idx, w, E


# ---- synthetic recordings and segment files --------------------------------------------------------------------------
REFINE_P = dict(fs=32000, nperseg=256, noverlap=128, min_freq=400, max_freq=10e3, spec_min_val=2.0, spec_max_val=6.0)
REFINE_MAX_LEN = 40           # shorter than the longest segment's spectrogram: that one is truncated

# per directory: per recording its name, seconds and the (onset, offset) lines of its segment file
REFINE_DIRS = [
    [("a_00", 0.60, [(0.020, 0.100), (0.150, 0.152), (0.200, 0.330), (0.400, 0.480)]),   # line 2: <= nperseg samples
     ("a_01", 0.50, []),                                                                 # no segments
     ("a_02", 0.70, [(0.010, 0.250), (0.300, 0.380), (0.450, 0.530)])],                  # line 1: longer than max_len
    [("b_00", 0.55, [(0.030, 0.110), (0.200, 0.290)]),
     ("b_01", 0.65, [(0.050, 0.130), (0.180, 0.185), (0.250, 0.340), (0.420, 0.500)])],
]


def refine_audio(name, seconds, fs=32000):
    """one int16 recording: ``syn.recordings`` cut to length, salted by its name"""
    salt = 4100 + sum(ord(c) for c in name)
    audio, _ = syn.recordings(n_files=1, fs=fs, seconds=1.0, salt=salt)
    return audio[0][:int(seconds * fs)].copy()


def write_refine_dirs(root):
    """writes the recordings and segment files of ``REFINE_DIRS`` under ``root``: (audio_dirs, seg_dirs) relative to
    ``root``.  ``update_segments`` writes the paths it is given into its headers, so callers work from inside ``root``
    to get the same bytes anywhere."""
    from scipy.io import wavfile
    audio_dirs, seg_dirs = [], []
    for d, files in enumerate(REFINE_DIRS):
        ad, sd = os.path.join(root, "audio_%d" % d), os.path.join(root, "segs_%d" % d)
        os.makedirs(ad)
        os.makedirs(sd)
        for name, seconds, segs in files:
            wavfile.write(os.path.join(ad, name + ".wav"), REFINE_P['fs'], refine_audio(name, seconds))
            np.savetxt(os.path.join(sd, name + ".txt"), np.array(segs).reshape(-1, 2), fmt='%.5f',
                       header="Onsets/offsets for " + name + ".wav")
        audio_dirs.append("audio_%d" % d)
        seg_dirs.append("segs_%d" % d)
    return audio_dirs, seg_dirs


def stub_vectors(d):
    """the two fixed hash vectors the stub transform projects rows on"""
    return syn.gauss(2 * d, 9960).reshape(2, d) / np.sqrt(d)


class StubTransform:
    """stands in for a fitted UMAP in ``update_segments``: rows projected on two fixed hash vectors"""

    def transform(self, rows):
        rows = rows.cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)
        rows = np.asarray(rows, dtype=np.float64)
        return rows @ stub_vectors(rows.shape[1]).T


def read_tree(dirs):
    """{directory index / file name: text} of every file in ``dirs``"""
    out = {}
    for d, path in enumerate(dirs):
        for fn in sorted(os.listdir(path)):
            with open(os.path.join(path, fn)) as f:
                out["%d/%s" % (d, fn)] = f.read()
    return out
