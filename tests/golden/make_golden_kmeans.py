"""Regenerates tests/golden/kmeans.npz from scikit-learn (needs scikit-learn only; run by hand from the repository root:
``python tests/golden/make_golden_kmeans.py``).  The arrays were made with scikit-learn 1.7.2.

For every case of ``tests/kmeans_cases.py::FIT_CASES`` the file stores what ``sklearn.cluster.KMeans(algorithm='lloyd',
**arguments).fit`` gives on the float64 rows -- ``labels``, ``centres``, ``inertia``, ``n_iter`` -- and ``pp``, the indices
of ``sklearn.cluster.kmeans_plusplus(X, n_clusters, random_state=...)`` with the case's ``random_state`` (0 where the case
has none).

Beside every float quantity ``q`` the file stores ``floor_q``: the larger of |sklearn - restatement| and |sklearn - sklearn
on rows perturbed by 1e-15 relative|, relative to max |sklearn| (the convention of make_golden_gmm.py).  That is the
reference-side noise the tests scale their bounds with.  Where the perturbed run takes another path (other labels or
another n_iter) only the restatement's difference counts; the script says so.
"""
import os
import sys
import warnings

import numpy as np
from sklearn.cluster import KMeans, kmeans_plusplus

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_cases as KC  # noqa: E402

warnings.filterwarnings("ignore")
PERTURBATION = 1e-15


def perturbed(X, salt):
    rng = np.random.RandomState(salt)
    return np.asarray(X, dtype=np.float64) * (1.0 + PERTURBATION * rng.standard_normal(X.shape))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(a).max(), np.finfo(float).tiny))


def sk_fit(X, kw):
    km = KMeans(algorithm='lloyd', **kw).fit(np.asarray(X, dtype=np.float64))
    return dict(labels=km.labels_.astype(np.int32), centres=km.cluster_centers_.astype(np.float64),
                inertia=np.float64(km.inertia_), n_iter=np.int64(km.n_iter_))


def main():
    out = {}
    for name in KC.FIT_CASES:
        X, kw = KC.fit_case(name)
        sk = sk_fit(X, kw)
        sp = sk_fit(perturbed(X, 3), kw)
        args = dict(kw)
        mine = KC.fit(X, args.pop('n_clusters'), **args)
        same_path = bool(np.array_equal(sk["labels"], sp["labels"]) and sk["n_iter"] == sp["n_iter"])
        for q in ("labels", "centres", "inertia", "n_iter"):
            out["%s/%s" % (name, q)] = sk[q]
        floors = []
        for q in ("centres", "inertia"):
            f = rel(sk[q], mine[q])
            if same_path:
                f = max(f, rel(sk[q], sp[q]))
            out["%s/floor_%s" % (name, q)] = np.float64(f)
            floors.append(f)
        seed = kw.get('random_state', 0)
        out["%s/pp" % name] = kmeans_plusplus(X, kw['n_clusters'], random_state=seed)[1].astype(np.int64)
        print("%-20s n_iter %3d (restatement %3d) labels equal %d  perturbed run on the same path %d  floors: %s"
              % (name, sk["n_iter"], mine["n_iter"], np.array_equal(sk["labels"], mine["labels"]), same_path,
                 " ".join("%.1e" % f for f in floors)))
    path = os.path.join(HERE, "kmeans.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
