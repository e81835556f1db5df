"""Writes tests/golden/dbscan.npz: scikit-learn 1.7.2's own DBSCAN results for the cases of tests/dbscan_cases.py
(needs scikit-learn only; run from the repository root: ``python tests/golden/make_golden_dbscan.py``).

Per case: sklearn's ``labels_`` (``labels``) and ``core_sample_indices_`` (``core``) on the float64 copy of the rows
under ``algorithm='brute'`` (the other three settings are asserted to agree), the number of clusters (``n_clusters``)
and the case's margin (``margin``: how far, relative to eps^2, the nearest pair is from the radius).  Data only: the GPU
tests read it where scikit-learn may be absent."""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dbscan_cases as DC  # noqa: E402

ALGORITHMS = ("brute", "kd_tree", "ball_tree", "auto")


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out = {}
    for name in DC.CASES:
        X, eps, min_samples = DC.case(name)
        X64 = np.asarray(X, dtype=np.float64)
        fits = [DBSCAN(eps=eps, min_samples=min_samples, algorithm=a).fit(X64) for a in ALGORITHMS]
        for f in fits[1:]:
            assert np.array_equal(f.labels_, fits[0].labels_), name
            assert np.array_equal(f.core_sample_indices_, fits[0].core_sample_indices_), name
        want = DC.expected(name)
        labels = fits[0].labels_.astype(np.int64)
        out[name + "_labels"] = labels
        out[name + "_core"] = fits[0].core_sample_indices_.astype(np.int64)
        out[name + "_n_clusters"] = np.int64(labels.max() + 1)
        out[name + "_margin"] = np.float64(want["margin"])
        print("%-14s N %4d d %2d eps %-10.4g min_samples %3d: %d clusters, %d core, %d border (%d ambiguous), %d noise,"
              " margin %.1e" % (name, X.shape[0], X.shape[1], eps, min_samples, out[name + "_n_clusters"],
                                len(out[name + "_core"]), want["n_border"], want["ambiguous"], want["n_noise"],
                                want["margin"]))
    path = os.path.join(HERE, "dbscan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
