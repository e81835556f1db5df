"""Writes tests/golden/hdbscan.npz: scikit-learn 1.7.2's own HDBSCAN results for the blob cases of
tests/hdbscan_cases.py (needs scikit-learn only; run from the repository root:
``python tests/golden/make_golden_hdbscan.py``).

Per blob case: sklearn's ``labels_`` (``labels``) and ``probabilities_`` (``probabilities``) on the float64 copy of the
rows under ``algorithm='brute'``, the seed the case's generator settles on (``seed``), the restatement's smallest
relative gap of a stability comparison (``stability_gap``) and ``prob_err``, the largest |restatement - sklearn| over
``probabilities_``, measured here, when the file is written.  The generator condition (the restatement's partition equals
sklearn's under 'brute', 'kd_tree' and 'ball_tree', at least two clusters, some noise, a gap of at least 1e-9) is
asserted.  Data only: the GPU tests read it where scikit-learn may be absent."""
import os
import sys

import numpy as np
import sklearn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dbscan_cases as DC  # noqa: E402
import hdbscan_cases as HC  # noqa: E402


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out = {}
    for name in HC.BLOB_CASES:
        seed = HC.find_seed(name)
        assert seed == HC.SEEDS[name], (name, seed)
        X, mcs, ms, method = HC.case(name)
        assert HC.generator_condition(X, mcs, ms), name
        want = HC.expected(name)
        sk = HC.sklearn_fit(X, mcs, ms, "brute", method)
        assert np.array_equal(DC.by_smallest_member(sk.labels_), DC.by_smallest_member(want["labels"])), name
        out[name + "_labels"] = sk.labels_.astype(np.int64)
        out[name + "_probabilities"] = sk.probabilities_.astype(np.float64)
        out[name + "_seed"] = np.int64(seed)
        out[name + "_stability_gap"] = np.float64(want["stability_gap"])
        out[name + "_prob_err"] = np.float64(np.abs(want["probabilities"] - sk.probabilities_).max())
        print("%-10s N %4d d %2d min_cluster_size %2d min_samples %4s seed %d: %d clusters, %d noise, %d hub rows, "
              "stability gap %.2e, prob_err %.2e" % (name, X.shape[0], X.shape[1], mcs, ms, seed, want["n_clusters"],
                                                     want["n_noise"], len(want["hub_rows"]), want["stability_gap"],
                                                     out[name + "_prob_err"]))
    path = os.path.join(HERE, "hdbscan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
