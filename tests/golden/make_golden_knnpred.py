"""Writes tests/golden/knnpred.npz: scikit-learn 1.7.2's own cross-validated k-nearest-neighbour predictions for the
cases of tests/knnpred_cases.py (needs scikit-learn only; run from the repository root:
``python tests/golden/make_golden_knnpred.py``).

Per case of ``SKLEARN_CASES`` and weighting ``w`` in ('uniform', 'distance'), for the k of the case's sweep, on the float64
copy of the rows with ``algorithm='brute'`` and ``cv=PredefinedSplit(fold)``:

* ``<case>_<w>_classes`` int64 [n_k, N]: ``cross_val_predict(KNeighborsClassifier)``;
* ``<case>_<w>_values`` float64 [n_k, N, 3]: ``cross_val_predict(KNeighborsRegressor)``;
* ``<case>_<w>_accuracy`` / ``<case>_<w>_r2`` float64 [n_folds, n_k]: ``cross_val_score`` of the two (the leave-one-out
  cases have no R^2: a fold of one row has none).

Data only: the GPU tests read it where scikit-learn may be absent."""
import os
import sys

import numpy as np
import sklearn
from sklearn.model_selection import PredefinedSplit, cross_val_predict, cross_val_score
from sklearn.neighbors import KNeighborsClassifier, KNeighborsRegressor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import knnpred_cases as KC  # noqa: E402


def sklearn_results(name):
    """the arrays of one case, keyed as in the file"""
    c = KC.case(name)
    X = np.asarray(c["X"], dtype=np.float64)
    cv = PredefinedSplit(c["fold"])
    loo = len(np.unique(c["fold"])) == len(X)
    out = {}
    for w in KC.WEIGHTS:
        clf = [KNeighborsClassifier(k, weights=w, algorithm='brute') for k in c["ks"]]
        reg = [KNeighborsRegressor(k, weights=w, algorithm='brute') for k in c["ks"]]
        out["%s_%s_classes" % (name, w)] = np.stack([cross_val_predict(m, X, c["y"], cv=cv) for m in clf]).astype(np.int64)
        out["%s_%s_values" % (name, w)] = np.stack([cross_val_predict(m, X, c["Y"], cv=cv) for m in reg])
        out["%s_%s_accuracy" % (name, w)] = np.stack([cross_val_score(m, X, c["y"], cv=cv) for m in clf], axis=1)
        if not loo:
            out["%s_%s_r2" % (name, w)] = np.stack([cross_val_score(m, X, c["Y"], cv=cv) for m in reg], axis=1)
    return out


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out = {}
    for name in KC.SKLEARN_CASES:
        res = sklearn_results(name)
        out.update(res)
        c, e = KC.case(name), KC.expected(name)
        print("%-22s seed %5d k %s: distance margin %.1e, score margin %.1e, accuracy at the largest k %.3f / %.3f"
              % (name, c["seed"], c["ks"], e["distance_margin"], e["score_margin"],
                 res[name + "_uniform_accuracy"][:, -1].mean(), res[name + "_distance_accuracy"][:, -1].mean()))
    path = os.path.join(HERE, "knnpred.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
