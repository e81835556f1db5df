"""Writes tests/golden/cluster_metrics.npz: scikit-learn 1.7.2's own values for the golden cases of
tests/silhouette_cases.py (needs scikit-learn only; run from the repository root:
``python tests/golden/make_golden_silhouette.py``).

Per case: sklearn's ``silhouette_samples`` (``s``), ``silhouette_score`` (``score``), ``calinski_harabasz_score``
(``ch``) and ``davies_bouldin_score`` (``db``) on the float64 copy of the rows.  Beside every quantity ``q`` the file
stores ``floor_q``: the larger of |sklearn - the longdouble restatement| and |sklearn - sklearn on the rows in reversed
order| (the results put back in order), relative to max |sklearn|.  That is the reference-side noise the tests scale
their bounds with."""
import os
import sys

import numpy as np
import sklearn
from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score, silhouette_samples, silhouette_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import silhouette_cases as SC  # noqa: E402


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(a).max(), np.finfo(float).tiny))


def sk_values(X, labels):
    return dict(s=silhouette_samples(X, labels), score=np.float64(silhouette_score(X, labels)),
                ch=np.float64(calinski_harabasz_score(X, labels)), db=np.float64(davies_bouldin_score(X, labels)))


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out = {}
    for name in SC.GOLDEN_CASES:
        X, labels = SC.case(name)
        X64 = np.asarray(X, dtype=np.float64)
        mine = dict(SC.silhouette(name), ch=SC.calinski_harabasz(X, labels), db=SC.davies_bouldin(X, labels))
        sk = sk_values(X64, labels)
        rev = sk_values(X64[::-1].copy(), labels[::-1].copy())
        rev["s"] = rev["s"][::-1]
        floors = []
        for q in ("s", "score", "ch", "db"):
            out["%s_%s" % (name, q)] = sk[q]
            out["%s_floor_%s" % (name, q)] = np.float64(max(rel(sk[q], mine[q]), rel(sk[q], rev[q])))
            floors.append(out["%s_floor_%s" % (name, q)])
        print("%-14s floors (s, score, ch, db): %s" % (name, " ".join("%.1e" % f for f in floors)))
    path = os.path.join(HERE, "cluster_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
