"""Writes tests/golden/tsne.npz: scikit-learn 1.7's own values for the cases of tests/tsne_cases.py (needs
scikit-learn only; run from the repository root: ``python tests/golden/make_golden_tsne.py``).

For each golden case of the probabilities: sklearn's ``squareform(_joint_probabilities(D2, perplexity, 0))`` and
``_kl_divergence`` (value and gradient) at a stored Y.  For each whole-run case: sklearn's ``kl_divergence_`` with
``init=`` the same array as the device gets, and the final KL of the restatement from ``RUN_STARTS`` starts perturbed by
``RUN_PERTURBATION`` relative."""
import os
import sys

import numpy as np
from scipy.spatial.distance import squareform
from sklearn.manifold import TSNE
from sklearn.manifold import _t_sne

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import tsne_cases as TC  # noqa: E402


def main():
    out = {}
    for name in TC.GOLDEN_P_CASES:
        X, perplexity, _, D2, P = TC.p_case(name)
        n = len(X)
        cond = _t_sne._joint_probabilities(D2.copy(), perplexity, 0)
        out["P_" + name] = squareform(cond)
        Y = TC.spread_y(n)
        kl, grad = _t_sne._kl_divergence(Y.ravel().copy(), cond, 1, n, 2)
        out["Y_" + name], out["kl_" + name], out["grad_" + name] = Y, np.float64(kl), grad.reshape(n, 2)
        print("%-10s n=%3d  |P - restatement| / max P = %.2e" % (name, n, np.abs(out["P_" + name] - P).max() / P.max()))
    for name in TC.RUN_CASES:
        metric, X, labels, perplexity, D2, P = TC.run_case(name)
        n = len(P)
        Y0 = TC.random_init(n)
        sk = TSNE(n_components=2, perplexity=perplexity, metric=metric, method="exact", init=Y0.astype(np.float32))
        emb = sk.fit_transform(np.array(X))
        out["sklearn_kl_" + name] = np.float64(sk.kl_divergence_)
        rng = np.random.RandomState(1)
        kls, fracs = [], []
        for _ in range(TC.RUN_STARTS):
            Y, kl, it = TC.run(P, Y0 * (1.0 + TC.RUN_PERTURBATION * rng.standard_normal(Y0.shape)))
            assert it == 999
            kls.append(kl)
            fracs.append(TC.neighbour_label_fraction(Y, labels))
        out["restatement_kl_" + name] = np.array(kls)
        print("%-14s sklearn kl %.4f (neighbour fraction %.3f); restatement kl %.4f .. %.4f, fraction >= %.3f"
              % (name, sk.kl_divergence_, TC.neighbour_label_fraction(emb, labels), min(kls), max(kls), min(fracs)))
    path = os.path.join(HERE, "tsne.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
