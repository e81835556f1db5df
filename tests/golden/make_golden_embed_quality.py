"""Writes tests/golden/embed_quality.npz: scikit-learn 1.7's trustworthiness on the cases of
``tests/embed_quality_cases.py::GOLDEN_CASES`` (imports numpy and sklearn only, beside that cases module).

For every case (n, d, k, seed): ``rs = RandomState(seed)``, ``X = rs.standard_normal((n, d))`` and then
``Y = PCA(2).fit_transform(X) + 0.3 * rs.standard_normal((n, 2))``.  X is regenerated from the seed by the cases module;
Y is stored, because PCA's last bits are not portable.  The file stores

* ``c{i}_Y``: the embedding;
* ``c{i}_trust`` / ``c{i}_cont``: ``sklearn.manifold.trustworthiness(X, Y, n_neighbors=k)`` and ``(Y, X, ...)``;
* ``c{i}_pen_t`` / ``c{i}_pen_c``: the integer penalty sums of the restatement, which reproduce those floats exactly;
* ``c{i}_rank_x`` / ``c{i}_rank_y`` for the first two cases: the rank tables [n, k].

Condition on the cases, asserted here: in every row of both spaces consecutive sorted distances differ by at least
``MIN_GAP`` relative, so sklearn's expanded, rooted distances and its unstable sort order no pair differently from the
strict (distance, index) order, and the restatement's floats equal sklearn's.

    python tests/golden/make_golden_embed_quality.py
"""
import os
import sys

import numpy as np
from sklearn.decomposition import PCA
from sklearn.manifold import trustworthiness

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import embed_quality_cases as EC  # noqa: E402


def main():
    out = {}
    for i, (n, d, k, seed) in enumerate(EC.GOLDEN_CASES):
        rs, X = EC.golden_x(n, d, seed)
        Y = PCA(2).fit_transform(X) + 0.3 * rs.standard_normal((n, 2))
        gaps = EC.min_gap(EC.sqd(X)), EC.min_gap(EC.sqd(Y))
        assert min(gaps) >= EC.MIN_GAP, (i, gaps)
        t, c = float(trustworthiness(X, Y, n_neighbors=k)), float(trustworthiness(Y, X, n_neighbors=k))
        pair = EC.Pair(X, Y, k)
        cur = pair.curve([k])
        assert cur["trustworthiness"][0] == t and cur["continuity"][0] == c, (i, cur, t, c)
        out["c%d_Y" % i] = Y
        out["c%d_trust" % i], out["c%d_cont" % i] = np.float64(t), np.float64(c)
        out["c%d_pen_t" % i], out["c%d_pen_c" % i] = cur["penalty_t"][0], cur["penalty_c"][0]
        if i < EC.GOLDEN_RANK_TABLES:
            out["c%d_rank_x" % i], out["c%d_rank_y" % i] = pair.rank_x, pair.rank_y
        print("case %d: n=%d d=%d k=%d trust=%.17g cont=%.17g least gaps %.3g / %.3g" % ((i, n, d, k, t, c) + gaps))
    path = os.path.join(HERE, "embed_quality.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
