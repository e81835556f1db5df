"""Regenerate tests/golden/neighbors.npz (row f7): the searches of the reference's shotgun_movie_DC on the cases of
tests/neighbor_cases.py.

Correlation cases: ``NearestNeighbors(n_neighbors=1, metric='correlation').fit(refs).kneighbors(queries)``
(shotgun_movie.py:148-153).  Euclidean cases: ``np.argmin([euclidean(latent[i], j) for j in original_latent])``
(shotgun_movie.py:126-129), run literally, with the distance scipy gives for the chosen row.  Per case the npz holds
``<name>_params`` (metric, nq, nr, d, dtype, salt, dup, flat), ``<name>_idx``, ``<name>_dist`` and ``<name>_gap``:
the second-best minus the best distance of each query (``pairwise_distances`` / the same euclidean list).

Needs scikit-learn and scipy; run from the repository root:  python tests/golden/make_golden_neighbors.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import neighbor_cases as NC                                   # noqa: E402
from scipy.spatial.distance import euclidean                  # noqa: E402
from sklearn.metrics import pairwise_distances                # noqa: E402
from sklearn.neighbors import NearestNeighbors                # noqa: E402


def main():
    out = {}
    for name, (metric, nq, nr, d, dtype, salt, dup, flat) in NC.CASES.items():
        queries, refs = NC.case_inputs(name)
        if metric == "correlation":
            nbrs = NearestNeighbors(n_neighbors=1, metric='correlation')
            nbrs.fit(refs)
            dist, idx = nbrs.kneighbors(queries)
            idx, dist = idx.flatten(), dist.flatten()
            gap = NC.gap(pairwise_distances(queries, refs, metric='correlation'))
        else:
            idx, dist, gap = [], [], []
            for i in range(len(queries)):
                row = [euclidean(queries[i], j) for j in refs]
                index = np.argmin(row)
                idx.append(index)
                dist.append(row[index])
                gap.append(NC.gap(np.array([row]))[0])
        out[name + "_params"] = NC.params_row(name)
        out[name + "_idx"] = np.asarray(idx, dtype=np.int64)
        out[name + "_dist"] = np.asarray(dist, dtype=np.float64)
        out[name + "_gap"] = np.asarray(gap, dtype=np.float64)
        print(name, "min gap %.3g" % np.min(out[name + "_gap"]))
    path = os.path.join(ROOT, "tests", "golden", "neighbors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
