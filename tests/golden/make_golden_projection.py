"""Regenerate tests/golden/projection.npz: sklearn's outputs on the cases of tests/projection_cases.py, so that the
GPU tests of ava_amd.projection do not need scikit-learn.

``<name>_knn_idx``  ``NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)`` indices of the tie-free kNN cases
                    (``projection_cases.GOLDEN_CASES``; X float32 as UMAP casts it)
``<name>_pca``      ``PCA(n_components=2, copy=False, random_state=42).fit_transform(X)`` of
                    ``projection_cases.PCA_CASES`` (the float32 case as float64)
``trust_*``         ``sklearn.manifold.trustworthiness`` of two fixed embeddings, for the numpy restatement

The inputs are regenerated from their hash salts.  Needs scikit-learn; run from the repository root:
    python tests/golden/make_golden_projection.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import projection_cases as PC                                 # noqa: E402
from sklearn.decomposition import PCA                         # noqa: E402
from sklearn.manifold import trustworthiness                  # noqa: E402
from sklearn.neighbors import NearestNeighbors                # noqa: E402


def main():
    out = {}
    for name in PC.GOLDEN_CASES:
        X, k = PC.golden_input(name)
        idx = NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X, return_distance=False)
        want, _ = PC.knn(X, k)
        assert np.array_equal(idx, want), name
        out[name + "_knn_idx"] = idx.astype(np.int32)
    for name in PC.PCA_CASES:
        X = PC.pca_input(name).astype(np.float64)
        out[name + "_pca"] = PCA(n_components=2, copy=False, random_state=42).fit_transform(X)
    X, labels = PC.blobs(n=300, d=16, c=3, salt=9120)
    Y = np.stack([labels + 0.3 * np.sin(np.arange(300)), np.cos(np.arange(300))], 1)
    out["trust_X"], out["trust_Y"] = X, Y
    out["trust_10"] = np.float64(trustworthiness(X, Y, n_neighbors=10))
    path = os.path.join(ROOT, "tests", "golden", "projection.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
