"""Regenerates tests/golden/spectral.npz with scikit-learn 1.7.2 (run from the repository root):
``SpectralEmbedding(affinity='precomputed').fit_transform`` on the graphs of ``spectral_cases.EMBED_CASES`` and
``SpectralClustering(affinity='nearest_neighbors').fit_predict`` on the rows of ``spectral_cases.CLUSTER_CASES``.  It
refuses cases that do not meet the gap condition or that sklearn does not cluster with an adjusted Rand index of 1."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import spectral_cases as SC  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import SpectralClustering
    from sklearn.manifold import SpectralEmbedding
    from sklearn.metrics import adjusted_rand_score
    out = {"sklearn_version": np.array(sklearn.__version__)}
    warnings.simplefilter("ignore")
    for i, (name, k) in enumerate(SC.EMBED_CASES):
        A = SC.case_graph(name)
        c, _ = SC.components(A)
        lam = SC.dense_spectrum(A)[0]
        assert SC.gaps(lam, c, k + 1) >= SC.MIN_GAP, (name, SC.gaps(lam, c, k + 1))
        Y = SpectralEmbedding(n_components=k, affinity='precomputed', random_state=0).fit_transform(A)
        out["e%d_Y" % i] = np.asarray(Y, dtype=np.float64)
    for i, name in enumerate(SC.CLUSTER_CASES):
        X, truth, k = SC.cluster_rows(name)
        labels = SpectralClustering(n_clusters=k, affinity='nearest_neighbors', n_neighbors=SC.BLOB_K,
                                    random_state=0).fit_predict(X)
        assert adjusted_rand_score(truth, labels) == 1.0, name
        out["l%d" % i] = labels.astype(np.int32)
    path = os.path.join(HERE, "spectral.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
