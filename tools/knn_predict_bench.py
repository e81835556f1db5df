"""Cross-validated kNN prediction (ava_amd.knn_predict, row f24) at shotgun-dataset scale: N latent rows of d columns from
ava_amd.synthetic in K blobs, resident in HBM, 5 folds, kmax = 32 and an 8-value sweep of k.  Prints one JSON line per N
(and appends it to ``--out``, by default ``profiles/f24_knn_predict/knn_predict_bench.jsonl``).  Every time is the best of
``--repeats`` calls after a warm-up call, taken twice: ``*_ms`` from HIP events around the call, ``*_host_ms`` from the
host clock around the call and a synchronisation.

* ``masked_interleaved``: the masked neighbour pass ``ava_kp_knn_masked`` at kmax with fold = row % 5: no tile lies in one
  fold, nothing is skipped.
* ``masked_sorted``: the same pass with the folds of ``kfold(N, 5)``, five runs of rows: about one tile in five lies in
  the fold of its queries and is skipped.  ``sorted_over_interleaved`` is the ratio; above 1 the skip would be wrong.
* ``plain``: ``ava_pj_knn`` at the same N, d and k in the same run, the yardstick; ``masked_over_plain`` is
  ``masked_interleaved`` over it.
* ``vote_*`` / ``regress_*``: one ``ava_kp_vote`` / ``ava_kp_regress`` launch over the whole sweep (K classes; 12
  outputs), for both weightings.
* ``accuracy`` / ``r2``: the pooled scores at every k under uniform weights, for the record.
* ``--sklearn N``: sklearn's ``cross_val_predict(KNeighborsClassifier(algorithm='brute'), cv=PredefinedSplit)`` over the
  same sweep on the CPU on the float64 copy of the same rows (wall clock, all k), if scikit-learn is installed, for
  context, and the number of rows whose class differs at any k.

    python tools/knn_predict_bench.py [--n 20000 100000] [--d 32] [--k 8] [--kmax 32] [--folds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEFAULT_OUT = os.path.join(ROOT, "profiles", "f24_knn_predict", "knn_predict_bench.jsonl")
N_OUT = 12

from dbscan_bench import best_of, rows  # noqa: E402


def sweep_of(kmax):
    """8 ascending values of k ending at kmax (fewer when kmax is small)"""
    return sorted({max(1, int(round(kmax * f))) for f in (1 / 32, 1 / 16, 3 / 32, 5 / 32, 1 / 4, 3 / 8, 5 / 8, 1.0)})


def measure(n, d, k, kmax, n_folds, repeats, sklearn_n):
    import torch
    from ava_amd import _lib
    from ava_amd import knn_predict as KP
    from ava_amd import projection as PJ
    X, blob = rows(n, d, k)
    xd = torch.from_numpy(X).cuda()
    ks = np.asarray(sweep_of(kmax), dtype=np.int32)
    interleaved = np.arange(n, dtype=np.int64) % n_folds
    folds = {"interleaved": torch.from_numpy(interleaved.astype(np.int32)).cuda(),
             "sorted": torch.from_numpy(KP.kfold(n, n_folds).astype(np.int32)).cuda()}
    yd = torch.from_numpy(blob.astype(np.int32)).cuda()
    Yd = xd[:, :min(N_OUT, d)].to(torch.float64).contiguous()
    out = {"mode": "device", "N": n, "d": d, "K": k, "kmax": kmax, "folds": n_folds, "sweep": ks.tolist(),
           "n_out": int(Yd.shape[1]), "repeats": repeats}

    def timed(name, fn):
        out[name + "_ms"], out[name + "_host_ms"] = best_of(fn, repeats)

    for order, fold in folds.items():
        timed("masked_" + order, lambda: KP._masked_device(xd, fold, kmax))
    timed("plain", lambda: PJ._knn_device(xd, kmax, KP._KNN_CHUNK))
    out["masked_over_plain"] = round(out["masked_interleaved_ms"] / out["plain_ms"], 3)
    out["sorted_over_interleaved"] = round(out["masked_sorted_ms"] / out["masked_interleaved_ms"], 3)
    idx, dist = KP._masked_device(xd, folds["interleaved"], kmax)
    for weighted, weights in enumerate(("uniform", "distance")):
        timed("vote_" + weights, lambda: KP._vote_device(idx, dist, yd, ks, weighted))
        timed("regress_" + weights, lambda: KP._regress_device(idx, dist, Yd, ks, weighted))
    pred = KP._vote_device(idx, dist, yd, ks, 0)
    out["accuracy"] = [round(float(v), 4) for v in (pred == yd[None, :]).double().mean(dim=1).cpu()]
    val = KP._regress_device(idx, dist, Yd, ks, 0)
    out["r2"] = [round(KP._r2(Yd, val[a]), 4) for a in range(len(ks))]
    timed("cross_val_predict", lambda: KP.cross_val_predict(xd, blob, interleaved, n_neighbors=ks.tolist()))
    if sklearn_n == n:
        try:
            from sklearn.model_selection import PredefinedSplit, cross_val_predict
            from sklearn.neighbors import KNeighborsClassifier
        except ImportError:
            out["sklearn_cpu_wall_s"] = None
        else:
            X64, cv = X.astype(np.float64), PredefinedSplit(interleaved)
            t0 = time.perf_counter()
            sk = np.stack([cross_val_predict(KNeighborsClassifier(int(kk), algorithm="brute"), X64, blob, cv=cv)
                           for kk in ks])
            out["sklearn_cpu_wall_s"] = round(time.perf_counter() - t0, 3)
            out["sklearn_rows_differing"] = int((sk != pred.cpu().numpy()).any(axis=0).sum())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--kmax", type=int, default=32)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn", type=int, default=0)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("knn_predict_bench.py measures on the MI355X: no GPU found")
    for n in a.n:
        line = json.dumps(measure(n, a.d, a.k, a.kmax, a.folds, a.repeats, a.sklearn))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
