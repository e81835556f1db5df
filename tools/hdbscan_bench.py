"""HDBSCAN (ava_amd.hdbscan, row f23) at shotgun-dataset scale: N latent rows of d columns from ava_amd.synthetic in K
blobs, resident in HBM.  Prints one JSON line per N (and appends it to ``--out``, by default
``profiles/f23_hdbscan/hdbscan_bench.jsonl``).  Every time is the best of ``--repeats`` calls after a warm-up call, taken
twice: ``*_ms`` from HIP events around the call, ``*_host_ms`` from the host clock around the call and a synchronisation.

* ``core``: the core-distance step (the exact kNN of ``projection`` for ``min_samples`` neighbours, then ``ava_hd_core``).
* ``rowmin_ms``: every Boruvka round's row-minimum launch (device events inside ``ava_hd_mst``; per round the least of
  the repeats) and ``rounds`` their number.
* ``mst``: ``ava_hd_mst`` and the sort of its edges by key.
* ``tail``: the host tree tail ``ava_hd_tree`` (host clock only).
* ``fit``: ``HDBSCAN(min_cluster_size, min_samples).fit`` on the device tensor, ending with the labels on the host.
* ``db_counts``: ``ava_db_counts`` (row f22) at the same N and d, in the same run.  It walks half the pairs, an unskipped
  round forms all of them, so the yardstick for one round is 2 x that pass: ``rowmin_over_2counts`` are the ratios.
* ``--order blocked`` puts every blob's rows in one run of rows (the default interleaves the blobs row by row): the
  tile skip needs 64-row blocks that lie inside one component, which interleaved rows never give it.
* ``--sklearn N``: sklearn's ``HDBSCAN(algorithm='brute')`` on the CPU on the float64 copy of the same rows (wall
  clock), if scikit-learn is installed, for context.

    python tools/hdbscan_bench.py [--n 20000 100000] [--d 32] [--k 8] [--min-cluster-size 25] [--min-samples 10]
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "f23_hdbscan", "hdbscan_bench.jsonl")

from dbscan_bench import best_of, rows  # noqa: E402


def measure(n, d, k, min_cluster_size, min_samples, repeats, sklearn_n, order):
    import torch
    from ava_amd import _lib
    from ava_amd import hdbscan as HD
    lib = _lib.load()
    X, blob = rows(n, d, k)
    if order == "blocked":                                                # every blob's rows in one run of rows
        X = np.ascontiguousarray(X[np.argsort(blob, kind="stable")])
    xd = torch.from_numpy(X).cuda()
    st = _lib.stream()
    out = {"mode": "device", "N": n, "d": d, "K": k, "min_cluster_size": min_cluster_size, "min_samples": min_samples,
           "order": order, "repeats": repeats}

    def timed(name, fn):
        out[name + "_ms"], out[name + "_host_ms"] = best_of(fn, repeats)

    timed("core", lambda: HD._core_device(xd, min_samples, 'euclidean'))
    core = HD._core_device(xd, min_samples, 'euclidean')
    per_round = []

    def mst():
        ms = []
        res = HD._mst_device(xd, core, 'euclidean', timings=ms)
        per_round.append(ms)
        return res
    timed("mst", mst)
    ei, ej, ew, em, rounds = mst()
    out["rounds"] = rounds
    out["rowmin_ms"] = [round(min(r[i] for r in per_round), 3) for i in range(rounds)]
    mst_host, core_host, _ = HD._mst_host(xd, min_samples, 'euclidean')
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        labels, prob, count, _ = HD._tree_host(mst_host, n, min_cluster_size, 'eom')
        t.append((time.perf_counter() - t0) * 1e3)
    out["tail_host_ms"] = round(min(t), 3)
    model = HD.HDBSCAN(min_cluster_size, min_samples=min_samples)
    timed("fit", lambda: model.fit(xd))
    assert np.array_equal(model.labels_, labels)
    out.update({"n_clusters": int(count), "noise_share": round(float((labels == -1).mean()), 4)})
    # the yardstick: the neighbour-count pass of row f22 over the same tile, half the pairs
    eps = np.asarray([float(np.median(core_host))], dtype=np.float64)
    counts = torch.empty((1, n), dtype=torch.int32, device=xd.device)
    timed("db_counts", lambda: _lib.check(lib.ava_db_counts(xd.data_ptr(), 0, n, d, eps.ctypes.data, 1, counts.data_ptr(),
                                                            st), "ava_db_counts"))
    out["rowmin_over_2counts"] = [round(r / (2.0 * out["db_counts_ms"]), 3) for r in out["rowmin_ms"]]
    out["rowmin_sum_ms"] = round(sum(out["rowmin_ms"]), 3)
    out["mst_over_2counts"] = round(out["mst_ms"] / (2.0 * out["db_counts_ms"]), 3)
    if sklearn_n == n:
        try:
            from sklearn.cluster import HDBSCAN
        except ImportError:
            out["sklearn_cpu_wall_s"] = None
        else:
            t0 = time.perf_counter()
            sk = HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, algorithm="brute",
                         copy=True).fit(X.astype(np.float64))
            out["sklearn_cpu_wall_s"] = round(time.perf_counter() - t0, 3)
            out["sklearn_rows_differing"] = int((partition(sk.labels_) != partition(labels)).sum())
    return out


def partition(labels):
    """the partition renumbered by each part's smallest member"""
    labels = np.asarray(labels)
    first = {}
    return np.asarray([-1 if l < 0 else first.setdefault(l, i) for i, l in enumerate(labels.tolist())])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--min-cluster-size", type=int, default=25)
    ap.add_argument("--min-samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn", type=int, default=0)
    ap.add_argument("--order", choices=("interleaved", "blocked"), default="interleaved")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hdbscan_bench.py measures on the MI355X: no GPU found")
    for n in a.n:
        line = json.dumps(measure(n, a.d, a.k, a.min_cluster_size, a.min_samples, a.repeats, a.sklearn, a.order))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
