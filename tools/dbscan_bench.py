"""DBSCAN (ava_amd.dbscan, row f22) at shotgun-dataset scale: N latent rows of d columns from ava_amd.synthetic in K
blobs, resident in HBM, at the radius where about ``--core`` of the rows are core rows (the ``min_samples``-th distance's
quantile, from ``k_distances``).  Prints one JSON line per N (and appends it to ``--out``, by default
``profiles/f22_dbscan/dbscan_bench.jsonl``).  Every time is the best of ``--repeats`` calls after a warm-up call, taken
twice: ``*_ms`` from HIP events around the call, ``*_host_ms`` from the host clock around the call and a synchronisation.

* ``counts``, ``union``, ``assign``: the three distance passes alone through the C entry points into preallocated
  buffers: ``ava_db_counts``; ``ava_db_union`` (parent initialisation, the union pass, the flatten);
  ``ava_db_assign`` (the border pass, the scan and the relabel).
* ``fit``: ``DBSCAN(eps, min_samples).fit`` on the device tensor, ending with the labels on the host.
* ``sweep8`` / ``fits8``: ``dbscan_sweep`` over 8 radii from 0.85 to 1.15 of that radius, against 8 single fits.
* ``sil_sums``: ``ava_sil_cluster_sums`` (row f21) at the same N and d with the K blob labels: the comparable full N^2
  pass over the same distance tile, with a square root per pair.  ``*_over_sil_sums`` are the ratios to it.
* ``--sklearn N``: sklearn's ``DBSCAN(algorithm='brute')`` on the CPU on the float64 copy of the same rows (wall clock,
  the threads the environment allows), if scikit-learn is installed, for context.

    python tools/dbscan_bench.py [--n 20000 100000] [--d 32] [--k 8] [--min-samples 10] [--core 0.7] [--repeats 5]
    python tools/dbscan_bench.py --n 100000 --core 0.98          # a denser setting: about 500 neighbours per row
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "f22_dbscan", "dbscan_bench.jsonl")


def rows(n, d, k):
    """n latent rows in k Gaussian blobs (float32) and their blob labels"""
    from ava_amd import synthetic as syn
    centres = 4.0 * syn.gauss(k * d, 7400).reshape(k, d)
    labels = np.arange(n) % k
    return (centres[labels] + syn.gauss(n * d, 7401 + n).reshape(n, d)).astype(np.float32), labels.astype(np.int64)


def best_of(fn, repeats):
    """(best HIP-event ms, best host-clock ms) of ``repeats`` calls after one warm-up call"""
    import torch
    fn()
    ev, host = float("inf"), float("inf")
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        host = min(host, (time.perf_counter() - t0) * 1e3)
        ev = min(ev, e0.elapsed_time(e1))
    return round(ev, 3), round(host, 3)


def measure(n, d, k, min_samples, core_share, repeats, sklearn_n):
    import torch
    from ava_amd import _lib
    from ava_amd import cluster_metrics as CM
    from ava_amd import dbscan as DB
    lib = _lib.load()
    X, blob = rows(n, d, k)
    xd = torch.from_numpy(X).cuda()
    eps = float(DB.k_distances(xd, min_samples)[int(core_share * n)])
    radii = np.asarray([eps], dtype=np.float64)
    st = _lib.stream()
    counts = torch.empty((1, n), dtype=torch.int32, device=xd.device)
    nbytes = lib.ava_db_workspace_bytes(n, d, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xd.device)
    labels = torch.empty((1, n), dtype=torch.int64, device=xd.device)
    core = torch.empty((1, n), dtype=torch.uint8, device=xd.device)
    ncl = torch.empty(1, dtype=torch.int32, device=xd.device)
    head = (xd.data_ptr(), 0, n, d, radii.ctypes.data, 1)
    out = {"mode": "device", "N": n, "d": d, "K": k, "min_samples": min_samples, "eps": eps, "repeats": repeats}

    def timed(name, fn):
        out[name + "_ms"], out[name + "_host_ms"] = best_of(fn, repeats)

    timed("counts", lambda: _lib.check(lib.ava_db_counts(*head, counts.data_ptr(), st), "ava_db_counts"))
    timed("union", lambda: _lib.check(lib.ava_db_union(*head, min_samples, counts.data_ptr(), ws.data_ptr(), nbytes,
                                                       st), "ava_db_union"))
    timed("assign", lambda: _lib.check(lib.ava_db_assign(*head, min_samples, counts.data_ptr(), core.data_ptr(),
                                                         labels.data_ptr(), ncl.data_ptr(), ws.data_ptr(), nbytes, st),
                                       "ava_db_assign"))
    lab = labels[0].cpu().numpy()
    out.update({"core_share": round(float(core.float().mean().item()), 4), "n_clusters": int(ncl.item()),
                "noise_share": round(float((lab == -1).mean()), 4),
                "mean_neighbours": round(float(counts.float().mean().item()), 1)})
    model = DB.DBSCAN(eps, min_samples=min_samples)
    timed("fit", lambda: model.fit(xd))
    assert np.array_equal(model.labels_, lab)
    sweep = [float(r) for r in eps * np.linspace(0.85, 1.15, 8)]
    timed("sweep8", lambda: DB.dbscan_sweep(xd, sweep, min_samples=min_samples))
    timed("fits8", lambda: [DB.DBSCAN(r, min_samples=min_samples).fit(xd) for r in sweep])
    # the parent commit's comparable pass: the silhouette sums over the same tile
    enc, kk = CM._encode(blob, n, CM.MAX_K)
    order, off = (torch.from_numpy(a).cuda() for a in CM._tables(enc, kk))
    sws, sbytes = CM._workspace(n, d, kk, xd.device)
    S = torch.empty((n, kk), dtype=torch.float64, device=xd.device)
    timed("sil_sums", lambda: _lib.check(lib.ava_sil_cluster_sums(xd.data_ptr(), 0, n, d, kk, order.data_ptr(),
                                                                  off.data_ptr(), S.data_ptr(), sws.data_ptr(), sbytes,
                                                                  st), "ava_sil_cluster_sums"))
    for name in ("counts", "union", "assign", "fit"):
        out[name + "_over_sil_sums"] = round(out[name + "_ms"] / out["sil_sums_ms"], 3)
    out["sweep8_over_fits8"] = round(out["sweep8_host_ms"] / out["fits8_host_ms"], 3)
    out["sweep8_over_fit"] = round(out["sweep8_host_ms"] / out["fit_host_ms"], 3)
    if sklearn_n == n:
        try:
            from sklearn.cluster import DBSCAN
        except ImportError:
            out["sklearn_cpu_wall_s"] = None
        else:
            X64 = X.astype(np.float64)
            threads = min(16, int(os.environ.get("OMP_NUM_THREADS", os.cpu_count())))
            t0 = time.perf_counter()
            sk = DBSCAN(eps=eps, min_samples=min_samples, algorithm="brute", n_jobs=threads).fit(X64)
            out["sklearn_cpu_wall_s"] = round(time.perf_counter() - t0, 3)
            out["sklearn_labels_equal"] = bool(np.array_equal(sk.labels_, lab))
            out["cpu_threads"] = threads
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--min-samples", type=int, default=10)
    ap.add_argument("--core", type=float, default=0.7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn", type=int, default=0)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dbscan_bench.py measures on the MI355X: no GPU found")
    for n in a.n:
        line = json.dumps(measure(n, a.d, a.k, a.min_samples, a.core, a.repeats, a.sklearn))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
