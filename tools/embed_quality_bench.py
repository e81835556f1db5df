"""Embedding quality (ava_amd.embedding_quality, row f26) at repertoire scale: N latent rows X of d columns from
ava_amd.synthetic in 8 blobs and Y, their ``pca_projection`` plus 0.3 noise, both resident in HBM.  Prints one JSON line
per N (and appends it to ``--out``, by default ``profiles/f26_embed_quality/embed_quality_bench.jsonl``).  Every device
time is the median of ``--repeats`` windows after a warm-up window, from HIP events around the window; ``*_spread`` is
(max - min) / median over the windows, the run-to-run noise a difference has to exceed.  All of one line is timed in one
run, so its ratios are within one run.

* ``ranks_x_m15_ms`` / ``ranks_x_m63_ms``: ``ava_eq_ranks`` in X of the 15 / 63 nearest rows in Y (the trustworthiness
  pass), the target check and its host read included; ``ranks_y_m15_ms`` / ``ranks_y_m63_ms``: the same in Y of the
  neighbours in X (the continuity pass, d = 2).
* ``knn_x_ms`` / ``knn_y_ms``: the two ``ava_pj_knn`` passes at k = 64.
* ``penalties_ms`` / ``overlap_ms``: ``ava_eq_penalties`` and ``ava_eq_overlap`` at m = 63 over ``--ks``.
* ``curve_ms``: a whole ``quality_curve(X, Y, ks)`` on the resident rows (host clock around the call, host reads
  included).
* ``sil_sums_ms``: the yardstick, ``ava_sil_cluster_sums`` at the same N and d with the 8 blob labels: the full N^2
  pass over the same tile.  ``ranks_x_m15_over_sil`` is the ratio the issue of row f26 asks about (expectation: at most
  1.5).
* with ``--sklearn N`` (0: none): ``sklearn_trust_s``, sklearn's ``trustworthiness`` on the CPU on the first N rows at
  k = 15 (host clock, one run), and ``device_trust_s``, ``trustworthiness`` here on the same rows with the upload.

    python tools/embed_quality_bench.py [--n 20000 100000] [--d 32] [--sklearn 10000]
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "f26_embed_quality", "embed_quality_bench.jsonl")
BLOBS = 8

from dbscan_bench import rows  # noqa: E402
from kmeans_bench import windows  # noqa: E402


def measure(n, d, ks, repeats, n_sklearn):
    import torch
    from ava_amd import _lib
    from ava_amd import cluster_metrics as CM
    from ava_amd import embedding_quality as EQ
    from ava_amd import projection as PJ
    lib = _lib.load()
    X, labels = rows(n, d, BLOBS)
    Y = (PJ.pca_projection(X) + 0.3 * np.random.RandomState(n).standard_normal((n, 2))).astype(np.float32)
    xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    out = {"mode": "device", "N": n, "d": d, "ks": ks, "repeats": repeats}

    out["knn_x_ms"], out["knn_x_spread"] = windows(lambda: PJ._knn_device(xd, PJ.MAX_K), repeats)
    out["knn_y_ms"], out["knn_y_spread"] = windows(lambda: PJ._knn_device(yd, PJ.MAX_K), repeats)
    nx, ny = EQ._neighbours_device(xd, EQ.MAX_NEIGHBORS), EQ._neighbours_device(yd, EQ.MAX_NEIGHBORS)
    for m in (15, 63):
        tx, ty = nx[:, :m].contiguous(), ny[:, :m].contiguous()
        key = "ranks_x_m%d" % m
        out[key + "_ms"], out[key + "_spread"] = windows(lambda: EQ._ranks_device(xd, ty), repeats)
        key = "ranks_y_m%d" % m
        out[key + "_ms"], out[key + "_spread"] = windows(lambda: EQ._ranks_device(yd, tx), repeats)
    rank = EQ._ranks_device(xd, ny)
    out["rank_x_mean"] = round(float(rank.double().mean()), 1)
    out["rank_x_max"] = int(rank.max())
    out["penalties_ms"], out["penalties_spread"] = windows(lambda: EQ._penalties_device(rank, ks), repeats)
    out["overlap_ms"], out["overlap_spread"] = windows(lambda: EQ._overlap_device(nx, ny, ks), repeats)

    enc, kk = CM._encode(labels, n, CM.MAX_K)
    order, off = (torch.from_numpy(a).cuda() for a in CM._tables(enc, kk))
    ws, nbytes = CM._workspace(n, d, kk, xd.device)
    S = torch.empty((n, kk), dtype=torch.float64, device=xd.device)

    def sil():
        _lib.check(lib.ava_sil_cluster_sums(xd.data_ptr(), _lib.dtype_code(xd), n, d, kk, order.data_ptr(), off.data_ptr(),
                                            S.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "ava_sil_cluster_sums")

    out["sil_sums_ms"], out["sil_sums_spread"] = windows(sil, repeats)
    out["ranks_x_m15_over_sil"] = round(out["ranks_x_m15_ms"] / out["sil_sums_ms"], 3)
    out["ranks_x_m63_over_sil"] = round(out["ranks_x_m63_ms"] / out["sil_sums_ms"], 3)
    out["ranks_x_m15_over_knn_x"] = round(out["ranks_x_m15_ms"] / out["knn_x_ms"], 3)

    curves = []
    for _ in range(1 + min(repeats, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cur = EQ.quality_curve(xd, yd, ks)
        torch.cuda.synchronize()
        curves.append((time.perf_counter() - t0) * 1e3)
    out["curve_ms"] = round(float(np.median(curves[1:])), 2)
    for key in ("trustworthiness", "continuity", "preservation"):
        out[key] = [round(float(v), 6) for v in cur[key]]

    if n_sklearn:
        from sklearn.manifold import trustworthiness
        ns = min(n, n_sklearn)
        Xs, Ys = X[:ns], Y[:ns]
        t0 = time.perf_counter()
        ref = float(trustworthiness(Xs, Ys, n_neighbors=15))
        out["sklearn_N"], out["sklearn_trust_s"] = ns, round(time.perf_counter() - t0, 3)
        EQ.trustworthiness(Xs, Ys, n_neighbors=15)
        t0 = time.perf_counter()
        got = EQ.trustworthiness(Xs, Ys, n_neighbors=15)
        out["device_trust_s"] = round(time.perf_counter() - t0, 4)
        out["sklearn_trust"], out["device_trust"] = ref, got
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", nargs="+", type=int, default=[20000, 100000])
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--ks", nargs="+", type=int, default=[5, 15, 30, 63])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sklearn", type=int, default=10000, help="rows of the sklearn run on the CPU (0: none)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("embed_quality_bench.py measures on the MI355X: no GPU found")
    for i, n in enumerate(a.n):
        line = json.dumps(measure(n, a.d, a.ks, a.repeats, a.sklearn if i == 0 else 0))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
