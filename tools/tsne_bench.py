"""Exact t-SNE (ava_amd.tsne, row f19) at DataContainer scale: N latent rows of 32 columns from ava_amd.synthetic,
1000 iterations.  Prints JSON lines:

* ``fit``: the wall time of one ``TSNE(random_state=0).fit_transform`` (after a warm-up fit at N = 512), the time of the
  squared distances and of the joint probabilities (HIP events), and the time per descent iteration (HIP events around
  ``--timed-iters`` iterations enqueued in one call), with the P bytes per second that time would mean if the gradient
  pass were all of it (8 N^2 bytes per iteration; a lower bound on the pass's own rate).
* ``--iters-only K``: nothing but K descent iterations at N (the program to run under ``rocprofv3 --kernel-trace
  --stats``, in a run of its own).
* ``--kernel-stats CSV``: no GPU work; reads the profiler's ``*_kernel_stats.csv`` of such a run and prints the time per
  launch of ts_z_kernel, ts_grad_kernel (without and with the KL) and ts_update_kernel, and the gradient pass's P bytes
  per second beside the 6.29 TB/s that a float4 copy measures on this chip (MI355X, HBM3E; 8.0 TB/s nominal).
* ``--sklearn N``: sklearn's exact TSNE on the CPU at N rows, and the device at the same N (wall clock, same init).

    python tools/tsne_bench.py [--n 10000] [--d 32] [--max-iter 1000] [--timed-iters 100]
    python tools/tsne_bench.py --iters-only 100
    python tools/tsne_bench.py --kernel-stats prof/x_kernel_stats.csv [--n 10000]
    python tools/tsne_bench.py --sklearn 2000
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBPS = 6.29            # measured float4 copy on an MI355X
KERNELS = ("ts_z_kernel", "ts_grad_kernel<false>", "ts_grad_kernel<true>", "ts_update_kernel")


def rows(n, d):
    """n latent rows: 8 Gaussian blobs in d dimensions, float32"""
    from ava_amd import synthetic as syn
    centres = 4.0 * syn.gauss(8 * d, 7300).reshape(8, d)
    return (centres[np.arange(n) % 8] + syn.gauss(n * d, 7301 + n).reshape(n, d)).astype(np.float32)


def _events_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _descent_state(n, d, perplexity):
    import torch
    from ava_amd import tsne as T
    xd = torch.from_numpy(rows(n, d)).cuda()
    T.squared_distances(xd[:512])                                   # code objects loaded before anything is timed
    sq_ms, D2 = _events_ms(lambda: T.squared_distances(xd))
    joint_ms, P = _events_ms(lambda: T.joint_probabilities(D2, perplexity))
    Y = torch.from_numpy(1e-4 * np.random.RandomState(0).standard_normal((n, 2))).cuda()
    return P, Y, torch.zeros_like(Y), torch.ones_like(Y), sq_ms, joint_ms


def iters_only(n, d, perplexity, iters):
    import torch
    from ava_amd import tsne as T
    P, Y, update, gains, _, _ = _descent_state(n, d, perplexity)
    lr = max(n / 12.0 / 4.0, 50.0)
    T.descend(Y, update, gains, P, 2, 0.5, lr, 12.0)
    ms, last = _events_ms(lambda: T.descend(Y, update, gains, P, iters, 0.5, lr, 12.0))
    torch.cuda.synchronize()
    print(json.dumps({"mode": "iters-only", "N": n, "iters": iters, "ms_per_iter": round(ms / iters, 4),
                      "kl": last[0], "grad_norm": last[1]}), flush=True)


def fit(n, d, perplexity, max_iter, timed_iters):
    import torch
    from ava_amd import _lib, tsne as T
    X = rows(n, d)
    T.TSNE(random_state=0, max_iter=250).fit(X[:512])               # warm-up: every kernel once
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = T.TSNE(random_state=0, perplexity=perplexity, max_iter=max_iter)
    emb = model.fit_transform(X)
    wall = time.perf_counter() - t0
    P, Y, update, gains, sq_ms, joint_ms = _descent_state(n, d, perplexity)
    lr = model.learning_rate_
    T.descend(Y, update, gains, P, 2, 0.5, lr, 12.0)
    ms, _ = _events_ms(lambda: T.descend(Y, update, gains, P, timed_iters, 0.5, lr, 12.0))
    per_iter = ms / timed_iters
    out = {"mode": "fit", "N": n, "d": d, "perplexity": perplexity, "max_iter": max_iter, "n_iter": model.n_iter_,
           "col_chunks": _lib.load().ava_ts_col_chunks(n), "fit_transform_wall_s": round(wall, 3),
           "kl_divergence": model.kl_divergence_, "finite": bool(np.all(np.isfinite(emb))),
           "sqdist_ms": round(sq_ms, 3), "joint_ms": round(joint_ms, 3), "ms_per_iter": round(per_iter, 4),
           "p_bytes": 8 * n * n, "p_tbps_if_all_gradient": round(8.0 * n * n / (per_iter * 1e-3) / 1e12, 3),
           "hbm_copy_tbps": HBM_COPY_TBPS}
    print(json.dumps(out), flush=True)


def kernel_stats(path, n):
    found = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name:
                    found[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    out = {"mode": "kernel-stats", "N": n, "kernels": found}
    for k, tag in (("ts_grad_kernel<false>", "grad"), ("ts_grad_kernel<true>", "grad_with_kl")):
        if k in found:
            tbps = 8.0 * n * n / (found[k]["avg_us"] * 1e-6) / 1e12
            out[tag + "_p_tbps"] = round(tbps, 3)
            out[tag + "_share_of_hbm_copy"] = round(tbps / HBM_COPY_TBPS, 3)
    out["hbm_copy_tbps"] = HBM_COPY_TBPS
    print(json.dumps(out), flush=True)


def sklearn_compare(n, d, perplexity):
    import torch
    from sklearn.manifold import TSNE as SkTSNE
    from ava_amd import tsne as T
    X = rows(n, d)
    Y0 = (1e-4 * np.random.RandomState(0).standard_normal((n, 2))).astype(np.float32)
    T.TSNE(random_state=0, max_iter=250).fit(X[:512])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = T.TSNE(perplexity=perplexity, init=Y0).fit(X)
    dev_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    sk = SkTSNE(perplexity=perplexity, method="exact", init=Y0).fit(X)
    sk_s = time.perf_counter() - t0
    print(json.dumps({"mode": "sklearn", "N": n, "d": d, "device_wall_s": round(dev_s, 3), "device_kl": dev.kl_divergence_,
                      "device_n_iter": dev.n_iter_, "sklearn_exact_cpu_wall_s": round(sk_s, 3),
                      "sklearn_kl": float(sk.kl_divergence_), "sklearn_n_iter": int(sk.n_iter_),
                      "cpu_threads": os.cpu_count() if "OMP_NUM_THREADS" not in os.environ
                      else int(os.environ["OMP_NUM_THREADS"])}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--timed-iters", type=int, default=100)
    ap.add_argument("--iters-only", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--sklearn", type=int, default=0)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.n)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench.py measures on the MI355X: no GPU found")
    if a.iters_only:
        return iters_only(a.n, a.d, a.perplexity, a.iters_only)
    if a.sklearn:
        return sklearn_compare(a.sklearn, a.d, a.perplexity)
    fit(a.n, a.d, a.perplexity, a.max_iter, a.timed_iters)


if __name__ == "__main__":
    main()
