"""Silhouette coefficients (ava_amd.cluster_metrics, row f21) at shotgun-dataset scale: N latent rows of d columns from
ava_amd.synthetic in K blobs, labelled by blob.  Prints one JSON line per configuration (and appends it to ``--out``):

* ``samples_ms``: host clock around ``silhouette_samples`` on rows already resident in HBM, ending in the copy of the
  coefficients to the host (the labels are encoded and sorted on the host inside it); the best of ``--repeats`` calls
  after a warm-up call.
* ``sums_ms``: HIP-event time of the ``ava_sil_cluster_sums`` call alone (the gather and the tile launch) into
  preallocated buffers, mean of ``--repeats`` calls after a warm-up; ``sums_tflops`` counts 3 d + 1 flop per ordered
  pair (a subtraction and a fused multiply-add per feature, one square root) and ``sums_share_of_fp64_vector_peak``
  holds it against ``--vector-tflops`` (78.6 by default: the fp64 vector peak taken as half the chip's 157.3 TFLOP/s
  fp32 vector rate; the bound of this kernel is arithmetic, its bytes are N d per row tile out of L2).
* ``--variant-lib PATH``: the same call through another build of the library (a scratch copy of silhouette.hip without
  the square root, which is not shipped: replace ``sqrt(acc[i][j])`` in ``sil_sums_kernel`` by ``acc[i][j]`` and build the
  copy alone with ``hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on -shared``): ``variant_sums_ms``
  and ``sqrt_share`` = 1 - variant / shipped.
* ``--sklearn N``: sklearn's ``silhouette_samples`` on the CPU on the float64 copy of the same rows (wall clock, the
  threads the environment allows), and the device's ``samples_ms`` at that N, for context.

    python tools/cluster_metrics_bench.py [--n 20000 100000] [--d 32] [--k 8] [--repeats 3]
    python tools/cluster_metrics_bench.py --sklearn 20000
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VECTOR_TFLOPS = 78.6       # taken as the MI355X fp64 vector peak: half its 157.3 TFLOP/s fp32 vector rate


def rows(n, d, k):
    """n latent rows in k Gaussian blobs (float32) and their blob labels"""
    from ava_amd import synthetic as syn
    centres = 4.0 * syn.gauss(k * d, 7400).reshape(k, d)
    labels = np.arange(n) % k
    return (centres[labels] + syn.gauss(n * d, 7401 + n).reshape(n, d)).astype(np.float32), labels.astype(np.int64)


def _events_ms(fn, repeats):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / repeats


def _sums_call(lib, xd, order, off, S, ws, nbytes, k):
    from ava_amd import _lib
    n, d = xd.shape
    fn = lib.ava_sil_cluster_sums
    fn.restype, fn.argtypes = _lib.SIGNATURES["ava_sil_cluster_sums"]

    def call():
        _lib.check(fn(xd.data_ptr(), 0, n, d, k, order.data_ptr(), off.data_ptr(), S.data_ptr(), ws.data_ptr(), nbytes,
                      _lib.stream()), "ava_sil_cluster_sums")
    return call


def measure(n, d, k, repeats, vector_tflops, variant_lib):
    import torch
    from ava_amd import _lib
    from ava_amd import cluster_metrics as CM
    X, labels = rows(n, d, k)
    xd = torch.from_numpy(X).cuda()
    CM.silhouette_samples(xd, labels)                                   # warm-up: every kernel once
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = CM.silhouette_samples(xd, labels)
        best = min(best, time.perf_counter() - t0)
    enc, kk = CM._encode(labels, n, CM.MAX_K)
    order, off = (torch.from_numpy(a).cuda() for a in CM._tables(enc, kk))
    ws, nbytes = CM._workspace(n, d, kk, xd.device)
    S = torch.empty((n, kk), dtype=torch.float64, device=xd.device)
    call = _sums_call(_lib.load(), xd, order, off, S, ws, nbytes, kk)
    call()
    sums_ms = _events_ms(call, repeats)
    flop = float(n) * n * (3 * d + 1)
    out = {"mode": "device", "N": n, "d": d, "K": kk, "samples_ms": round(best * 1e3, 3), "sums_ms": round(sums_ms, 3),
           "sums_tflops": round(flop / (sums_ms * 1e-3) / 1e12, 3),
           "sums_share_of_fp64_vector_peak": round(flop / (sums_ms * 1e-3) / 1e12 / vector_tflops, 4),
           "fp64_vector_peak_tflops": vector_tflops, "workspace_mb": round(nbytes / 2 ** 20, 1),
           "mean_silhouette": float(s.mean())}
    if variant_lib:
        S2 = torch.empty_like(S)
        vcall = _sums_call(ctypes.CDLL(os.path.abspath(variant_lib)), xd, order, off, S2, ws, nbytes, kk)
        vcall()
        # alternate the two builds: the clock the chip holds drifts over a run
        pairs = [(_events_ms(call, 1), _events_ms(vcall, 1)) for _ in range(max(repeats, 3))]
        shipped, variant = (float(np.mean([p[i] for p in pairs])) for i in (0, 1))
        out.update({"variant_lib": os.path.basename(variant_lib), "shipped_sums_ms_alternating": round(shipped, 3),
                    "variant_sums_ms": round(variant, 3), "sqrt_share": round(1.0 - variant / shipped, 4)})
    return out


def sklearn_compare(n, d, k, repeats):
    import torch
    from sklearn.metrics import silhouette_samples
    from ava_amd import cluster_metrics as CM
    X, labels = rows(n, d, k)
    xd = torch.from_numpy(X).cuda()
    CM.silhouette_samples(xd, labels)
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = CM.silhouette_samples(xd, labels)
        best = min(best, time.perf_counter() - t0)
    X64 = X.astype(np.float64)
    t0 = time.perf_counter()
    sk = silhouette_samples(X64, labels)
    sk_s = time.perf_counter() - t0
    return {"mode": "sklearn", "N": n, "d": d, "K": k, "device_samples_ms": round(best * 1e3, 3),
            "sklearn_cpu_wall_s": round(sk_s, 3), "max_abs_difference": float(np.abs(s - sk).max()),
            "cpu_threads": os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--vector-tflops", type=float, default=FP64_VECTOR_TFLOPS)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--sklearn", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cluster_metrics_bench.py measures on the MI355X: no GPU found")
    if a.sklearn:
        results = [sklearn_compare(a.sklearn, a.d, a.k, a.repeats)]
    else:
        results = [measure(n, a.d, a.k, a.repeats, a.vector_tflops, a.variant_lib) for n in a.n]
    for r in results:
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
