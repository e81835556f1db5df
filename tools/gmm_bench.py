"""Gaussian mixture models (ava_amd.mixture, row f20) at shotgun-dataset scale: N latent rows of d columns from
ava_amd.synthetic, K components.  Prints one JSON line per configuration (and appends it to ``--out``):

* ``e_step_ms``, ``means_ms``, ``m_step_ms``: HIP-event times of one call of ``ava_gm_e_step`` (1 launch),
  ``ava_gm_means`` (2 launches: chunk sums, finish) and ``ava_gm_m_step`` (those 2 and the 3 covariance launches) after a
  warm-up call of each; ``cov_ms`` is their difference.
* ``ms_per_iter``: HIP events around ``--timed-iters`` EM iterations enqueued by one ``ava_gm_fit`` call with tol = 0.
* the shares the issue asks for: the E-step's and the covariance partials' fp64 multiply-adds (2 N K d^2 flop each
  for 'full', counted over the d x d products, not over the padded 16-blocks) against ``--mfma-tflops`` (the chip's fp64
  matrix peak), and the bytes every iteration has to move at least (X once per launch that reads it, resp and log_resp
  written once and resp read twice) against the measured copy rate.
* ``--sklearn N``: sklearn's GaussianMixture on the CPU for ``--sk-iters`` iterations at N rows from the same start, and
  the device for the same iterations (wall clock), for context.

    python tools/gmm_bench.py [--n 100000 1000000] [--d 32] [--k 8 32] [--cov full diag] [--timed-iters 20]
    python tools/gmm_bench.py --sklearn 100000 --k 8
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBPS = 6.29            # measured float4 copy on an MI355X (8.0 TB/s nominal)
FP64_MFMA_TFLOPS = 78.6         # MI355X fp64 matrix peak (data sheet)


def rows(n, d, blobs=8):
    """n latent rows: Gaussian blobs in d dimensions, float32"""
    from ava_amd import synthetic as syn
    centres = 4.0 * syn.gauss(blobs * d, 7400).reshape(blobs, d)
    return (centres[np.arange(n) % blobs] + syn.gauss(n * d, 7401 + n).reshape(n, d)).astype(np.float32)


def _events_ms(fn, repeats=1):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / repeats, out


def start_params(xd, k, cov_type):
    """the parameters after the 'random_from_data' start and two EM iterations (the variances of the bare start are
    reg_covar, which no later iteration looks like)"""
    from ava_amd import mixture as M
    g = M.GaussianMixture(k, covariance_type=cov_type, init_params="random_from_data", tol=0.0, max_iter=2).fit(xd)
    return g


def measure(n, d, k, cov_type, timed_iters, mfma_tflops):
    import torch
    from ava_amd import mixture as M
    xd = torch.from_numpy(rows(n, d)).cuda()
    g = start_params(xd, k, cov_type)                              # also the warm-up: every kernel once
    code = M._COV[cov_type]
    weights, means, cov, pchol, log_det = g._params
    lib, st = M._lib.load(), M._lib.stream()
    lpn, log_resp, resp = M._e_step(xd, weights, means, pchol, log_det, code)

    def only_e_step():                                             # into the same buffers: no allocation is timed
        M._lib.check(lib.ava_gm_e_step(xd.data_ptr(), 0, n, d, k, code, weights.data_ptr(), means.data_ptr(),
                                       pchol.data_ptr(), log_det.data_ptr(), lpn.data_ptr(), log_resp.data_ptr(),
                                       resp.data_ptr(), st), "ava_gm_e_step")

    only_e_step()
    e_ms, _ = _events_ms(only_e_step, 3)
    ws = M._workspace(n, d, k, code, xd.device)
    M._m_step(xd, resp, 1e-6, code, ws)
    m_ms, _ = _events_ms(lambda: M._m_step(xd, resp, 1e-6, code, ws), 3)
    nk = torch.empty(k, dtype=torch.float64, device=xd.device)
    w2, mu2 = torch.empty_like(weights), torch.empty_like(means)

    def only_means():
        M._lib.check(lib.ava_gm_means(xd.data_ptr(), 0, n, d, k, resp.data_ptr(), w2.data_ptr(), mu2.data_ptr(),
                                      nk.data_ptr(), ws[0].data_ptr(), ws[1], st), "ava_gm_means")

    only_means()
    mean_ms, _ = _events_ms(only_means, 3)
    fit = M.GaussianMixture(k, covariance_type=cov_type, tol=0.0, max_iter=timed_iters, iter_block=timed_iters)
    params = [p.clone() for p in g._params]
    it_ms, _ = _events_ms(lambda: fit._em(xd, params, ws))
    per_iter = it_ms / timed_iters
    flop = 2.0 * n * k * d * d if cov_type == "full" else 0.0
    x_bytes, r_bytes = 4.0 * n * d, 8.0 * n * k
    iter_bytes = 3 * x_bytes + 4 * r_bytes + 8.0 * n              # X: E-step, chunk sums, covariance; resp w + 2 r, log_resp w
    out = {"mode": "device", "N": n, "d": d, "K": k, "covariance_type": cov_type, "e_step_ms": round(e_ms, 4),
           "means_ms": round(mean_ms, 4), "m_step_ms": round(m_ms, 4), "cov_ms": round(m_ms - mean_ms, 4),
           "ms_per_iter": round(per_iter, 4), "timed_iters": timed_iters,
           "workspace_mb": round(ws[1] / 2 ** 20, 1),
           "iter_min_bytes": iter_bytes, "iter_share_of_hbm_copy": round(iter_bytes / (per_iter * 1e-3) / 1e12 /
                                                                         HBM_COPY_TBPS, 4),
           "hbm_copy_tbps": HBM_COPY_TBPS}
    if flop:
        out.update({"e_step_tflops": round(flop / (e_ms * 1e-3) / 1e12, 3),
                    "e_step_share_of_fp64_mfma_peak": round(flop / (e_ms * 1e-3) / 1e12 / mfma_tflops, 4),
                    "cov_tflops": round(flop / ((m_ms - mean_ms) * 1e-3) / 1e12, 3),
                    "cov_share_of_fp64_mfma_peak": round(flop / ((m_ms - mean_ms) * 1e-3) / 1e12 / mfma_tflops, 4),
                    "fp64_mfma_peak_tflops": mfma_tflops})
    return out


def sklearn_compare(n, d, k, cov_type, iters):
    import torch
    from sklearn.mixture import GaussianMixture as SK
    from ava_amd import mixture as M
    X = rows(n, d)
    xd = torch.from_numpy(X).cuda()
    g = start_params(xd, k, cov_type)
    init = dict(weights_init=g.weights_ / g.weights_.sum(), means_init=g.means_, precisions_init=g.precisions_)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = M.GaussianMixture(k, covariance_type=cov_type, tol=0.0, max_iter=iters, **init).fit(xd)
    dev_s = time.perf_counter() - t0
    X64 = X.astype(np.float64)
    t0 = time.perf_counter()
    sk = SK(k, covariance_type=cov_type, tol=0.0, max_iter=iters, **init).fit(X64)
    sk_s = time.perf_counter() - t0
    return {"mode": "sklearn", "N": n, "d": d, "K": k, "covariance_type": cov_type, "iters": iters,
            "device_wall_s": round(dev_s, 4), "sklearn_cpu_wall_s": round(sk_s, 3),
            "device_lower_bound": dev.lower_bound_, "sklearn_lower_bound": float(sk.lower_bound_),
            "cpu_threads": os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--cov", nargs="+", default=["full", "diag"])
    ap.add_argument("--timed-iters", type=int, default=20)
    ap.add_argument("--mfma-tflops", type=float, default=FP64_MFMA_TFLOPS)
    ap.add_argument("--sklearn", type=int, default=0)
    ap.add_argument("--sk-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gmm_bench.py measures on the MI355X: no GPU found")
    results = []
    if a.sklearn:
        results = [sklearn_compare(a.sklearn, a.d, k, c, a.sk_iters) for c in a.cov for k in a.k]
    else:
        results = [measure(n, a.d, k, c, a.timed_iters, a.mfma_tflops) for c in a.cov for n in a.n for k in a.k]
    for r in results:
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
