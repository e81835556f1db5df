#!/usr/bin/env python3
"""Throughput of the MMD^2 kernels (csrc/mmd.hip) next to the numpy oracle and the reference-style Python double loop.
GPU box:  python tools/mmd_bench.py [--n 20000] [--z 32]
          python tools/mmd_bench.py --matrix C N_PER [--z 32] [--reps 3]
--matrix: the whole condition-by-condition matrix of C conditions of N_PER rows each, the per-pair loop
(mmd.mmd2_matrix) against the one-pass launch sequence (mmd.mmd2_matrix_one_pass) on the same device-resident latents:
five rounds, the two alternating, each round the median of --reps calls (host clock, device synchronised before every
stop); one JSON line with the median and the spread (max - min) of the five round medians of each, the ratio, the
one-pass workspace size and the largest absolute difference between the two matrices."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ava_amd import mmd, synthetic as syn
from oracle import mmd_oracle as MO

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000)
ap.add_argument("--z", type=int, default=32)
ap.add_argument("--matrix", type=int, nargs=2, metavar=("C", "N_PER"))
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
n, z = a.n, a.z


def matrix_bench(C, n_per, z, reps):
    N = C * n_per
    condition = np.arange(N) % C                                 # interleaved rows: every index list is a gather
    latent = syn.gauss(N * z, 31).reshape(N, z) + 0.05 * condition[:, None]
    sigma = float(np.sqrt(z))
    L = mmd._latent_dev(latent)
    paths = {"loop": mmd.mmd2_matrix, "one_pass": mmd.mmd2_matrix_one_pass}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(L, condition, sigma=sigma)[0]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    out = {k: timed(fn)[1] for k, fn in paths.items()}           # warm-up of both paths at the timed shape
    rounds = {k: [] for k in paths}
    for _ in range(5):
        for k, fn in paths.items():
            rounds[k].append(float(np.median([timed(fn)[0] for _ in range(reps)])))
    plan = mmd._group_plan(condition)
    res = {"matrix": [C, n_per], "z": z, "reps_per_round": reps,
           "workspace_bytes": (int(plan["blocks"][-1, 1]) + 8) * 8, "tiles": int(plan["blocks"][-1, 0]),
           "max_abs_diff": float(np.abs(out["loop"] - out["one_pass"]).max())}
    for k, r in rounds.items():
        res[k + "_median_s"] = round(float(np.median(r)), 6)
        res[k + "_spread_s"] = round(max(r) - min(r), 6)
        res[k + "_rounds_s"] = [round(v, 6) for v in r]
    res["ratio_loop_over_one_pass"] = round(res["loop_median_s"] / res["one_pass_median_s"], 3)
    res["one_pass_faster_in_every_round"] = max(rounds["one_pass"]) < min(rounds["loop"])
    print(json.dumps(res))


if a.matrix:
    matrix_bench(a.matrix[0], a.matrix[1], z, a.reps)
    sys.exit(0)
latent = syn.gauss(2 * n * z, 31).reshape(2 * n, z)
latent[n:] += 0.3
i1, i2 = np.arange(n), n + np.arange(n)
sigma = float(np.sqrt(z))
L = mmd._latent_dev(latent)
mmd._terms(L, i1[:128], i2[:128], sigma)                       # warm-up / attribute set-up
torch.cuda.synchronize()
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    got = mmd._terms(L, i1, i2, sigma)
    ts.append(time.perf_counter() - t0)
pairs = n * (n - 1) + n * n                                      # kernel evaluations: two upper triangles + the cross term
gpu = min(ts)
# CPU references on a sample that finishes in seconds
m = min(n, 1500)
t0 = time.perf_counter(); want = MO.estimate_mmd2_terms(latent, i1[:m], i2[:m], sigma); cpu_np = time.perf_counter() - t0
mm = min(n, 120)
A = -0.5 / sigma ** 2
t0 = time.perf_counter()
t3 = 0.0
for i in range(mm):
    for j in range(mm):
        t3 += np.exp(A * np.sum(np.power(latent[i1[i]] - latent[i2[j]], 2)))
cpu_loop = time.perf_counter() - t0
sub = mmd._terms(L, i1[:m], i2[:m], sigma)
print(json.dumps({"n_per_condition": n, "z": z, "gpu_s": round(gpu, 5), "gpu_pairs_per_s": pairs / gpu,
                  "gpu_kernel_flops_per_s": pairs * (3 * z + 20) / gpu,
                  "numpy_oracle_pairs_per_s": (m * (m - 1) + m * m) / cpu_np,
                  "reference_python_loop_pairs_per_s": mm * mm / cpu_loop,
                  "max_rel_err_vs_oracle": float(max(abs(g - w) / max(abs(w), 1e-3) for g, w in zip(sub, want))),
                  "mmd2": float(got[3])}))
