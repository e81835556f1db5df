#!/usr/bin/env python3
"""Throughput of the MMD^2 kernels (csrc/mmd.hip) next to the numpy oracle and the reference-style Python double loop.
GPU box:  python tools/mmd_bench.py [--n 20000] [--z 32]
          python tools/mmd_bench.py --matrix C N_PER [--z 32] [--reps 3]
--matrix: the whole condition-by-condition matrix of C conditions of N_PER rows each, the per-pair loop
(mmd.mmd2_matrix) against the one-pass launch sequence (mmd.mmd2_matrix_one_pass) on the same device-resident latents:
five rounds, the two alternating, each round the median of --reps calls (host clock, device synchronised before every
stop); one JSON line with the median and the spread (max - min) of the five round medians of each, the ratio, the
one-pass workspace size and the largest absolute difference between the two matrices.
          python tools/mmd_bench.py --perm [--z 32] [--n-perm 1000] [--loop-pairs 4]
--perm: the permutation test of row f18 (mmd.mmd2_permutation_test on two sets of 2000 rows, mmd.mmd2_permutation_matrix
on 20 conditions of 500 rows) against what the package offered before it: a host loop of n_perm + 1 ``_estimate_mmd2``
calls on index arrays permuted by the same memberships (read back from ``ava_mmd2_perm_membership`` outside the timed
region).  For the matrix the loop is timed over the first --loop-pairs pairs only and SCALED to all 190.  Each path is
warmed up at its shape, then five rounds alternate the two (the device path: median of --reps calls per round; the
loop: one pass per round), host clock with a device synchronisation before every stop.  One JSON line per shape: the
round medians and their spread, launches per path, the fp64 multiply-adds of K0 S per second, and whether the loop's
count of statistics >= stat_0 equals the device's."""
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
ap.add_argument("--perm", action="store_true")
ap.add_argument("--n-perm", type=int, default=1000)
ap.add_argument("--loop-pairs", type=int, default=4)
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


def perm_memberships(table, n_perm, seed):
    """uint8 [n_perm + 1, all positions] of every problem of the table, from the device"""
    from ava_amd import _lib
    lib = _lib.load()
    dev = mmd._device()
    tab = torch.from_numpy(table).to(dev)
    out = torch.empty((n_perm + 1) * int(table[-1, 5]), dtype=torch.uint8, device=dev)
    _lib.check(lib.ava_mmd2_perm_membership(table.ctypes.data, tab.data_ptr(), len(table) - 1, 0, n_perm + 1, seed,
                                            out.data_ptr(), _lib.stream()), "ava_mmd2_perm_membership")
    return out.cpu().numpy().reshape(n_perm + 1, -1)


def perm_bench(z, n_perm, reps, loop_pairs):
    sigma, seed = float(np.sqrt(z)), 0

    def host_loop(L, pool, n1, member):
        """the statistics of all splits the way the package could compute them before row f18"""
        return np.array([mmd._estimate_mmd2(L, pool[m == 1], pool[m == 0], sigma=sigma) for m in member])

    def rounds(device_fn, loop_fn):
        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        dev_out, loop_out = timed(device_fn)[1], timed(loop_fn)[1]        # warm-up of both paths at the timed shape
        r = {"device": [], "loop": []}
        for _ in range(5):
            r["device"].append(float(np.median([timed(device_fn)[0] for _ in range(reps)])))
            r["loop"].append(timed(loop_fn)[0])
        return r, dev_out, loop_out

    def report(res, r, scale):
        for k, v in r.items():
            f = scale if k == "loop" else 1.0
            res[k + "_median_s"] = round(float(np.median(v)) * f, 6)
            res[k + "_spread_s"] = round((max(v) - min(v)) * f, 6)
            res[k + "_rounds_s"] = [round(x * f, 6) for x in v]
        res["ratio_loop_over_device"] = round(res["loop_median_s"] / res["device_median_s"], 2)
        res["product_fp64_madds_per_s"] = res["product_fp64_madds"] / res["device_median_s"]
        print(json.dumps(res), flush=True)

    # one pair
    n = 2000
    latent = syn.gauss(2 * n * z, 31).reshape(2 * n, z)
    latent[n:] += 0.05
    L = mmd._latent_dev(latent)
    i1, i2 = np.arange(n), n + np.arange(n)
    pool = np.concatenate([i1, i2])
    table = mmd._perm_table(0, n, n, n, 0)
    member = perm_memberships(table, n_perm, seed)
    chunks = -(-(n_perm + 1) // mmd._perm_chunk(table, n_perm + 1, None))
    r, dev_out, loop_out = rounds(
        lambda: mmd.mmd2_permutation_test(L, i1, i2, n_perm=n_perm, seed=seed, sigma=sigma, return_null=True),
        lambda: host_loop(L, pool, n, member))
    res = {"perm": "pair", "n1": n, "n2": n, "z": z, "n_perm": n_perm, "reps_per_round": reps, "chunks": chunks,
           "device_launches": 4 * chunks, "loop_launches": 4 * (n_perm + 1), "chunk_bytes": mmd._perm_bytes(
               table, min(n_perm + 1, mmd._perm_chunk(table, n_perm + 1, None))),
           "product_fp64_madds": float((2 * n) ** 2) * (n_perm + 1 + chunks), "mmd2": dev_out[0], "pvalue": dev_out[1],
           "max_abs_diff_null": float(np.abs(dev_out[2] - loop_out[1:]).max()),
           "loop_count_equals_device": int((loop_out[1:] >= loop_out[0]).sum()) == round(dev_out[1] * (n_perm + 1)) - 1}
    report(res, r, 1.0)

    # the matrix: 20 conditions of 500 rows, rows interleaved
    C, n_per = 20, 500
    N = C * n_per
    condition = np.arange(N) % C
    latent = syn.gauss(N * z, 32).reshape(N, z) + 0.02 * condition[:, None]
    L = mmd._latent_dev(latent)
    plan = mmd._group_plan(condition)
    pa, pb = np.triu_indices(C, 1)
    table = mmd._perm_table(plan["offsets"][pa], plan["offsets"][pb], plan["counts"][pa], plan["counts"][pb],
                            np.arange(len(pa)))
    sub = np.ascontiguousarray(np.concatenate([table[:loop_pairs], table[-1:]]))
    sub[-1, 5], sub[-1, 6] = table[loop_pairs, 5], table[loop_pairs, 6]      # the sentinel of the shorter table
    member = perm_memberships(sub, n_perm, seed)
    lists = [plan["index"][plan["offsets"][c]:plan["offsets"][c + 1]] for c in range(C)]

    def loop_matrix():
        out = []
        for q in range(loop_pairs):
            pool = np.concatenate([lists[pa[q]], lists[pb[q]]])
            out.append(host_loop(L, pool, n_per, member[:, sub[q, 5]:sub[q + 1, 5]]))
        return np.array(out)
    chunks = -(-(n_perm + 1) // mmd._perm_chunk(table, n_perm + 1, None))
    r, dev_out, loop_out = rounds(
        lambda: mmd.mmd2_permutation_matrix(L, condition, n_perm=n_perm, seed=seed, sigma=sigma),
        loop_matrix)
    counts = (loop_out[:, 1:] >= loop_out[:, :1]).sum(axis=1)
    dev_counts = np.round(dev_out[1][pa[:loop_pairs], pb[:loop_pairs]] * (n_perm + 1)).astype(int) - 1
    res = {"perm": "matrix", "conditions": C, "n_per": n_per, "pairs": len(pa), "z": z, "n_perm": n_perm,
           "reps_per_round": reps, "chunks": chunks, "device_launches": 4 * chunks,
           "loop_launches": 4 * (n_perm + 1) * len(pa), "loop_timed_pairs": loop_pairs,
           "loop_scaled_by": len(pa) / loop_pairs,
           "chunk_bytes": mmd._perm_bytes(table, min(n_perm + 1, mmd._perm_chunk(table, n_perm + 1, None))),
           "product_fp64_madds": float(len(pa)) * (2 * n_per) ** 2 * (n_perm + 1 + chunks),
           "pvalue_min": float(dev_out[1].min()), "pvalue_median_offdiag": float(np.median(dev_out[1][pa, pb])),
           "max_abs_diff_mmd2": float(np.abs(dev_out[0][pa[:loop_pairs], pb[:loop_pairs]] - loop_out[:, 0]).max()),
           "loop_count_equals_device": bool((counts == dev_counts).all())}
    report(res, r, len(pa) / loop_pairs)


if a.perm:
    perm_bench(z, a.n_perm, a.reps, a.loop_pairs)
    sys.exit(0)
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
