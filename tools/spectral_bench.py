"""The sparse eigensolver of ava_amd.spectral on the graph UMAP's spectral init solves: the pruned fuzzy
graph of N synthetic latent means (z = 32, k = 20), three eigenpairs at tol 1e-4.  Prints one JSON line per N: the device
components pass and, for every ncv of the sweep, the whole solve (HIP events, median of --reps after a warm-up) with its
operator applications and restarts; one operator call (with its graph check and the wait for it) and one restart cycle of
64 Lanczos steps with the bytes they move
(operator: 20 bytes per stored entry and 8 per gathered ``x[col] dinv[col]`` pair, 16 n for dinv and y; Gram-Schmidt: the
basis is read four times a step, twice by ``B^T w`` and twice by ``w -= B h``, 32 n m bytes at m vectors); and in the same
session scipy's ``connected_components`` plus ARPACK ``eigsh`` exactly as ``projection._spectral`` calls them.

    python tools/spectral_bench.py [--sizes 20000 200000] [--z 32] [--reps 3] [--no-scipy]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def pruned_graph(n, z, k=20):
    """the graph ``UMAP.fit`` hands to ``init_embedding`` for n gaussian latent means"""
    import torch
    from ava_amd import projection as P, synthetic as syn
    X = syn.gauss(n * z, 7100 + n).reshape(n, z).astype(np.float32)
    idx, dist = P._knn_device(torch.from_numpy(X).cuda(), k)
    _, _, w = P._smooth_device(idx, dist, 1.0)
    G = P.fuzzy_union(idx.cpu().numpy(), w.cpu().numpy(), n)
    n_epochs = 500 if n <= 10000 else 200
    G.data[G.data < G.data.max() / float(n_epochs)] = 0.0
    G.eliminate_zeros()
    return G


def bench(n, z, reps, scipy_too):
    import torch
    from ava_amd import projection as P, spectral as SP
    G = pruned_graph(n, z)
    A = SP._check_graph(G)
    out = {"N": n, "z": z, "graph_nnz": int(A.nnz), "max_row_nnz": int(np.diff(A.indptr).max()), "tol": 1e-4}

    def components():
        g = SP._Graph(A)
        g.components()
        return g

    t0 = time.perf_counter()
    g = components()
    torch.cuda.synchronize()
    out["upload_degrees_components_first_s"] = round(time.perf_counter() - t0, 4)

    def components_only():
        g._components = None
        g.components()

    out["components_ms"] = round(_events_ms(components_only, reps), 3)
    out["n_components"] = g.components()[0]
    if out["n_components"] == 1:
        sweep = {}
        for ncv in sorted({32, 64, 128, int(np.sqrt(n))}):
            stats = {}

            def solve():
                try:
                    sol = SP._solve(g, 3, 1e-4, ncv=ncv)
                    stats.update(n_ops=sol.n_ops, n_restarts=sol.n_restarts, lam=[float(v) for v in 1.0 - sol.mu],
                                 residual=float(sol.residuals.max()))
                except SP.SpectralConvergenceError as e:
                    stats.update(error=str(e)[:80])
            stats["solve_ms"] = round(_events_ms(solve, reps), 3)
            sweep[str(ncv)] = stats
        out["ncv_sweep"] = sweep
        x = torch.from_numpy(np.random.RandomState(0).normal(size=n)).cuda()
        op_ms = _events_ms(lambda: g.apply(x), reps * 5)
        out["operator_ms"] = round(op_ms, 4)
        out["operator_gbs"] = round((A.nnz * 28.0 + 32.0 * n) / (op_ms * 1e6), 1)
        steps = 64
        b = SP._Basis(g, 1 + steps + 1, 1)
        b.null_vectors(g.components()[1], 1)
        b.start(0)
        cyc_ms = _events_ms(lambda: b.lanczos(0, steps), reps)
        gs_bytes = sum(32.0 * n * (1 + j + 1) for j in range(steps))
        out["cycle64_ms"] = round(cyc_ms, 3)
        out["cycle64_basis_gbs"] = round(gs_bytes / (cyc_ms * 1e6), 1)          # over the whole step, operator included
        rest_ms = cyc_ms - steps * op_ms                 # op_ms is a call with its graph check: too large for small N
        out["gram_schmidt_gbs"] = round(gs_bytes / (rest_ms * 1e6), 1) if rest_ms > 0.0 else None
    if scipy_too:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            Y = P._spectral(G)
            out["scipy_components_eigsh_s"] = round(time.perf_counter() - t0, 3)
            out["scipy_converged"] = Y is not None
            t0 = time.perf_counter()
            P._spectral_device(G)
            out["device_init_s"] = round(time.perf_counter() - t0, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 200000])
    ap.add_argument("--z", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    for n in args.sizes:
        print(json.dumps(bench(n, args.z, args.reps, not args.no_scipy)), flush=True)


if __name__ == "__main__":
    main()
