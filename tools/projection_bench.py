"""UMAP and PCA projections of latent means (ava_amd.projection) at DataContainer scale: N latent means of z = 32.
Prints one JSON line per N with the stages of ``UMAP().fit_transform`` -- device kNN, device bandwidths + host fuzzy
union, host init, device layout (HIP events, median of --reps after a warm-up; host stages wall clock) and the
wall-clock total of one call -- the achieved fp64 GFLOP/s of the kNN pass (3 N^2 z for the differences), and for PCA
the device moments and projection times beside sklearn's CPU ``PCA(n_components=2).fit_transform`` (when sklearn is
installed).  There is no umap-learn CPU time to compare with.

    python tools/projection_bench.py [--sizes 20000 200000] [--z 32] [--reps 3] [--quality-n 20000]
"""
import argparse
import json
import os
import sys
import time

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


def bench(n, z, reps, quality_n=20000):
    import torch
    from ava_amd import _lib, projection as P, synthetic as syn
    X = syn.gauss(n * z, 7100 + n).reshape(n, z).astype(np.float32)
    xd = torch.from_numpy(X).cuda()
    model = P.UMAP()
    k = model.n_neighbors
    out = {"N": n, "z": z, "k": k}

    out["knn_ms"] = round(_events_ms(lambda: P._knn_device(xd, k), reps), 3)
    out["knn_fp64_gflops"] = round(3.0 * n * n * z / (out["knn_ms"] * 1e6), 1)
    idx, dist = P._knn_device(xd, k)
    out["bandwidths_ms"] = round(_events_ms(lambda: P._smooth_device(idx, dist, 1.0), reps), 3)
    sigma, rho, w = P._smooth_device(idx, dist, 1.0)
    t0 = time.perf_counter()
    G = P.fuzzy_union(idx.cpu().numpy(), w.cpu().numpy(), n)
    out["union_host_s"] = round(time.perf_counter() - t0, 3)
    n_epochs = 500 if n <= 10000 else 200
    Gp = G.copy()
    Gp.data[Gp.data < Gp.data.max() / float(n_epochs)] = 0.0
    Gp.eliminate_zeros()
    rs = np.random.RandomState(42)
    t0 = time.perf_counter()
    Y0 = P.init_embedding(Gp, 'spectral', rs)
    out["init_host_s"] = round(time.perf_counter() - t0, 3)
    P.init_embedding(Gp, 'spectral', np.random.RandomState(42), eigen_solver='device')        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    P.init_embedding(Gp, 'spectral', np.random.RandomState(42), eigen_solver='device')
    out["init_device_s"] = round(time.perf_counter() - t0, 4)
    salt = rs.randint(2 ** 31 - 1)
    a, b = P.find_ab_params(1.0, 0.1)
    out["graph_nnz"] = int(Gp.nnz)
    out["layout_epochs"] = n_epochs
    out["layout_ms"] = round(_events_ms(lambda: P.Layout(Gp, Y0, n_epochs, a, b, salt=salt).run(), reps), 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Y = P.UMAP().fit_transform(X)
    out["umap_total_s"] = round(time.perf_counter() - t0, 3)
    assert Y.shape == (n, 2) and np.all(np.isfinite(Y))
    t0 = time.perf_counter()
    Yd = P.UMAP(eigen_solver='device').fit_transform(X)
    out["umap_total_device_s"] = round(time.perf_counter() - t0, 3)
    assert Yd.shape == (n, 2) and np.all(np.isfinite(Yd))
    if n <= quality_n:
        from ava_amd import embedding_quality as EQ
        ks = [5, 15, 30]
        for name, pic in (("quality_scipy_init", Y), ("quality_device_init", Yd)):
            out[name] = {key: [round(float(v), 4) for v in val] for key, val in EQ.quality_curve(X, pic, ks).items()}
        out["quality_ks"] = ks

    lib = _lib.load()
    nbytes = lib.ava_pj_gram_workspace_bytes(n, z)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xd.device)
    gram = torch.empty((z + 1, z + 1), dtype=torch.float64, device=xd.device)
    out["pca_moments_ms"] = round(_events_ms(lambda: _lib.check(lib.ava_pj_gram(
        xd.data_ptr(), 0, n, z, gram.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "ava_pj_gram"), reps), 3)
    V = torch.zeros((2, z), dtype=torch.float64, device=xd.device)
    muv = torch.zeros(2, dtype=torch.float64, device=xd.device)
    proj = torch.empty((n, 2), dtype=torch.float64, device=xd.device)
    out["pca_project_ms"] = round(_events_ms(lambda: _lib.check(lib.ava_pj_project(
        xd.data_ptr(), 0, n, z, V.data_ptr(), muv.data_ptr(), 2, proj.data_ptr(), _lib.stream()), "ava_pj_project"),
        reps), 3)
    t0 = time.perf_counter()
    P.pca_projection(X)
    out["pca_total_s"] = round(time.perf_counter() - t0, 4)
    try:
        from sklearn.decomposition import PCA
    except ImportError:
        out["cpu_sklearn_pca_s"] = None
    else:
        X64 = X.astype(np.float64)
        t0 = time.perf_counter()
        PCA(n_components=2, copy=False, random_state=42).fit_transform(X64)
        out["cpu_sklearn_pca_s"] = round(time.perf_counter() - t0, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 200000])
    ap.add_argument("--z", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quality-n", type=int, default=20000)
    args = ap.parse_args()
    for n in args.sizes:
        print(json.dumps(bench(n, args.z, args.reps, args.quality_n)), flush=True)


if __name__ == "__main__":
    main()
