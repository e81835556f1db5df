"""Device nearest-neighbour search (ava_amd.neighbors) at shotgun-movie scale: a 60 s movie
at 30 fps (1800 query windows) against 20000 syllables.  Prints one JSON line: the device time of ava_nn_argmin (HIP
events, median of --reps after a warm-up) for the correlation search over 128 x 128 fp32 spectrograms (d = 16384) and
the euclidean search over z = 32 latent means, and the achieved fp64 GFLOP/s (2 nq nr d for the centred dot
products, 3 nq nr d for the differences).  With --cpu also the reference's CPU paths at a reduced size -- sklearn's
NearestNeighbors(metric='correlation') and the latent_nn loop of scipy euclidean calls -- extrapolated linearly to the
full size and labelled as such.

    python tools/nn_bench.py [--nq 1800] [--nr 20000] [--d 16384] [--z 32] [--reps 5] [--cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _device_ms(lib, q, r, metric, reps):
    import torch
    from ava_amd import _lib
    nq, d = q.shape
    nr = r.shape[0]
    nbytes = lib.ava_nn_workspace_bytes(nq, nr, d, metric)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    idx = torch.empty(nq, dtype=torch.int64, device=q.device)
    dist = torch.empty(nq, dtype=torch.float64, device=q.device)
    code = 0 if q.dtype == torch.float32 else 1

    def run():
        _lib.check(lib.ava_nn_argmin(q.data_ptr(), code, nq, r.data_ptr(), code, nr, d, metric, idx.data_ptr(),
                                     dist.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "ava_nn_argmin")

    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def _cpu_baselines(d, z, nq, nr):
    from scipy.spatial.distance import euclidean
    from sklearn.neighbors import NearestNeighbors
    from ava_amd import synthetic as syn
    sq, sr = 60, 2000
    specs = syn.spectrograms(sq + sr, salt=71, shape=(1, d)).reshape(sq + sr, d)
    t0 = time.perf_counter()
    nbrs = NearestNeighbors(n_neighbors=1, metric='correlation').fit(specs[sq:])
    nbrs.kneighbors(specs[:sq], return_distance=False)
    sk = time.perf_counter() - t0
    lq, lr = 3, nr
    lat = syn.gauss((lq + lr) * z, 72).reshape(lq + lr, z)
    t0 = time.perf_counter()
    for i in range(lq):
        np.argmin([euclidean(lat[i], j) for j in lat[lq:]])
    loop = time.perf_counter() - t0
    return {"cpu_sklearn_correlation_measured": {"nq": sq, "nr": sr, "d": d, "s": round(sk, 3)},
            "cpu_sklearn_correlation_s_extrapolated": round(sk * (nq * nr) / (sq * sr), 1),
            "cpu_latent_nn_loop_measured": {"nq": lq, "nr": lr, "z": z, "s": round(loop, 3)},
            "cpu_latent_nn_loop_s_extrapolated": round(loop * nq / lq, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=1800)
    ap.add_argument("--nr", type=int, default=20000)
    ap.add_argument("--d", type=int, default=16384)
    ap.add_argument("--z", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from ava_amd import _lib
    lib = _lib.load()
    nq, nr, d, z = args.nq, args.nr, args.d, args.z
    g = torch.Generator(device="cuda").manual_seed(0)
    # clipped log-spectrogram-like fp32 rows (as ava_amd.synthetic.spectrograms), generated on the device
    refs = (1.4 * torch.rand(nr, d, generator=g, device="cuda") - 0.4).clamp_(0.0, 1.0)
    queries = (1.4 * torch.rand(nq, d, generator=g, device="cuda") - 0.4).clamp_(0.0, 1.0)
    corr = _device_ms(lib, queries, refs, 0, args.reps)
    del refs, queries
    lat_r = torch.randn(nr, z, generator=g, device="cuda", dtype=torch.float64)
    lat_q = torch.randn(nq, z, generator=g, device="cuda", dtype=torch.float64)
    eucl = _device_ms(lib, lat_q, lat_r, 1, args.reps)
    c_med, e_med = float(np.median(corr)), float(np.median(eucl))
    out = {"workload": "1-NN, %d queries x %d references" % (nq, nr),
           "correlation_d": d, "correlation_dtype": "float32", "correlation_ms_median": round(c_med, 3),
           "correlation_ms_all": [round(x, 3) for x in corr],
           "correlation_fp64_gflops": round(2.0 * nq * nr * d / (c_med * 1e-3) / 1e9, 1),
           "euclidean_z": z, "euclidean_dtype": "float64", "euclidean_ms_median": round(e_med, 3),
           "euclidean_ms_all": [round(x, 3) for x in eucl],
           "euclidean_fp64_gflops": round(3.0 * nq * nr * z / (e_med * 1e-3) / 1e9, 1)}
    if args.cpu:
        out.update(_cpu_baselines(d, z, nq, nr))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
