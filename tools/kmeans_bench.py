"""k-means (ava_amd.kmeans, row f25) at repertoire scale: N latent rows of d columns from ava_amd.synthetic in K blobs,
resident in HBM.  Prints one JSON line per (N, K) (and appends it to ``--out``, by default
``profiles/f25_kmeans/kmeans_bench.jsonl``).  Every time is the median of ``--repeats`` windows after a warm-up window,
from HIP events around the window; ``*_spread`` is (max - min) / median over the windows, the run-to-run noise a
difference has to exceed.

* ``iteration_ms``: one Lloyd iteration of ``ava_km_fit`` (assign + chunk sums + reduce + finish, the control array
  zeroed before it), a window of 10.
* ``assign_ms``: ``ava_km_assign`` alone; ``assign_tflops`` counts 3 N K d operations (a difference and a fused
  multiply-add per feature) and ``assign_share_of_fp64_peak`` divides by the 78.6 TFLOP/s fp64 vector peak of the MI355X
  (half the 157.3 TFLOP/s fp32 vector rate).
* ``parent_round_ms`` (K <= 64, all it can do): one round of ``mixture._kmeans``, the only k-means of the parent commit,
  at the same rows and centres: ``ava_nn_argmin`` + ``ava_gm_onehot`` + ``ava_gm_means`` + the empty-cluster select,
  without its host read.  ``parent_over_new`` is the ratio to ``iteration_ms``; ``onehot_mb`` the N K 16 bytes the
  one-hot matrix moves per round.
* ``plusplus_centre_ms``: one ``ava_km_pp_step`` (scan, pick, update, commit, apply), a window of 10.
* ``fit_ms`` / ``fit_n_iter``: a whole ``KMeans(K, random_state=0).fit`` on the resident rows, seeding and host reads
  included (host clock around the call and a synchronisation).

    python tools/kmeans_bench.py [--shapes 100000x8 100000x64 100000x256 1000000x64] [--d 32]
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "f25_kmeans", "kmeans_bench.jsonl")
FP64_VECTOR_PEAK = 78.6e12
WINDOW = 10

from dbscan_bench import rows  # noqa: E402


def windows(fn, repeats, inner=1):
    """(median ms per call, (max - min) / median) over ``repeats`` event-timed windows of ``inner`` calls, after one
    warm-up window"""
    import torch
    for _ in range(inner):
        fn()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / inner)
    med = float(np.median(times))
    return round(med, 4), round((max(times) - min(times)) / med, 3)


def measure(n, d, k, repeats):
    import torch
    from ava_amd import _lib
    from ava_amd import kmeans as KM
    from ava_amd import mixture as MX
    lib = _lib.load()
    X, _ = rows(n, d, k)
    xd = torch.from_numpy(X).cuda()
    dev, code, st = xd.device, _lib.dtype_code(xd), _lib.stream()
    seeds = np.random.RandomState(0).choice(n, size=k, replace=False)
    start = xd[torch.from_numpy(seeds).cuda()].to(torch.float64).contiguous()
    out = {"mode": "device", "N": n, "d": d, "K": k, "repeats": repeats, "window": WINDOW}

    ws, nbytes = KM._workspace(n, d, k, dev)
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    ctl = torch.zeros(8, dtype=torch.int32, device=dev)
    mean_var = KM._variance_device(xd)
    centres = start.clone()

    def iteration():
        ctl.zero_()
        _lib.check(lib.ava_km_fit(xd.data_ptr(), code, n, d, k, centres.data_ptr(), labels.data_ptr(), d2.data_ptr(), 0.0,
                                  mean_var.data_ptr(), 0, 1, ctl.data_ptr(), None, ws.data_ptr(), nbytes, st),
                   "ava_km_fit")

    out["iteration_ms"], out["iteration_spread"] = windows(iteration, repeats, WINDOW)

    def assign():
        _lib.check(lib.ava_km_assign(xd.data_ptr(), code, n, d, k, start.data_ptr(), labels.data_ptr(), d2.data_ptr(),
                                     None, ws.data_ptr(), nbytes, st), "ava_km_assign")

    out["assign_ms"], out["assign_spread"] = windows(assign, repeats, WINDOW)
    out["assign_tflops"] = round(3.0 * n * k * d / (out["assign_ms"] * 1e-3) / 1e12, 3)
    out["assign_share_of_fp64_peak"] = round(out["assign_tflops"] * 1e12 / FP64_VECTOR_PEAK, 4)

    if k <= MX.MAX_K:
        nn_bytes = lib.ava_nn_workspace_bytes(n, k, d, 1)
        nn_ws = _lib.workspace(nn_bytes, dev, "nn")
        gws, gbytes = MX._workspace(n, d, k, 1, dev)
        lab64 = torch.empty(n, dtype=torch.int64, device=dev)
        dist = torch.empty(n, dtype=torch.float64, device=dev)
        prev = torch.full((n,), -1, dtype=torch.int64, device=dev)
        resp = torch.empty((n, k), dtype=torch.float64, device=dev)
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        weights = torch.empty(k, dtype=torch.float64, device=dev)
        means = torch.empty((k, d), dtype=torch.float64, device=dev)
        nk = torch.empty(k, dtype=torch.float64, device=dev)
        state = {"centres": start.clone()}

        def parent_round():
            c = state["centres"]
            _lib.check(lib.ava_nn_argmin(xd.data_ptr(), code, n, c.data_ptr(), 1, k, d, 1, lab64.data_ptr(),
                                         dist.data_ptr(), nn_ws.data_ptr(), nn_bytes, st), "ava_nn_argmin")
            changed.zero_()
            _lib.check(lib.ava_gm_onehot(lab64.data_ptr(), prev.data_ptr(), n, k, resp.data_ptr(), changed.data_ptr(),
                                         st), "ava_gm_onehot")
            _lib.check(lib.ava_gm_means(xd.data_ptr(), code, n, d, k, resp.data_ptr(), weights.data_ptr(),
                                        means.data_ptr(), nk.data_ptr(), gws.data_ptr(), gbytes, st), "ava_gm_means")
            state["centres"] = torch.where(nk[:, None] > 0.5, means, c).contiguous()

        out["parent_round_ms"], out["parent_round_spread"] = windows(parent_round, repeats, WINDOW)
        out["parent_over_new"] = round(out["parent_round_ms"] / out["iteration_ms"], 3)
        out["onehot_mb"] = round(n * k * 16 / 1e6, 1)

    trials = KM._n_trials(k)
    closest = torch.empty(n, dtype=torch.float64, device=dev)
    rand = torch.from_numpy(np.random.RandomState(1).uniform(size=trials)).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    pot = torch.zeros(1, dtype=torch.float64, device=dev)
    _lib.check(lib.ava_km_pp_start(xd.data_ptr(), code, n, d, int(seeds[0]), closest.data_ptr(), st), "ava_km_pp_start")

    def centre():
        _lib.check(lib.ava_km_pp_step(xd.data_ptr(), code, n, d, trials, rand.data_ptr(), closest.data_ptr(),
                                      idx.data_ptr(), pot.data_ptr(), ws.data_ptr(), nbytes, st), "ava_km_pp_step")

    out["plusplus_trials"] = trials
    out["plusplus_centre_ms"], out["plusplus_centre_spread"] = windows(centre, repeats, WINDOW)

    fits = []
    for _ in range(1 + min(repeats, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = KM.KMeans(k, random_state=0).fit(xd)
        torch.cuda.synchronize()
        fits.append((time.perf_counter() - t0) * 1e3)
    fits = fits[1:]
    out["fit_ms"] = round(float(np.median(fits)), 2)
    out["fit_spread"] = round((max(fits) - min(fits)) / float(np.median(fits)), 3)
    out["fit_n_iter"], out["fit_inertia"] = m.n_iter_, m.inertia_
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", nargs="+", default=["100000x8", "100000x64", "100000x256", "1000000x64"],
                    help="NxK pairs")
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench.py measures on the MI355X: no GPU found")
    for shape in a.shapes:
        n, k = (int(v) for v in shape.lower().split("x"))
        line = json.dumps(measure(n, a.d, k, a.repeats))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
