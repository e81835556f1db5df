"""The time-warp fit (ava_amd.warp_fit) at motif-dataset scale: ``align_specs`` on 512
synthetic motifs of 128 x 128 float32 (sums of wide Gaussian bumps with per-row gains, warped by known shifts and
slopes), 10 iterations: three shift-only, then seven with decreasing penalties.  Prints one JSON line.

    python tools/warpfit_bench.py                      the device: wall time of align_specs after a warm-up call, with
                                                       a device synchronisation before the clock stops; the loss
                                                       kernel's time per launch (HIP events, median of --reps) for the
                                                       35-candidate grid, and its bytes per second: every workgroup
                                                       reads its motif (F T 4 bytes) and the target (F T 8 bytes) once
                                                       per block of 8 candidates
    python tools/warpfit_bench.py --n-knots 4          the same with the piecewise-linear warp of row f14 (6 knots per
                                                       motif): every iteration that is not shift-only adds the
                                                       coordinate search, (knot rounds x 6) x 3 small launches; the
                                                       loss_kernel_* fields still time the shift-and-slope kernel
                                                       (stage A of every iteration), pl_loss_kernel_* the knot
                                                       search's kernel on its 7 candidates of 6 knots
    python tools/warpfit_bench.py --reference PATH     the reference's ava.preprocessing.warping.align_specs (numpy and
                                                       scipy's Powell) on the same workload, on this machine's CPU

The two numbers come from different machines when the reference is timed on a box without the device.
"""
import argparse
import io
import json
import os
import sys
import time
import warnings
from contextlib import redirect_stdout

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHIFT_LAMBDAS = [1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 1e-3, 0.0, 0.0]
SLOPE_LAMBDAS = [np.inf, np.inf, np.inf, 100.0, 10.0, 1.0, 0.1, 0.01, 0.0, 0.0]


def workload(N, F, T, salt=5150):
    from ava_amd import synthetic as syn
    u = syn.u01(2 * N, salt)
    shifts, slopes = (2 * u[:N] - 1) * 4.0, 0.93 + 0.17 * u[N:]
    centres, widths = [0.25, 0.5, 0.8], [0.06, 0.09, 0.05]
    gains = 0.5 + syn.u01(F * 3, salt + 1).reshape(F, 3)
    pos = (np.arange(T)[None, :] - shifts[:, None]) / slopes[:, None]
    out = np.zeros((N, F, T))
    for k in range(3):
        out += gains[None, :, k, None] * np.exp(-0.5 * ((pos - centres[k] * T) / (widths[k] * T)) ** 2)[:, None, :]
    out += 0.01 * syn.u01(N * F * T, salt + 2).reshape(N, F, T)
    return out.astype(np.float32)


def spread(w):
    w = np.asarray(w, dtype=np.float64)
    return float(((w - w.mean(axis=0)) ** 2).sum())


def device(specs, reps, n_knots=0):
    import torch
    from ava_amd import _lib
    from ava_amd import warp_fit as wf
    N, F, T = specs.shape
    d = torch.from_numpy(specs).cuda()

    def fit():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return wf.align_specs(d, SHIFT_LAMBDAS, SLOPE_LAMBDAS, verbose=False, n_knots=n_knots)

    fit()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    warped, _ = fit()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    # the loss kernel alone, on the grid of a two-parameter round
    lib = _lib.load()
    ks, kl, rounds = wf.search_rounds(T, False)
    C = (2 * ks + 1) * (2 * kl + 1)
    x = torch.zeros((N, 2), dtype=torch.float64, device="cuda")
    cand = torch.empty((N, C, 2), dtype=torch.float64, device="cuda")
    loss = torch.empty((N, C), dtype=torch.float64, device="cuda")
    target = d.double().mean(dim=0).contiguous()
    _lib.check(lib.ava_warpfit_candidates(x.data_ptr(), N, T, ks, kl, rounds[3][0], rounds[3][1], cand.data_ptr(), _lib.stream()),
               "ava_warpfit_candidates")

    def run():
        _lib.check(lib.ava_warpfit_loss(d.data_ptr(), 0, N, F, T, target.data_ptr(), cand.data_ptr(), C, 1e-3, 1.0,
                                        loss.data_ptr(), _lib.stream()), "ava_warpfit_loss")

    def median_ms(launch):
        launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    med = median_ms(run)
    blocks = N * ((C + 7) // 8)
    nbytes = blocks * F * T * (specs.dtype.itemsize + 8)
    launches = sum(len(wf.search_rounds(T, lam == np.inf)[2]) for lam in SLOPE_LAMBDAS)
    knot_launches = 3 * (n_knots + 2) * len(wf.knot_rounds(T, n_knots + 2)) * sum(lam != np.inf for lam in SLOPE_LAMBDAS) \
        if n_knots else 0
    out = {"n_knots": n_knots, "knot_search_launches_per_fit": knot_launches, "loss_kernel": "warpfit_loss_kernel<float, WfAffine>"}
    if n_knots:
        # the knot search's loss kernel alone: one knot of every motif moved, 2 KNOT_KS + 1 candidates of K knots
        K, Cp = n_knots + 2, 2 * wf.KNOT_KS + 1
        u = torch.from_numpy(np.tile(wf.knot_columns(T, K), (N, 1))).cuda()
        pcand = torch.empty((N, Cp, K), dtype=torch.float64, device="cuda")
        ploss = torch.empty((N, Cp), dtype=torch.float64, device="cuda")
        _lib.check(lib.ava_warpfit_pl_candidates(u.data_ptr(), N, K, 1, wf.KNOT_KS, wf.knot_rounds(T, K)[3], pcand.data_ptr(),
                                                 _lib.stream()), "ava_warpfit_pl_candidates")

        def run_pl():
            _lib.check(lib.ava_warpfit_pl_loss(d.data_ptr(), 0, N, F, T, target.data_ptr(), pcand.data_ptr(), Cp, K, 1e-3, 1.0,
                                               ploss.data_ptr(), _lib.stream()), "ava_warpfit_pl_loss")

        pmed = median_ms(run_pl)
        pbytes = N * ((Cp + 7) // 8) * F * T * (specs.dtype.itemsize + 8)
        out.update({"pl_loss_kernel": "warpfit_loss_kernel<float, WfKnots>", "pl_loss_kernel_ms": pmed, "pl_loss_kernel_candidates": Cp,
                    "pl_loss_kernel_bytes": pbytes, "pl_loss_kernel_TB_per_s": pbytes / (pmed * 1e-3) / 1e12,
                    "pl_loss_kernel_interp_per_s": N * Cp * F * T / (pmed * 1e-3), "pl_loss_launches_per_fit": knot_launches // 3})
    out.update({"align_specs_wall_s": wall, "spread_before": spread(specs), "spread_after": spread(warped.cpu().numpy()),
            "loss_kernel_ms": med, "loss_kernel_candidates": C, "loss_kernel_bytes": nbytes,
            "loss_kernel_TB_per_s": nbytes / (med * 1e-3) / 1e12, "loss_kernel_fraction_of_8TBps": nbytes / (med * 1e-3) / 8e12,
            "loss_launches_per_fit": launches,
            "loss_kernel_interp_per_s": N * C * F * T / (med * 1e-3)})
    return out


def reference(specs, path):
    sys.path.append(path)
    import ava.preprocessing.warping as W
    t0 = time.perf_counter()
    with warnings.catch_warnings(), redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        warped, _ = W.align_specs(specs, SHIFT_LAMBDAS, SLOPE_LAMBDAS, verbose=False)
    wall = time.perf_counter() - t0
    assert warped is not None
    return {"reference_align_specs_wall_s": wall, "spread_before": spread(specs), "spread_after": spread(warped)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--t", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n-knots", type=int, default=0, help="inner knots of the piecewise-linear warp (0: shift and slope)")
    ap.add_argument("--reference", default=None, help="path of the reference package: time its align_specs on the CPU")
    a = ap.parse_args()
    specs = workload(a.n, a.f, a.t)
    out = {"bench": "warpfit", "N": a.n, "F": a.f, "T": a.t, "iterations": len(SHIFT_LAMBDAS), "dtype": str(specs.dtype)}
    out.update(reference(specs, a.reference) if a.reference else device(specs, a.reps, a.n_knots))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
