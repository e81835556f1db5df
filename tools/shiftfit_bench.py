"""The integer-shift fit (ava_amd.shift_fit) at the sizes of segment_sylls_from_songs:
``ShiftWarping(maxlag=0.2, smoothness_reg_scale=10.0).fit(iterations=50)`` on synthetic renditions (three Gaussian
bumps with per-row gains, moved by known integer shifts, in a little noise; float32), at two shapes: K = 10000 amplitude
traces of T = 155 bins (the reference's use) and K = 2000 whole spectrograms of F = 128, T = 155.  Prints one JSON line.

Per shape: the wall time of ``fit`` after a warm-up call, with a device synchronisation before the clock stops; the loss
kernel's time per launch (HIP events, median of --reps launches) and the terms per second it sums; and, as the baseline,
``ava_warpfit_loss`` fed the same integer shifts as (shift, log slope = 0) candidates with ``slope_λ = inf`` at the same
shape.  The two kernels are timed alternately, --rounds times each, so that the spread of the baseline's medians is on
record beside the difference: ``faster_beyond_spread`` says whether the slowest median of the new kernel is below the
fastest of the baseline.  The two losses are compared as well (``max_rel_diff``: the same terms in another order, and the
baseline not divided by F T)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(10000, 1, 155), (2000, 128, 155)]
MAXLAG, SMOOTHNESS, ITERATIONS = 0.2, 10.0, 50


def workload(K, F, T, salt=5600):
    from ava_amd import synthetic as syn
    L = int(MAXLAG * T)
    centres, widths = np.array([0.2, 0.45, 0.75]) * T, np.array([0.05, 0.07, 0.04]) * T
    gains = (0.5 + syn.u01(3 * F, salt + 1).reshape(F, 3)).astype(np.float32)
    sh = np.round((2 * syn.u01(K, salt) - 1) * 0.5 * L)
    t = (np.arange(T)[None, :] - sh[:, None]).astype(np.float32)               # [K, T]
    x = np.zeros((K, F, T), dtype=np.float32)
    for b in range(3):
        x += gains[None, :, b, None] * np.exp(-0.5 * ((t - centres[b]) / widths[b]) ** 2)[:, None, :]
    x += (0.02 * syn.u01(K * F * T, salt + 2)).astype(np.float32).reshape(K, F, T)
    if F == 1:
        x -= x.mean(axis=2, keepdims=True)
        x /= x.std(axis=2, keepdims=True) + 1e-12
    return x, sh.astype(np.int64)


def one_shape(K, F, T, reps, rounds):
    import torch
    from ava_amd import _lib
    from ava_amd import shift_fit as sf
    x, planted = workload(K, F, T)
    d = torch.from_numpy(x).cuda()
    data = d.transpose(1, 2)                                                   # affinewarp's [K, T, N], a view
    L = int(MAXLAG * T)
    C = 2 * L + 1

    def fit():
        return sf.ShiftWarping(maxlag=MAXLAG, smoothness_reg_scale=SMOOTHNESS).fit(data, iterations=ITERATIONS)

    fit()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = fit()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    offsets = model.shifts - planted

    lib, st = _lib.load(), _lib.stream()
    m = model.template.t().contiguous()
    loss = torch.empty((K, C), dtype=torch.float64, device="cuda")
    base = torch.empty((K, C), dtype=torch.float64, device="cuda")
    cand = torch.zeros((K, C, 2), dtype=torch.float64, device="cuda")
    cand[:, :, 0] = torch.from_numpy(sf.lag_order(L)).cuda().double()

    def run_new():
        _lib.check(lib.ava_shiftfit_loss(d.data_ptr(), 0, K, F, T, m.data_ptr(), L, loss.data_ptr(), st), "ava_shiftfit_loss")

    def run_base():
        _lib.check(lib.ava_warpfit_loss(d.data_ptr(), 0, K, F, T, m.data_ptr(), cand.data_ptr(), C, 0.0, float('inf'),
                                        base.data_ptr(), st), "ava_warpfit_loss")

    def median_ms(launch):
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    run_new()
    run_base()
    torch.cuda.synchronize()
    rel = float((loss * (F * T) / base - 1).abs().max())
    new_ms, base_ms = [], []
    for _ in range(rounds):
        base_ms.append(median_ms(run_base))
        new_ms.append(median_ms(run_new))
    terms = K * C * F * T
    return {"K": K, "F": F, "T": T, "L": L, "lags": C, "fit_wall_s": wall, "loss_hist_first": model.loss_hist[0],
            "loss_hist_last": model.loss_hist[-1], "shifts_equal_planted_up_to_one_offset": bool(len(set(offsets.tolist())) == 1),
            "loss_kernel": "shiftfit_loss_kernel", "loss_kernel_ms": float(np.median(new_ms)), "loss_kernel_ms_rounds": new_ms,
            "loss_kernel_terms_per_s": terms / (float(np.median(new_ms)) * 1e-3),
            "baseline_kernel": "warpfit_loss_kernel<float, WfAffine>", "baseline_ms": float(np.median(base_ms)), "baseline_ms_rounds": base_ms,
            "baseline_spread_ms": max(base_ms) - min(base_ms), "speedup": float(np.median(base_ms) / np.median(new_ms)),
            "faster_beyond_spread": bool(max(new_ms) < min(base_ms)), "max_rel_diff": rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9, help="launches per median")
    ap.add_argument("--rounds", type=int, default=5, help="medians per kernel, the two kernels alternating")
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("K", "F", "T"),
                    help="a shape instead of the two default ones (may be repeated)")
    a = ap.parse_args()
    shapes = [tuple(s) for s in a.shape] if a.shape else SHAPES
    out = {"bench": "shiftfit", "maxlag": MAXLAG, "smoothness_reg_scale": SMOOTHNESS, "iterations": ITERATIONS,
           "dtype": "float32", "reps": a.reps, "rounds": a.rounds,
           "shapes": [one_shape(K, F, T, a.reps, a.rounds) for K, F, T in shapes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
