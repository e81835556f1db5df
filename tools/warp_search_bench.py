"""The warp parameter search (ava_amd.warp_search) at its default size: 30 sampled settings
(knot counts -1, 0, 1, ten each) x 5 bin splits = 150 fits of N = 256 synthetic motifs of 128 x 128 float32 on their
train bins (78 of 128), under the default 8-iteration schedule.  Prints one JSON line.

Two ways to the same 150 fits, timed after a warm-up of each, with a device synchronisation before the clock stops:

    grouped   ``warp_fit.align_specs_grouped``, one call per knot count: all 50 fits of a knot count advance together
              over the spectrograms where they lie
    loop      the fit as it was before row f17: for every fit the train bins are gathered into a tensor of their own
              and ``warp_fit.align_specs`` runs on it

and checks that both return the same bits.  The launch counts are counted at the C ABI (every ``ava_warpfit_*`` call is
one kernel launch); the torch elementwise launches around them (a handful per iteration) are not.  ``--scores`` adds the
wall time of the whole ``cross_validate`` (fits, templates and sums of squares of the three bin sets).
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.warpfit_bench import workload  # noqa: E402


class CountingLib:
    """the loaded library with its ``ava_warpfit_*`` calls counted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ava_warpfit_") or name.startswith("ava_warpfit_max"):
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--t", type=int, default=128)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--samples-per-knot", type=int, default=10)
    ap.add_argument("--scores", action="store_true", help="also time the whole cross_validate")
    a = ap.parse_args()
    import torch
    from ava_amd import _lib
    from ava_amd import warp_fit as wf
    from ava_amd import warp_search as ws

    specs = workload(a.n, a.f, a.t)
    d = torch.from_numpy(specs).cuda()
    params = {'samples_per_knot': a.samples_per_knot}
    knots, _, _, schedules, splits = ws.search_plan(a.f, params, a.seed)
    n_splits = len(splits[0])
    jobs = {}                                                # knot count -> [(train bins, shift_λs, slope_λs)]
    for s, k in enumerate(knots.tolist()):
        jobs.setdefault(k, []).extend((splits[s][v][0], schedules[s][0], schedules[s][1]) for v in range(n_splits))

    def grouped():
        out = []
        for k, fits in sorted(jobs.items()):
            out += wf.align_specs_grouped(d, [(None, b) for b, _, _ in fits], np.array([s for _, s, _ in fits]).T,
                                          np.array([s for _, _, s in fits]).T, n_knots=max(k, 0))
        return out

    def loop():
        out = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for k, fits in sorted(jobs.items()):
                for b, shift, slope in fits:
                    sub = d[:, torch.from_numpy(b).cuda(), :].contiguous()
                    out.append(wf.align_specs(sub, shift, slope, verbose=False, n_knots=max(k, 0))[1])
        return out

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        real, counting = _lib.load, CountingLib(_lib.load())
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        _lib.load = lambda: counting                        # a third run, only to count the launches
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            _lib.load = real
        return res, wall, counting.calls

    g_res, g_wall, g_calls = timed(grouped)
    l_res, l_wall, l_calls = timed(loop)
    same = all(torch.equal(x[key].view(torch.int64), y[key].view(torch.int64)) for x, y in zip(g_res, l_res) for key in y)
    out = {"bench": "warp_search", "N": a.n, "F": a.f, "T": a.t, "dtype": str(specs.dtype), "seed": a.seed,
           "fits": len(g_res), "fits_per_knot_count": {str(k): len(v) for k, v in sorted(jobs.items())},
           "train_bins": int(len(splits[0][0][0])), "iterations": len(schedules[0][0]),
           "grouped_wall_s": g_wall, "loop_wall_s": l_wall, "loop_over_grouped": l_wall / g_wall,
           "grouped_kernel_launches": g_calls, "loop_kernel_launches": l_calls, "same_bits": bool(same)}
    if a.scores:
        ws.cross_validate(d, params, a.seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ws.cross_validate(d, params, a.seed)
        torch.cuda.synchronize()
        out["cross_validate_wall_s"] = time.perf_counter() - t0
        med = np.median(res['valid_rsq'], axis=1)
        out["median_valid_rsq_by_knot_count"] = {str(k): float(med[knots == k].max()) for k in sorted(set(knots.tolist()))}
        best = ws.best_warp_params(res)
        out["best_warp_params"] = {k: v if k == 'n_knots' else [x if np.isfinite(x) else "inf" for x in v] for k, v in best.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
