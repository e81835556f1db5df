"""Warped shotgun windows (ava_amd.warped_window): a batch out of the motif cache against
the same batch through get_spec_batch(0, template_dur), which transforms the whole motif for every window (what the
reference does per window, and all the library offered before the cache).

On synthetic motifs of 0.5 s and 1.0 s with the finch parameter set, at batch 64 and 256:
  (a) the cache build, once (device events around ava_warp_cache_build, after a warm-up build);
  (b) a batch through DeviceWarpedWindowDataset.windows;
  (c) the same windows through spec.get_spec_batch(audio, file_idx, 0.0, template_dur, ..., target_times).
(b) and (c) include their per-batch parameter upload.  Every shape is warmed up; a timing is device events around
--iters calls; (b) and (c) alternate within each of --reps rounds, and the spread reported is the min .. max over the
rounds.  The outputs of (b) and (c) are compared bit for bit before anything is timed.  Prints one JSON line.

The measurement runs in ONE child process under a time limit (--timeout seconds); no retries.

    python tools/warped_bench.py [--files 32] [--iters 50] [--reps 7] [--timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _stats(ms):
    import numpy as np
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def child(args):
    import numpy as np
    import torch
    from ava_amd import spec as sp
    from ava_amd import synthetic as syn
    from ava_amd import warped_window as ww

    assert torch.cuda.is_available(), "warped_bench needs the GPU"
    p = dict(syn.FINCH_PARAMS)
    fs = p['fs']
    out = {"workload": "warped windows, finch parameters, %d motif files" % args.files, "iters": args.iters,
           "reps": args.reps, "cases": []}
    for seconds in (0.5, 1.0):
        ex, _, _ = syn.songs(n_exemplars=args.files, n_songs=0, fs=fs, seconds=1.0, motif_seconds=seconds, salt=8800)
        xk = np.tile(np.array([0.0, 0.3, 0.7, 1.0]), (args.files, 1))
        yk = np.tile(np.array([0.0, 0.35, 0.65, 1.0]), (args.files, 1))
        ds = ww.DeviceWarpedWindowDataset.from_arrays(ex, fs, p, x_knots=xk, y_knots=yk)
        ds.build_cache()                                            # warm-up build
        torch.cuda.synchronize()
        build = [_timed(ds.build_cache, 1) for _ in range(args.reps)]
        nstep = p['nperseg'] - p['noverlap']
        entry = {"motif_seconds": seconds, "template_dur": round(float(ds.template_dur), 6),
                 "frames_per_motif": int(round(ds.template_dur * fs)) // nstep + 1, "cache_bytes": ds.cache_bytes,
                 "cache_build": _stats(build), "batches": []}
        for n in (64, 256):
            file_idx, tt = ds._draw(n, seed=n)
            t1, t2 = np.zeros(n), np.full(n, ds.template_dur)

            def cached():
                return ds.windows(file_idx, tt)

            def whole():
                return sp.get_spec_batch(ds.audio, file_idx, t1, t2, p, fs, tt)

            same = bool(torch.equal(cached(), whole()))             # also the warm-up of both shapes
            _timed(cached, 3), _timed(whole, 3)
            b_ms, c_ms = [], []
            for _ in range(args.reps):                              # alternate within the same process
                b_ms.append(_timed(cached, args.iters))
                c_ms.append(_timed(whole, args.iters))
            b, c = _stats(b_ms), _stats(c_ms)
            entry["batches"].append({"batch": n, "bit_identical": same, "cache_path": b, "whole_motif_path": c,
                                     "speedup_median": round(c["median_ms"] / b["median_ms"], 2),
                                     "cache_not_slower_beyond_spread": b["min_ms"] <= c["max_ms"]})
        out["cases"].append(entry)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--files", str(args.files), "--iters", str(args.iters),
           "--reps", str(args.reps)]
    try:
        res = subprocess.run(cmd, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": "timed out after %d s" % args.timeout}))
        return 124
    return res.returncode


if __name__ == "__main__":
    sys.exit(main())
