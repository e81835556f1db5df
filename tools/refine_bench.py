"""Wall time of the segment refinement (row f10) on one MI355X: ``get_specs`` over synthetic recordings and segment
files, the ``TransformableUMAP`` fit of the flattened spectrograms, and one ``transform`` of the segments of one
directory; with ``--cpu N`` also the numpy restatement of the transform (tests/refine_cases.py) of N rows against the
same training rows, on the host.  Prints one JSON line.

    python tools/refine_bench.py --segments 10000 [--seconds 0.1] [--cpu 50]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--seconds", type=float, default=0.1, help="length of every segment")
    ap.add_argument("--per-file", type=int, default=50, help="segments per recording")
    ap.add_argument("--dirs", type=int, default=4)
    ap.add_argument("--cpu", type=int, default=0, help="rows of the host restatement of transform (0: skip)")
    args = ap.parse_args()
    import torch
    from scipy.io import wavfile
    from ava_amd import refine_segments as R
    from ava_amd import synthetic as syn

    p = dict(fs=32000, nperseg=256, noverlap=128, min_freq=400, max_freq=10e3, spec_min_val=2.0, spec_max_val=6.0)
    n_files = -(-args.segments // args.per_file)
    gap = 0.02
    dur = args.per_file * (args.seconds + gap) + gap
    segs = np.stack([gap + (args.seconds + gap) * np.arange(args.per_file),
                     gap + (args.seconds + gap) * np.arange(args.per_file) + args.seconds], 1)
    with tempfile.TemporaryDirectory() as root:
        audio_dirs = [os.path.join(root, "audio_%d" % d) for d in range(args.dirs)]
        seg_dirs = [os.path.join(root, "segs_%d" % d) for d in range(args.dirs)]
        for d in audio_dirs + seg_dirs:
            os.makedirs(d)
        for f in range(n_files):
            audio, _ = syn.recordings(n_files=1, fs=p['fs'], seconds=dur, salt=7000 + f)
            d = f % args.dirs
            wavfile.write(os.path.join(audio_dirs[d], "rec_%05d.wav" % f), p['fs'], audio[0])
            np.savetxt(os.path.join(seg_dirs[d], "rec_%05d.txt" % f), segs, fmt='%.5f', header="Onsets/offsets")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        specs, max_len, _ = R.get_specs(audio_dirs, seg_dirs, p, max_num_specs=args.segments)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        transform, emb = R.embed(specs)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        one, _, _ = R.get_specs(audio_dirs[:1], seg_dirs[:1], p, max_len=max_len)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        rows = one.reshape(len(one), -1)
        Y = transform.transform(rows)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
    out = dict(segments=len(specs), row_length=int(specs.shape[1] * specs.shape[2]), max_len=max_len,
               get_specs_s=round(t1 - t0, 3), fit_s=round(t2 - t1, 3), transform_rows=len(one),
               transform_get_specs_s=round(t3 - t2, 3), transform_s=round(t4 - t3, 3),
               finite=bool(np.isfinite(emb).all() and np.isfinite(Y).all()))
    if args.cpu:
        import refine_cases as RC
        q = rows[:args.cpu].cpu().numpy().astype(np.float32)
        train = specs.reshape(len(specs), -1).cpu().numpy().astype(np.float32)
        t5 = time.perf_counter()
        want = RC.transform(q, train, emb, int(transform._n_neighbors), transform.a_, transform.b_)
        out.update(cpu_restatement_rows=len(q), cpu_restatement_s=round(time.perf_counter() - t5, 3),
                   cpu_vs_device_max_abs=float(np.abs(want - transform.transform(q)).max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
