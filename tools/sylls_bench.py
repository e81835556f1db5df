"""Wall time of the syllable path (row f11) on one MI355X: ``preprocess.syllables_to_device`` over synthetic mouse-like
recordings (250 kHz int16, ``nperseg`` 1024, syllables of ``--seconds``) in syllables/s, and the per-batch cost of
``ava_gather_rows_f32`` at ``B = 256`` rows of 128 x 128 from a float32 and from a float64 dataset; for information the
same batch as ``torch.index_select(...).float()``.  Prints one JSON line.

    python tools/sylls_bench.py --syllables 20000 [--seconds 0.06] [--per-file 200] [--rows 8192]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--syllables", type=int, default=20000)
    ap.add_argument("--seconds", type=float, default=0.06, help="length of every syllable")
    ap.add_argument("--per-file", type=int, default=200, help="syllables per recording")
    ap.add_argument("--rows", type=int, default=8192, help="rows of the resident dataset the gather draws from")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import torch
    from scipy.io import wavfile
    from ava_amd import preprocess as P
    from ava_amd import syllable_dataset as SD
    from ava_amd import synthetic as syn

    p = dict(syn.MOUSE_PARAMS, max_dur=0.2, time_stretch=True, sylls_per_file=20, max_num_syllables=None,
             normalize_quantile=0.5)
    fs = p['fs']
    n_files = -(-args.syllables // args.per_file)
    gap = 0.02
    dur = args.per_file * (args.seconds + gap) + gap
    onsets = gap + (args.seconds + gap) * np.arange(args.per_file)
    segs = np.stack([onsets, onsets + args.seconds], 1)
    with tempfile.TemporaryDirectory() as root:
        audio_dir, seg_dir = os.path.join(root, "audio"), os.path.join(root, "segs")
        os.makedirs(audio_dir)
        os.makedirs(seg_dir)
        base, _ = syn.recordings(n_files=1, fs=fs, seconds=dur, salt=7000)
        for f in range(n_files):
            wavfile.write(os.path.join(audio_dir, "rec_%05d.wav" % f), fs, np.roll(base[0], 977 * f))
            np.savetxt(os.path.join(seg_dir, "rec_%05d.txt" % f), segs, fmt='%.5f', header="Onsets/offsets")
        P.syllables_to_device([audio_dir], [seg_dir], dict(p, max_num_syllables=p['sylls_per_file']))     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = P.syllables_to_device([audio_dir], [seg_dir], p)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
    out = dict(syllables=len(store), audio_seconds=round(n_files * dur, 1), to_device_s=round(t1 - t0, 3),
               syllables_per_s=round(len(store) / (t1 - t0), 1), finite=bool(torch.isfinite(store.specs).all()))
    del store

    gen = torch.Generator().manual_seed(0)
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        data = torch.rand((args.rows, 128, 128), device="cuda").to(dtype)
        ds = SD.DeviceSyllableDataset.from_arrays(data)
        lists = [torch.randperm(args.rows, generator=gen)[:args.batch] for _ in range(args.iters)]
        dst = torch.empty((args.batch, 128, 128), device="cuda")

        def timed(fn):
            for idx in lists[:10]:
                fn(idx)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for idx in lists:
                fn(idx)
            torch.cuda.synchronize()
            return round((time.perf_counter() - t) / len(lists) * 1e6, 2)

        host_lists = {id(i): i.tolist() for i in lists}
        dev_lists = {id(i): i.cuda() for i in lists}
        out["gather_%s_us" % name] = timed(lambda idx: ds.gather(host_lists[id(idx)], out=dst))
        out["index_select_%s_us" % name] = timed(lambda idx: torch.index_select(data, 0, dev_lists[id(idx)]).float())
        want = torch.index_select(data, 0, dev_lists[id(lists[0])]).float()
        out["equal_%s" % name] = bool(torch.equal(ds.gather(host_lists[id(lists[0])]), want))
        out["gather_%s_gbps" % name] = round(args.batch * 16384 * (data.element_size() + 4) /
                                             out["gather_%s_us" % name] / 1e3, 1)
        del ds, data
    print(json.dumps(out))


if __name__ == "__main__":
    main()
