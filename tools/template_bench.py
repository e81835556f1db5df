"""Device template segmentation (ava_amd.template_segmentation) on one hour of synthetic
32 kHz int16 song: 60 files x 60 s in one DeviceAudio, finch parameters (nperseg 512, noverlap 256, 400 Hz - 10 kHz)
and a 0.5 s template (F = 153, L = 63) made from synthetic exemplars.  Prints one JSON line: the upload time, the
device time of the spectrogram and correlation launches (HIP events, median of --reps after a warm-up), the whole
segment_batch call (host decisions and copies included) and lags per second.

    python tools/template_bench.py [--files 60] [--seconds 60] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=60)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    from ava_amd import segment as S, synthetic as syn, template_segmentation as TS
    from ava_amd.spec import DeviceAudio

    fs = 32000
    p = dict(fs=fs, nperseg=512, noverlap=256, min_freq=400, max_freq=10e3, spec_min_val=2.0, spec_max_val=6.5)
    ex, songs, _ = syn.songs(n_exemplars=4, n_songs=4, fs=fs, seconds=15.0, motif_seconds=0.5, renditions=16)
    template = TS.get_template_from_audio([a[:15872] for a in ex], p)               # 63 frames of 256
    n = int(fs * args.seconds)
    pool = np.concatenate(songs)
    audio = [np.roll(np.tile(pool, 1 + n // len(pool)), 7919 * i)[:n].copy() for i in range(args.files)]
    nbytes = sum(a.nbytes for a in audio)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = DeviceAudio(audio)
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0

    def device_pass():
        band = TS._band(dev, p)
        keep = band[4] - template.shape[1] >= 5
        return band, keep

    band, keep = device_pass()
    TS._xcorr(band, template, keep)
    lags = int(np.where(keep, band[4] - template.shape[1], 0).sum())
    spec_ms, xcorr_ms = [], []
    for _ in range(args.reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        band = TS._band(dev, p)
        e[1].record()
        trace, _ = TS._xcorr(band, template, keep)          # its copy to the host synchronises after e[2]'s work
        e[2].record()
        e[2].synchronize()
        spec_ms.append(e[0].elapsed_time(e[1]))
        xcorr_ms.append(e[1].elapsed_time(e[2]))
    call_s = []
    for _ in range(max(3, args.reps // 2)):
        t0 = time.perf_counter()
        res = TS.segment_batch(dev, template, p)
        call_s.append(time.perf_counter() - t0)
    F, L = template.shape
    xm = float(np.median(xcorr_ms))
    print(json.dumps({
        "workload": "template segmentation, %d files x %g s of %d Hz int16, template %d x %d" % (
            args.files, args.seconds, fs, F, L),
        "audio_bytes": nbytes, "frames": int(band[3][-1]), "lags": lags,
        "segments": int(sum(len(r) for r in res)),
        "upload_ms": round(upload * 1e3, 2), "spec_ms_median": round(float(np.median(spec_ms)), 3),
        "xcorr_ms_median": round(xm, 3), "xcorr_ms_all": [round(x, 3) for x in xcorr_ms],
        "call_ms_median": round(float(np.median(call_s)) * 1e3, 2),
        "lags_per_s": round(lags / (xm * 1e-3), 1),
        "xcorr_fp64_flop": 3 * F * L * lags,
        "xcorr_fp64_tflops": round(3 * F * L * lags / (xm * 1e-3) / 1e12, 2)}))


if __name__ == "__main__":
    main()
