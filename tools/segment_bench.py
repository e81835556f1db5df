"""Device amplitude segmentation (ava_amd.segment) on one hour of synthetic 250 kHz int16
audio: 60 files x 60 s in one DeviceAudio, mouse parameters (examples/mouse_sylls_mwe.py), sum mode.  Prints one JSON
line: the upload time, the device time of the trace + decision launches (HIP events, median of --reps after a warm-up),
the whole get_onsets_offsets_batch call (host chain and copies included) and frames per second.

    python tools/segment_bench.py [--files 60] [--seconds 60] [--reps 7]
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
    from ava_amd import segment as S, synthetic as syn
    from ava_amd.spec import DeviceAudio

    fs = 250000
    p = dict(fs=fs, nperseg=1024, noverlap=512, min_freq=30e3, max_freq=110e3, spec_min_val=2.0, spec_max_val=6.0,
             th_1=2.0, th_2=5.0, th_3=10.0, min_dur=0.03, max_dur=0.3, smoothing_timescale=0.007, softmax=False,
             temperature=0.5)
    one, _ = syn.recordings(n_files=4, fs=fs, seconds=args.seconds / 1.39, dtype=np.int16)   # tiled to 60 s files
    n = int(fs * args.seconds)
    pool = np.concatenate(one)
    audio = [np.roll(pool, 7919 * i)[:n].copy() for i in range(args.files)]
    nbytes = sum(a.nbytes for a in audio)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = DeviceAudio(audio)
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0

    _, frame_off = S._frame_offsets(dev.lengths, p['nperseg'], p['noverlap'])
    frames = int(frame_off[-1])
    dt = S.frame_step(fs, p['nperseg'], p['noverlap'])

    def device_pass():
        trace, fo, _ = S._trace(dev, frame_off, p, dt)
        return S._decide(trace, frame_off, fo, p)        # its count read synchronises

    device_pass()
    dev_ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        trace, fo, _ = S._trace(dev, frame_off, p, dt)
        lib = S._lib.load()
        cnt = torch.zeros(1, dtype=torch.int64, device=trace.device)
        buf = torch.empty((3, frames), dtype=torch.int64, device=trace.device)
        th = S.decide_thresholds(p, np.float32)
        S._lib.check(lib.ava_amp_decide(trace.data_ptr(), 0, fo.data_ptr(), len(dev), frames, th[0], th[1], th[2],
                                        cnt.data_ptr(), buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(),
                                        frames, S._lib.stream()), "ava_amp_decide")
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    call_s = []
    for _ in range(max(3, args.reps // 2)):
        t0 = time.perf_counter()
        res = S.get_onsets_offsets_batch(dev, p)
        call_s.append(time.perf_counter() - t0)
    med = float(np.median(dev_ms))
    print(json.dumps({
        "workload": "amplitude segmentation, %d files x %g s of %d Hz int16" % (args.files, args.seconds, fs),
        "audio_bytes": nbytes, "frames": frames, "syllables": int(sum(len(r[0]) for r in res)),
        "upload_ms": round(upload * 1e3, 2), "device_ms_median": round(med, 3),
        "device_ms_all": [round(x, 3) for x in dev_ms], "call_ms_median": round(float(np.median(call_s)) * 1e3, 2),
        "frames_per_s": round(frames / (med * 1e-3), 1)}))


if __name__ == "__main__":
    main()
