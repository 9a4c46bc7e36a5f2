#!/usr/bin/env python3
"""Times track post-processing (csrc/smooth.hip, hip_ops.smooth_tracks) on a whole test set: (R, T, n) = (300, 600, 42),
i.e. 300 recordings of 600 frames, 14 classes x 3 slots.

smooth:   median = 7, min_frames = 3, max_gap = 2, doa = "weighted" (every stage of the kernel), and the identity settings
          (median = 1, on = off = 0.5, "frame": the kernel's floor; callers skip that launch).  HIP events around each of
          --reps calls after a warm-up; the median, the extremes, the algorithmic bytes (sed and doa read once, out_sed and
          out_doa written once) and the rate they give.
host:     the path this replaces: the track copied to the host, tests/smooth_ref.py (numpy, a loop over columns and runs)
          with the same settings, and the result copied back; wall time of one pass, the two copies included and also
          given on their own.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (300, 600, 42)
FULL = dict(median=7, on=0.5, off=0.5, min_frames=3, max_gap=2, doa="weighted")
IDENTITY = dict(median=1, on=0.5, off=0.5, min_frames=1, max_gap=0, doa="frame")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip_host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench.py needs a HIP device")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    import seld_amd
    from tests import smooth_ref
    H = seld_amd.hip_ops
    dev = torch.device("cuda:0")
    R, T, n = SHAPE
    sed, doa = smooth_ref.random_track(R, T, n, 1)
    sd, dd = torch.from_numpy(sed).to(dev), torch.from_numpy(doa).to(dev)
    nbytes = 2 * 4 * (sd.numel() + dd.numel())
    for name, kw in (("full", FULL), ("identity", IDENTITY)):
        for _ in range(3):
            out = H.smooth_tracks(sd, dd, **kw)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = H.smooth_tracks(sd, dd, **kw)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        med = statistics.median(us)
        print(json.dumps(dict(op="smooth_tracks", settings=name, shape=SHAPE, reps=a.reps, us=round(med, 1),
                              us_min_max=[round(min(us), 1), round(max(us), 1)], bytes_read_plus_written=nbytes,
                              GBps=round(nbytes / (med * 1e-6) / 1e9, 1), active_fraction=round(float(out[0].mean()), 4),
                              **{k: v for k, v in kw.items()})), flush=True)
    if a.skip_host:
        return
    kw = {k: v for k, v in FULL.items() if k != "doa"}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hs, hd = sd.cpu().numpy(), dd.cpu().numpy()
    t1 = time.perf_counter()
    ref = smooth_ref.smooth(hs, hd, doa_mode=FULL["doa"], **kw)
    t2 = time.perf_counter()
    back = torch.from_numpy(ref["sed"]).to(dev), torch.from_numpy(ref["doa"].astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    same = bool(torch.equal(back[0], H.smooth_tracks(sd, dd, **FULL)[0]))
    print(json.dumps(dict(op="host_path", settings="full", shape=SHAPE, ms=round((t3 - t0) * 1e3, 1),
                          copy_to_host_ms=round((t1 - t0) * 1e3, 2), numpy_ms=round((t2 - t1) * 1e3, 1),
                          copy_to_device_ms=round((t3 - t2) * 1e3, 2), events=len(ref["runs"]),
                          activity_equals_the_kernels=same)), flush=True)


if __name__ == "__main__":
    main()
