#!/usr/bin/env python3
"""Times the rotating gather for magnitude-phase predictors (csrc/loader.hip, hip_ops.gather_rows_polar) at the config-1
shape with phase.

One batch (32 x 16 x 128 x 512 fp32 predictors, two microphones [magnitude | phase], + 32 x 64 x 168 targets) out of a
resident array of --rows samples in a shuffled order.  On the same arrays, in the same run:
  gather_rows              the plain gather
  gather_rows_rot          hip_ops.gather_rows_rot with four channel triples over the same 12 directional channels, p_rot = 1
                           (the same bytes through a 3 x 3 real mix: what the transcendentals are measured against)
  gather_rows_polar        every sample rotated (p_rot = 1), standardised predictors (stats given)
  gather_rows_polar_raw    the same on raw predictors (stats None: no affine steps)
  gather_rows_polar_half   p_rot = 0.5 with two frequency masks (up to 16 bins) and two time masks (up to 64 frames), stats given
The calls ALTERNATE, --rounds times --reps calls each, HIP events around each call after a warm-up; per name the median
over all calls, the extremes, and the medians of the single rounds.  Bytes are the algorithmic ones (every batch byte
read once and written once).  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.3e12       # bytes/s read + written of a float4 copy kernel on an MI355X (8 TB/s is the HBM3E spec)
BATCH, X_SHAPE, Y_SHAPE = 32, (16, 128, 512), (64, 168)
STATS = (2.5, 3.1, 0.01, 1.8)


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per name and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=128, help="samples in the resident array (4 MB each)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("polar_bench.py needs a HIP device")
    import seld_amd
    H = seld_amd.hip_ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    half_c = X_SHAPE[0] // 2
    mag = torch.randn((a.rows, half_c) + X_SHAPE[1:], generator=g).abs() * 3
    phase = (torch.rand((a.rows, half_c) + X_SHAPE[1:], generator=g) * 2 - 1) * math.pi
    raw = torch.cat([mag, phase], 1).to(dev)
    x_all = torch.cat([(mag - STATS[0]) / STATS[1], (phase - STATS[2]) / STATS[3]], 1).to(dev)
    del mag, phase
    y_all = torch.randn((a.rows,) + Y_SHAPE, generator=g).to(dev)
    index = torch.randperm(a.rows, generator=g).to(dev)
    out_x, out_y = torch.empty((BATCH,) + X_SHAPE, device=dev), torch.empty((BATCH,) + Y_SHAPE, device=dev)
    cursor = torch.ones(1, device=dev, dtype=torch.int32)
    epoch = torch.zeros(1, device=dev, dtype=torch.int32)
    stats = torch.tensor(STATS, device=dev)
    groups = H.foa_polar(mics=2)
    triples = [g6[:3] for g6 in groups] + [g6[3:] for g6 in groups]
    rot = H.Augment(rot_triples=triples, p_rot=1.0, device=dev)
    polar = H.Augment(rot_polar=groups, p_rot=1.0, device=dev)
    half = H.Augment(rot_polar=groups, p_rot=0.5, freq_masks=2, freq_width=16, time_masks=2, time_width=64, device=dev)
    where = dict(epoch=epoch, seed=1, cursor=cursor)
    calls = dict(
        gather_rows=lambda: H.gather_rows(x_all, y_all, index, out_x, out_y, cursor=cursor),
        gather_rows_rot=lambda: H.gather_rows_rot(x_all, y_all, index, out_x, out_y, augment=rot, **where),
        gather_rows_polar=lambda: H.gather_rows_polar(x_all, y_all, index, out_x, out_y, augment=polar, stats=stats, **where),
        gather_rows_polar_raw=lambda: H.gather_rows_polar(raw, y_all, index, out_x, out_y, augment=polar, **where),
        gather_rows_polar_half=lambda: H.gather_rows_polar(x_all, y_all, index, out_x, out_y, augment=half, stats=stats, **where))
    # the rotated batch against torch (complex64) with the same explicit matrices, at the size that is timed
    q, _ = torch.linalg.qr(torch.randn((BATCH, 3, 3), generator=g))
    matrices = q.reshape(BATCH, 9).contiguous().to(dev)
    H.gather_rows_polar(raw, y_all, index, out_x, out_y, augment=polar, matrices=matrices, **where)
    batch = raw[index[BATCH:2 * BATCH]]
    err = 0.0
    for g6 in groups:
        z = torch.polar(batch[:, list(g6[:3])], batch[:, list(g6[3:])])
        want = torch.einsum("baj,bjft->baft", matrices.view(BATCH, 3, 3).to(torch.complex64), z)
        got = torch.polar(out_x[:, list(g6[:3])], out_x[:, list(g6[3:])])
        err = max(err, float((got - want).abs().max()))
    del batch, z, want, got
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [[] for _ in range(a.rounds)] for name in calls}
    for r in range(a.rounds):
        for _ in range(a.reps):
            for name, fn in calls.items():
                times[name][r].append(timed_once(fn))
    nbytes = 2 * 4 * (out_x.numel() + out_y.numel())
    runs = {}
    for name, rounds in times.items():
        flat = [t for rr in rounds for t in rr]
        us = statistics.median(flat)
        runs[name] = dict(us=round(us, 1), us_min_max=[round(min(flat), 1), round(max(flat), 1)],
                          us_round_medians=[round(statistics.median(rr), 1) for rr in rounds],
                          GBps=round(nbytes / (us * 1e-6) / 1e9, 1), fraction_of_copy_ceiling=round(nbytes / (us * 1e-6) / COPY_CEILING, 3),
                          fraction_of_hbm_peak=round(nbytes / (us * 1e-6) / 8e12, 3))
    for r in runs.values():
        r["time_over_gather_rows_rot"] = round(r["us"] / runs["gather_rows_rot"]["us"], 3)
    print(json.dumps(dict(op="gather_polar", rows=a.rows, batch=BATCH, x_shape=list(X_SHAPE), reps=a.reps, rounds=a.rounds,
                          bytes_read_plus_written=nbytes, max_abs_complex_error_against_torch=err, **runs)), flush=True)


if __name__ == "__main__":
    main()
