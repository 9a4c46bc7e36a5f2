#!/usr/bin/env python3
"""Times the gather with a rotation of the sound field (csrc/loader.hip, hip_ops.gather_rows_rot) at config 3.

One batch (32 x 8 x 128 x 512 fp32 predictors + 32 x 64 x 168 targets) out of a resident array of --rows samples in a
shuffled order, the 8 channels read as the quaternion layout of 2 microphones.  On the same arrays, in the same run:
  gather_rows_aug_swap   hip_ops.gather_rows_aug with the 16-row quaternion preset at p_swap = 1 (the yardstick: the same
                         bytes, a signed permutation instead of a 3 x 3 mix)
  gather_rows_rot        every sample rotated (p_rot = 1, mirror and z-flip on)
  gather_rows_rot_half   p_rot = 0.5 with two frequency masks (up to 16 bins) and two time masks (up to 64 frames)
  gather_rows_rot_matrices  explicit matrices, one per sample
  gather_rows            the plain gather
The calls ALTERNATE, --rounds times --reps calls each, HIP events around each call after a warm-up; per name the median
over all calls, the extremes, and the medians of the single rounds (their spread is the run-to-run spread inside one
session).  Bytes are the algorithmic ones (every batch byte read once and written once).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.3e12       # bytes/s read + written of a float4 copy kernel on an MI355X (8 TB/s is the HBM3E spec)
BATCH, X_SHAPE, Y_SHAPE = 32, (8, 128, 512), (64, 168)


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
    ap.add_argument("--rows", type=int, default=256, help="samples in the resident array (2 MB each)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rot_bench.py needs a HIP device")
    import seld_amd
    H = seld_amd.hip_ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x_all = torch.randn((a.rows,) + X_SHAPE, generator=g).to(dev)
    y_all = torch.randn((a.rows,) + Y_SHAPE, generator=g).to(dev)
    index = torch.randperm(a.rows, generator=g).to(dev)
    out_x, out_y = torch.empty((BATCH,) + X_SHAPE, device=dev), torch.empty((BATCH,) + Y_SHAPE, device=dev)
    cursor = torch.ones(1, device=dev, dtype=torch.int32)
    epoch = torch.zeros(1, device=dev, dtype=torch.int32)
    triples = H.foa_triples(mics=2, layout="quaternion")
    swap = H.Augment(table=H.foa_transforms(mics=2, layout="quaternion"), p_swap=1.0, device=dev)
    rot = H.Augment(rot_triples=triples, p_rot=1.0, device=dev)
    half = H.Augment(rot_triples=triples, p_rot=0.5, freq_masks=2, freq_width=16, time_masks=2, time_width=64, device=dev)
    q, _ = torch.linalg.qr(torch.randn((BATCH, 3, 3), generator=g))
    matrices = q.reshape(BATCH, 9).contiguous().to(dev)
    where = dict(epoch=epoch, seed=1, cursor=cursor)
    calls = dict(
        gather_rows_aug_swap=lambda: H.gather_rows_aug(x_all, y_all, index, out_x, out_y, augment=swap, **where),
        gather_rows_rot=lambda: H.gather_rows_rot(x_all, y_all, index, out_x, out_y, augment=rot, **where),
        gather_rows_rot_half=lambda: H.gather_rows_rot(x_all, y_all, index, out_x, out_y, augment=half, **where),
        gather_rows_rot_matrices=lambda: H.gather_rows_rot(x_all, y_all, index, out_x, out_y, augment=rot, matrices=matrices, **where),
        gather_rows=lambda: H.gather_rows(x_all, y_all, index, out_x, out_y, cursor=cursor))
    # the rotated batch against torch on the same matrices, at the size that is timed
    calls["gather_rows_rot_matrices"]()
    batch = index[BATCH:2 * BATCH]
    want = x_all[batch].clone()
    m = matrices.view(BATCH, 3, 3)
    for t in triples:
        want[:, list(t)] = torch.einsum("baj,bjft->baft", m, x_all[batch][:, list(t)])
    err = float((out_x - want).abs().max())
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
        r["time_over_aug_swap"] = round(r["us"] / runs["gather_rows_aug_swap"]["us"], 3)
    print(json.dumps(dict(op="gather_rot", rows=a.rows, batch=BATCH, reps=a.reps, rounds=a.rounds, bytes_read_plus_written=nbytes,
                          max_abs_error_against_torch=err, **runs)), flush=True)


if __name__ == "__main__":
    main()
