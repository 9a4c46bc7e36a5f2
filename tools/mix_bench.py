#!/usr/bin/env python3
"""Times the gather that mixes two clips (csrc/loader.hip, hip_ops.gather_rows_mix) at the config-1 shape with phase.

One batch (32 x 16 x 128 x 512 fp32 predictors, two microphones [magnitude | phase], + 32 x 64 x 168 targets with sparse
events) out of a resident array of --rows samples in a shuffled order.  On the same arrays, in the same run:
  gather_rows              the plain gather
  gather_rows_aug_masks    hip_ops.gather_rows_aug with two frequency masks (up to 16 bins) and two time masks (up to 64 frames)
  gather_rows_polar        hip_ops.gather_rows_polar, every sample rotated (p_rot = 1), standardised predictors: the
                           neighbour that the mix is compared with (per position three sincosf and three atan2f for six
                           channels; the mix has two and one for two channels of two rows)
  gather_rows_mix_p0_masks p_mix = 0 with the masks of gather_rows_aug_masks: what the flag costs a sample that draws nothing
  gather_rows_mix_half     p_mix = 0.5, standardised, with the occupancy table
  gather_rows_mix          p_mix = 1, standardised, no occupancy table: every sample mixed
  gather_rows_mix_half_raw / gather_rows_mix_raw   the same two on raw predictors (stats None: no affine steps)
The calls ALTERNATE, --rounds times --reps calls each, HIP events around each call after a warm-up; per name the median
over all calls, the extremes, and the medians of the single rounds.  Bytes are the algorithmic ones: every batch byte read
once and written once, and for a mixed sample its partner's rows read as well (the number of mixed samples is counted from
the batch).  Prints one JSON line."""
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
BATCH, X_SHAPE, Y_SHAPE, OVERLAPS = 32, (16, 128, 512), (64, 168), 3
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
        raise SystemExit("mix_bench.py needs a HIP device")
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
    n_sed = Y_SHAPE[1] // 4
    act = (torch.rand((a.rows, Y_SHAPE[0], n_sed), generator=g) < 0.02).float()
    loc = (torch.rand((a.rows, Y_SHAPE[0], 3 * n_sed), generator=g) * 2 - 1) * act.repeat_interleave(3, 2)
    y_all = torch.cat([act, loc], 2).to(dev)
    index = torch.randperm(a.rows, generator=g).to(dev)
    out_x, out_y = torch.empty((BATCH,) + X_SHAPE, device=dev), torch.empty((BATCH,) + Y_SHAPE, device=dev)
    cursor = torch.ones(1, device=dev, dtype=torch.int32)
    epoch = torch.zeros(1, device=dev, dtype=torch.int32)
    stats = torch.tensor(STATS, device=dev)
    occ = H.target_occupancy(y_all, OVERLAPS)
    masks = dict(freq_masks=2, freq_width=16, time_masks=2, time_width=64)
    aug_masks = H.Augment(device=dev, **masks)
    polar = H.Augment(rot_polar=H.foa_polar(mics=2), p_rot=1.0, device=dev)
    mix0, mix_half, mix_all = (H.Augment(p_mix=0.0, device=dev, **masks), H.Augment(p_mix=0.5, device=dev), H.Augment(p_mix=1.0, device=dev))
    where = dict(epoch=epoch, seed=1, cursor=cursor)
    mix = lambda x, aug, **kw: H.gather_rows_mix(x, y_all, index, out_x, out_y, augment=aug, overlaps=OVERLAPS, **kw, **where)
    calls = dict(
        gather_rows=lambda: H.gather_rows(x_all, y_all, index, out_x, out_y, cursor=cursor),
        gather_rows_aug_masks=lambda: H.gather_rows_aug(x_all, y_all, index, out_x, out_y, augment=aug_masks, **where),
        gather_rows_polar=lambda: H.gather_rows_polar(x_all, y_all, index, out_x, out_y, augment=polar, stats=stats, **where),
        gather_rows_mix_p0_masks=lambda: mix(x_all, mix0, stats=stats, occupancy=occ),
        gather_rows_mix_half=lambda: mix(x_all, mix_half, stats=stats, occupancy=occ),
        gather_rows_mix=lambda: mix(x_all, mix_all, stats=stats),
        gather_rows_mix_half_raw=lambda: mix(raw, mix_half, occupancy=occ),
        gather_rows_mix_raw=lambda: mix(raw, mix_all))
    # the mixed batch against torch (complex64) with explicit partners and gains, at the size that is timed
    partners = ((torch.arange(BATCH) + BATCH + 7) % a.rows).to(dev)                # positions outside this batch's own
    gains = (torch.rand(BATCH, generator=g) * 0.5 + 0.5).to(dev)
    H.gather_rows_mix(raw, y_all, index, out_x, out_y, augment=mix_all, overlaps=OVERLAPS, partners=partners, gains=gains, **where)
    za = raw[index[BATCH:2 * BATCH]]
    zb = raw[index[partners]]
    want = torch.polar(za[:, :half_c], za[:, half_c:]) + gains.view(-1, 1, 1, 1) * torch.polar(zb[:, :half_c], zb[:, half_c:])
    err = float((torch.polar(out_x[:, :half_c], out_x[:, half_c:]) - want).abs().max())
    del za, zb, want
    mixed = {}
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        src = raw if name.endswith("raw") else x_all
        mixed[name] = int((out_x != src[index[BATCH:2 * BATCH]]).flatten(1).any(1).sum()) if "mix" in name and "p0" not in name else 0
    torch.cuda.synchronize()
    times = {name: [[] for _ in range(a.rounds)] for name in calls}
    for r in range(a.rounds):
        for _ in range(a.reps):
            for name, fn in calls.items():
                times[name][r].append(timed_once(fn))
    row_bytes = 4 * (out_x[0].numel() + out_y[0].numel())
    runs = {}
    for name, rounds in times.items():
        flat = [t for rr in rounds for t in rr]
        us = statistics.median(flat)
        nbytes = row_bytes * (2 * BATCH + mixed[name])
        runs[name] = dict(us=round(us, 1), us_min_max=[round(min(flat), 1), round(max(flat), 1)],
                          us_round_medians=[round(statistics.median(rr), 1) for rr in rounds], mixed_samples=mixed[name],
                          bytes_read_plus_written=nbytes, GBps=round(nbytes / (us * 1e-6) / 1e9, 1),
                          fraction_of_copy_ceiling=round(nbytes / (us * 1e-6) / COPY_CEILING, 3),
                          fraction_of_hbm_peak=round(nbytes / (us * 1e-6) / 8e12, 3))
    for r in runs.values():
        r["time_over_gather_rows_polar"] = round(r["us"] / runs["gather_rows_polar"]["us"], 3)
    print(json.dumps(dict(op="gather_mix", rows=a.rows, batch=BATCH, x_shape=list(X_SHAPE), reps=a.reps, rounds=a.rounds,
                          max_abs_complex_error_against_torch=err, **runs)), flush=True)


if __name__ == "__main__":
    main()
