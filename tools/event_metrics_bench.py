#!/usr/bin/env python3
"""Times the scoring of event lists (csrc/event_metrics.hip, hip_ops.score_events) on 500 recordings x 600 frames x 42
slots decoded at about 5 % and about 50 % active slots, beside the fused dense path (hip_ops.metrics_accumulate) on the
tensors the lists were decoded from.  On every run the 13 shared counters of the two must be equal.

HIP events around the call, a warm-up, the median of `--reps` runs.  `flags` is passed, so the timed call makes no host
read.  Bytes are the algorithmic ones: every 40-byte row read once by the scoring kernel and its frame and class (16 bytes)
once more by the checking kernel, plus the offsets.  Rates are given as a fraction of the 6.3 TB/s float4-copy ceiling of
DESIGN.md.  Prints one JSON line per density.

--max_tracks N (1 .. 8) times the same lists with that association limit (above 3: the wave-per-cell instantiation; the
decoded lists hold no cell above 3, so this is what asking for more costs them).  --coords 2 turns the rows into
[frame, class, azimuth, elevation] in degrees first; the Euclidean counters then have no counterpart in the fused path,
and the ten DCASE21 counters are compared instead."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

H = seld_amd.hip_ops
COPY_CEILING = 6.3e12
dev = torch.device("cuda:0")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=500)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--coords", type=int, default=3, choices=(2, 3))
    ap.add_argument("--max_tracks", type=int, default=3)
    a = ap.parse_args()
    kw = {}
    if (a.coords, a.max_tracks) != (3, 3):              # the plain call otherwise: this file also times trees without them
        kw = dict(coords=a.coords, max_tracks=a.max_tracks)
    row_bytes = 8 * (2 + a.coords)
    R, T, n = a.recordings, a.frames, 42
    for density in (0.05, 0.5):
        g = torch.Generator().manual_seed(3)

        def dense():
            u = torch.rand(R, T, n, generator=g)
            act = torch.where(u < density, 0.5 + 0.5 * u / density + 0.001, 0.499 * (u - density) / (1 - density))
            return act.to(dev), (torch.rand(R, T, 3 * n, generator=g) * 2 - 1).to(dev)
        sed, doa = dense()
        t_act, t_loc = dense()
        target = torch.cat((t_act, t_loc), -1).contiguous()
        pr, _, po = H.decode_events(sed, doa)
        tr, _, to = H.decode_events(t_act, t_loc)
        if a.coords == 2:
            def degrees(r):
                az = torch.atan2(r[:, 3], r[:, 2]) * (180 / torch.pi)
                el = torch.atan2(r[:, 4], torch.hypot(r[:, 2], r[:, 3])) * (180 / torch.pi)
                return torch.stack((r[:, 0], r[:, 1], az, el), 1).contiguous()
            pr, tr = degrees(pr), degrees(tr)
        fused = H.metrics_new(dev)
        H.metrics_accumulate(fused, sed, doa, target, T)
        acc = H.score_events(H.event_metrics_new(dev), pr, po, tr, to, T, **kw)
        first = 3 if a.coords == 2 else 0
        same = acc[0][first:13].tolist() == fused[0][first:].tolist()
        de_err = abs(float(acc[1]) - float(fused[1])) / max(1.0, abs(float(fused[1])))
        if a.coords == 3 and (not same or de_err > 1e-12):  # (the degrees are a conversion: their agreement is reported only)
            raise SystemExit(f"score_events disagrees with metrics_accumulate: {acc[0].tolist()} / {fused[0].tolist()} / {de_err}")
        flags = torch.zeros(2, device=dev, dtype=torch.int64)
        scratch = H.event_metrics_new(dev)
        scratch_fused = H.metrics_new(dev)
        ev_us = timed(lambda: H.score_events(scratch, pr, po, tr, to, T, flags=flags, **kw), a.reps)
        fused_us = timed(lambda: H.metrics_accumulate(scratch_fused, sed, doa, target, T), a.reps)
        rows = pr.shape[0] + tr.shape[0]
        nbytes = rows * (row_bytes + 16) + 2 * (R + 1) * 8
        print(json.dumps(dict(
            shape=[R, T, n], density=density, coords=a.coords, max_tracks=a.max_tracks, pred_rows=pr.shape[0], true_rows=tr.shape[0], equals_fused_path=same,
            total_de_rel_err=de_err, score_events_us=round(ev_us[0], 1),
            score_events_us_min_max=[round(ev_us[1], 1), round(ev_us[2], 1)], bytes=nbytes,
            fraction_of_copy_ceiling=round(nbytes / (ev_us[0] * 1e-6) / COPY_CEILING, 4),
            fused_dense_path_us=round(fused_us[0], 1), fused_dense_path_us_min_max=[round(fused_us[1], 1), round(fused_us[2], 1)])),
            flush=True)


if __name__ == "__main__":
    main()
