#!/usr/bin/env python3
"""Times the breakdown by recording and class (hip_ops.score_events_by, hip_ops.metrics_accumulate_by) beside the plain
calls (hip_ops.score_events, hip_ops.metrics_accumulate) on a whole test set: the (R, T, n) = (300, 600, 42) track of
tools/smooth_bench.py as the prediction and a second draw of it as the reference, decoded for the event path.

HIP events around each of --reps calls after a warm-up; the median and the extremes.  `flags` is passed, so no timed call
reads anything back.  On every run row "all" of the tables, summed over the recordings, must equal the plain calls'
counters.  A tree without the breakdown calls (an earlier commit, to compare the plain calls against) is timed on the plain
calls alone.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (300, 600, 42)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return dict(us=round(statistics.median(us), 1), us_min_max=[round(min(us), 1), round(max(us), 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("class_metrics_bench.py needs a HIP device")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    import seld_amd
    from tests import smooth_ref
    H = seld_amd.hip_ops
    dev = torch.device("cuda:0")
    R, T, n = SHAPE
    sed, doa = (torch.from_numpy(x).to(dev) for x in smooth_ref.random_track(R, T, n, 1))
    t_act, t_loc = (torch.from_numpy(x).to(dev) for x in smooth_ref.random_track(R, T, n, 2))
    target = torch.cat((t_act, t_loc), -1).contiguous()
    pr, _, po = H.decode_events(sed, doa)
    tr, _, to = H.decode_events(t_act, t_loc)
    flags = torch.zeros(2, device=dev, dtype=torch.int64)
    ev_acc, dense_acc = H.event_metrics_new(dev), H.metrics_new(dev)
    out = dict(shape=list(SHAPE), reps=a.reps, pred_rows=pr.shape[0], true_rows=tr.shape[0],
               score_events=timed(lambda: H.score_events(ev_acc, pr, po, tr, to, T, flags=flags), a.reps),
               metrics_accumulate=timed(lambda: H.metrics_accumulate(dense_acc, sed, doa, target, T), a.reps))
    if hasattr(H, "score_events_by"):
        ev = H.score_events(H.event_metrics_new(dev), pr, po, tr, to, T)
        dense = H.metrics_accumulate(H.metrics_new(dev), sed, doa, target, T)
        tables = (torch.empty((R, 16, 16), device=dev, dtype=torch.int64), torch.empty((R, 16), device=dev, dtype=torch.float64))
        out["score_events_by"] = timed(lambda: H.score_events_by(pr, po, tr, to, T, flags=flags, out=tables), a.reps)
        ok = tables[0][:, -1].sum(0).tolist() == ev[0].tolist()
        out["metrics_accumulate_by"] = timed(lambda: H.metrics_accumulate_by(sed, doa, target, T, out=tables), a.reps)
        ok = ok and tables[0][:, -1, :13].sum(0).tolist() == dense[0].tolist()
        de_err = abs(float(tables[1][:, -1].sum()) - float(dense[1])) / max(1.0, abs(float(dense[1])))
        if not ok or de_err > 1e-12:
            raise SystemExit(f"rows 'all' disagree with the plain calls (total_de relative error {de_err})")
        out.update(rows_all_equal_the_plain_calls=ok, total_de_rel_err=de_err,
                   workspace_bytes=int(seld_amd._lib.lib().seld_metrics_breakdown_workspace(R, T, 14, 10)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
