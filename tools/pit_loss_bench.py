#!/usr/bin/env python3
"""Times the two loss kernels (csrc/train_step.hip: loss_kernel, loss_pit_kernel<3>) through the C ABI, forward + backward
as the training step calls them (perm and parts not requested), at the config-3 step (2048 rows = 32 x 64 frames, 14
classes x 3 slots) and at 32 times that.

One launch of either kernel is shorter than the host needs to enqueue it, so --launches of them are recorded into a HIP
graph (one stream: they run back to back, never overlapping) and the graph is replayed between two device events: the
figure is the time per launch on the device, launch gaps included.  A warm-up, then --reps replays per kernel with the two
kernels alternating; the median and the range are printed.  Bytes are the algorithmic ones: sed, doa and target read once,
both gradients written once.  Prints one JSON line per shape; for the time of the kernel alone, run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/pit_loss_bench.py`."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLASSES, OVERLAPS = 14, 3
SHAPES = (2048, 65536)


def recorded(fn, launches):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pit_loss_bench.py needs a HIP device")
    import bench
    pkg = importlib.import_module(bench.PKG)
    L = pkg._lib
    lib, p = L.lib(), L.ptr
    dev = torch.device("cuda:0")
    n_sed = CLASSES * OVERLAPS
    for rows in SHAPES:
        g = torch.Generator().manual_seed(rows)
        sed = torch.rand(rows, n_sed, generator=g).clamp(1e-4, 1 - 1e-4).to(dev)
        doa = (torch.rand(rows, 3 * n_sed, generator=g) * 2 - 1).to(dev)
        active = (torch.rand(rows, n_sed, generator=g) < 0.15).float()
        target = torch.cat((active, (torch.rand(rows, 3 * n_sed, generator=g) * 2 - 1) * active.repeat_interleave(3, 1)), 1).to(dev)
        loss, dsed, ddoa = torch.empty(1, device=dev), torch.empty_like(sed), torch.empty_like(doa)

        def plain():
            L.check(lib.seld_loss_fwd_bwd(p(sed), p(doa), p(target), rows, n_sed, 3 * n_sed, 1.0, 5.0, p(loss), p(dsed), p(ddoa),
                                          L.current_stream()), "seld_loss_fwd_bwd")

        def pit():
            L.check(lib.seld_loss_pit_fwd_bwd(p(sed), p(doa), p(target), rows, CLASSES, OVERLAPS, 1.0, 5.0, p(loss), p(dsed),
                                              p(ddoa), None, None, L.current_stream()), "seld_loss_pit_fwd_bwd")
        graphs = dict(plain=recorded(plain, a.launches), pit=recorded(pit, a.launches))
        for gr in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
        times = dict(plain=[], pit=[])
        for _ in range(a.reps):
            for name, gr in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gr.replay()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        nbytes = 4 * rows * (2 * 4 * n_sed + 4 * n_sed)
        out = dict(op="loss", rows=rows, classes=CLASSES, overlaps=OVERLAPS, launches_per_replay=a.launches, reps=a.reps,
                   bytes_read_plus_written=nbytes)
        for name, ts in times.items():
            us = statistics.median(ts)
            out[name] = dict(us_per_launch=round(us, 2), us_min_max=[round(min(ts), 2), round(max(ts), 2)],
                             GBps=round(nbytes / (us * 1e-6) / 1e9, 1))
        out["pit_over_plain"] = round(out["pit"]["us_per_launch"] / out["plain"]["us_per_launch"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
