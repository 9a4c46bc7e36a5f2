#!/usr/bin/env python3
"""Times the optimiser's launches (csrc/train_step.hip: adam_kernel; csrc/optim.hip: adam_ex_kernel, grad_norm_kernel) over
flat buffers of the benchmark's default workload's parameter count (bench.py c3).  The yardstick is bytes moved per
element, in 4-byte words, against plain Adam timed in the same run:

  adam (seld_adam_flat)                     read p g m v, write p m v          7 words
  adam_ex, extras off / clip / decoupled    the same                           7 words
  adam_ex with the moving average           + read ema, write ema              9 words
  adam_ex with all three                    the same                           9 words
  grad_norm                                 read g                             1 word

HIP events around bursts of --burst back-to-back launches of one variant through the C ABI (a single launch of a few
microseconds is below what a pair of events resolves), all variants alternating inside every repetition, after a warm-up
of each; the time per launch therefore includes the boundary between two dependent launches, as it does in a training step.
Reported per variant: the median microseconds per launch (with min and max), the achieved bytes per second, and `ratio`,
its median over plain Adam's median, beside `words_ratio`, the ratio of the bytes.  The buffers (a few MB each) stay in the
Infinity Cache between launches, as they do between the last backward kernels and the optimiser in a training step; a launch
of a few microseconds is also close to the launch floor, so a ratio above the ratio of the bytes is to be expected for
the norm, which moves one seventh of the bytes and still pays one launch and one ticketed reduction.

--n: another element count.  Prints ONE JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def c3_parameter_count():
    import bench
    import seld_amd
    model = seld_amd.model.SELD_Model(**bench.model_kwargs(bench.WORKLOADS["c3"], 128))
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--burst", type=int, default=20, help="launches per timed window")
    ap.add_argument("--n", type=int, default=0, help="elements per buffer (default: the c3 model's parameter count)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py needs a HIP device")
    if a.reps < 20 or a.burst < 1:
        raise SystemExit("at least 20 repetitions of at least one launch")
    import seld_amd
    L = seld_amd._lib
    lib, p = L.lib(), L.ptr
    dev = torch.device("cuda:0")
    n = a.n or c3_parameter_count()
    gen = torch.Generator().manual_seed(4)
    param, grad, m, ema = (torch.randn(n, generator=gen).to(dev) * s for s in (1.0, 1e-2, 1e-3, 1.0))
    v = (torch.rand(n, generator=gen) * 1e-6).to(dev)
    clip = torch.zeros(4, device=dev)
    st = L.current_stream()
    hyper = (1e-4, 0.9, 0.999, 1e-8)            # lr, betas, eps

    def adam_ex(wd, decoupled, use_clip, use_ema):
        return lambda: lib.seld_adam_flat_ex(p(param), p(grad), p(m), p(v), p(ema if use_ema else None), n, *hyper, wd,
                                             decoupled, 10, 1.0, p(clip if use_clip else None), 0.999, st)
    calls = {
        "adam": (7, lambda: lib.seld_adam_flat(p(param), p(grad), p(m), p(v), n, *hyper, 0.0, 10, 1.0, st)),
        "adam_ex_off": (7, adam_ex(0.0, 0, False, False)),
        "adam_ex_clip": (7, adam_ex(0.0, 0, True, False)),
        "adam_ex_decoupled": (7, adam_ex(1e-2, 1, False, False)),
        "adam_ex_ema": (9, adam_ex(0.0, 0, False, True)),
        "adam_ex_all": (9, adam_ex(1e-2, 1, True, True)),
        "grad_norm": (1, lambda: lib.seld_grad_norm(p(grad), n, 1.0, 1.0, p(clip), st)),
    }
    for _ in range(3):
        for k, (_, call) in calls.items():
            L.check(call(), k)
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, (_, call) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.burst):
                L.check(call(), k)
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / a.burst)
    base = statistics.median(us["adam"])
    rows = {}
    for k, (words, _) in calls.items():
        med = statistics.median(us[k])
        rows[k] = dict(words=words, us=round(med, 2), us_min_max=[round(min(us[k]), 2), round(max(us[k]), 2)],
                       GBps=round(words * 4 * n / (med * 1e-6) / 1e9, 1), ratio=round(med / base, 3),
                       words_ratio=round(words / 7, 3))
    print(json.dumps(dict(tool="optim_bench", reps=a.reps, burst=a.burst, n=n, MB_per_buffer=round(4 * n / 1e6, 2), launches=rows)), flush=True)


if __name__ == "__main__":
    main()
