#!/usr/bin/env python3
"""Times the squeeze-and-excitation kernels (csrc/squeeze_excite.hip) on the activations of the benchmark's default
workload (bench.py c3: DQ, batch 32, 192 CNN filters, G = 384, 128 mel x 512 frames, --se_reduction 4): the three CNN stage
outputs and the residual blocks' gated y.  Each streaming kernel is timed against a kernel of csrc/norm.hip with the same
traffic on the same tensor:

  se_scale, se_bwd_apply   bn_act_fwd          read 1, write 1
  se_squeeze               channel_stats       read 1
  se_bwd_reduce            bn_act_bwd_reduce   read 2 (the baseline reads a third tensor, y)

HIP events around single launches through the C ABI, the baseline and the SE kernel alternating inside every repetition,
after a warm-up of both.  `ok` is: the SE kernel's median is no slower than the baseline's slowest repetition.  The excite
kernels (one workgroup per sample) are given in microseconds only.

--step: also the training step of that workload (bench.py's model, batch and synthetic data, recorded and replayed as bench.py
does by default) with --se_reduction 0 and 4, --step replays each, the two alternating twice.  Prints ONE JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# (name, (N, C, *spatial)): bench.py's c3 at its batch; components 8, reduction 4
SHAPES = (("cnn.0", (32, 192, 16, 512)), ("cnn.1", (32, 192, 2, 512)), ("cnn.2", (32, 192, 1, 512)),
          ("resblock.y", (32, 384, 512)))
A, REDUCTION = 8, 4


def train_step_ms(steps):
    """Median milliseconds of a replayed c3 training step with se_reduction 0 and 4 (four measurements, alternating)."""
    import numpy as np
    import bench
    import seld_amd
    T, DP = seld_amd.train, seld_amd.dp
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["c3"]
    out = {0: [], 4: []}
    for reduction in (0, 4, 0, 4):
        np.random.seed(1)
        torch.manual_seed(1)
        model = seld_amd.model.SELD_Model(**bench.model_kwargs(w, 128), se_reduction=reduction).to(dev).train()
        opt = T.FlatAdam(model.parameters(), lr=1e-4)
        sync = DP.BucketedGradSync(opt, model)
        x, target = T.synthetic_batch(w["batch"], w["input_channels"], 128, 512, 42, 1234, dev)
        for _ in range(2):
            DP.dp_train_step(model, opt, sync, x, target, 42, T.seld_loss_fn)
        runner = T.GraphedTrainStep(model, opt, x, target, 42, 1.0, 5.0, sync=sync, warmup=1)
        for _ in range(3):
            runner()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            runner()
        e1.record()
        torch.cuda.synchronize()
        out[reduction].append(round(e0.elapsed_time(e1) / steps, 3))
        del runner, model, opt, sync
        torch.cuda.empty_cache()
    return dict(batch=w["batch"], steps=steps, mode="graph", se_reduction_0_ms=out[0], se_reduction_4_ms=out[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", type=int, default=0, metavar="K", help="also time K replayed training steps with SE off and on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("se_bench.py needs a HIP device")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    import seld_amd
    H, L = seld_amd.hip_ops, seld_amd._lib
    lib, p = L.lib(), L.ptr
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(4)
    results = []
    for name, shape in SHAPES:
        N, C = shape[:2]
        S = 1
        for d in shape[2:]:
            S *= d
        Cg = C // A
        Hd = max(1, Cg // REDUCTION)
        x = torch.randn(shape, generator=g).to(dev)
        dy = torch.randn(shape, generator=g).to(dev)
        out = torch.empty_like(x)
        w1, b1 = torch.randn(Hd, Cg, generator=g).to(dev) / Cg ** 0.5, torch.zeros(Hd, device=dev)
        w2, b2 = torch.randn(Cg, Hd, generator=g).to(dev) / Hd ** 0.5, torch.zeros(Cg, device=dev)
        rowsum, q = (torch.empty(N * C, device=dev) for _ in range(2))
        z, s, dp2, dz = (torch.empty(N * Cg, device=dev) for _ in range(4))
        h, dh = (torch.empty(N * Hd, device=dev) for _ in range(2))
        grads = [torch.empty_like(t) for t in (w1, b1, w2, b2)]
        mean, beta = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        invstd, gamma = torch.ones(C, device=dev), torch.full((C,), 0.5, device=dev)
        stats = H.new_stats(C, dev)
        red = torch.zeros(2 * C, device=dev)
        st = L.current_stream()
        calls = {
            "se_squeeze": lambda: lib.seld_se_squeeze(p(x), N * C, S, p(rowsum), st),
            "channel_stats": lambda: lib.seld_channel_stats(p(x), N, C, S, p(stats), st),
            "se_scale": lambda: lib.seld_se_scale(p(x), N, C, S, A, p(s), p(out), st),
            "se_bwd_apply": lambda: lib.seld_se_bwd_apply(p(dy), N, C, S, A, p(s), p(dz), p(out), st),
            "bn_act_fwd": lambda: lib.seld_bn_act_fwd(p(x), N, C, S, p(mean), p(invstd), p(gamma), p(beta), L.SELD_ACT_NONE,
                                                      p(out), st),
            "se_bwd_reduce": lambda: lib.seld_se_bwd_reduce(p(dy), p(x), N * C, S, p(q), st),
            "bn_act_bwd_reduce": lambda: lib.seld_bn_act_bwd_reduce(p(dy), p(x), p(out), N, C, S, p(mean), p(invstd), p(gamma),
                                                                    p(beta), L.SELD_ACT_NONE, p(red), st),
            "se_excite_fwd": lambda: lib.seld_se_excite_fwd(p(rowsum), N, C, S, A, Hd, p(w1), p(b1), p(w2), p(b2), p(z), p(h),
                                                            p(s), st),
            "se_excite_bwd": lambda: lib.seld_se_excite_bwd(p(q), N, C, A, Hd, p(w1), p(w2), p(z), p(h), p(s), p(dp2), p(dh),
                                                            p(dz), *(p(t) for t in grads), 0, st),
        }
        order = ("se_squeeze", "se_excite_fwd", "se_scale", "se_bwd_reduce", "se_excite_bwd", "se_bwd_apply", "channel_stats",
                 "bn_act_fwd", "bn_act_bwd_reduce")
        for _ in range(3):
            for k in order:
                L.check(calls[k](), k)
        torch.cuda.synchronize()
        us = {k: [] for k in order}
        for _ in range(a.reps):
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.check(calls[k](), k)
                e1.record()
                torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3)
        nbytes = 4 * N * C * S
        traffic = dict(se_squeeze=1, channel_stats=1, se_scale=2, se_bwd_apply=2, bn_act_fwd=2, se_bwd_reduce=2,
                       bn_act_bwd_reduce=3)
        row = dict(tensor=name, shape=shape, gated=Cg, hidden=Hd, MB=round(nbytes / 1e6, 1),
                   forms={op: H.se_kernel_label(op, S) for op in ("squeeze", "scale", "bwd_reduce", "bwd_apply")})
        for k in order:
            med = statistics.median(us[k])
            row[k] = dict(us=round(med, 1), us_min_max=[round(min(us[k]), 1), round(max(us[k]), 1)])
            if k in traffic:
                row[k]["GBps"] = round(traffic[k] * nbytes / (med * 1e-6) / 1e9, 1)
        for se, base in (("se_squeeze", "channel_stats"), ("se_scale", "bn_act_fwd"), ("se_bwd_apply", "bn_act_fwd"),
                         ("se_bwd_reduce", "bn_act_bwd_reduce")):
            row[se]["baseline"] = base
            row[se]["ok"] = bool(statistics.median(us[se]) <= max(us[base]))
        results.append(row)
    ok = all(row[k]["ok"] for row in results for k in ("se_squeeze", "se_scale", "se_bwd_apply", "se_bwd_reduce"))
    line = dict(tool="se_bench", reps=a.reps, components=A, reduction=REDUCTION, all_ok=ok, tensors=results)
    if a.step:
        del x, dy, out
        torch.cuda.empty_cache()
        line["train_step"] = train_step_ms(a.step)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
