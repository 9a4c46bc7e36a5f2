#!/usr/bin/env python3
"""Times the temporal-attention core (csrc/temporal_attention.hip) through the C ABI with HIP events:

  (a) seld_at_fwd and seld_at_bwd at (N, K, V, T) = (32, 16, 16, 512), (32, 16, 64, 512), (4, 16, 64, 4800), and the
      whole-clip K == V row (4, 16, 16, 4800), for the masks none, causal and band W = 64;
  (b) on the K == V rows the attention of csrc/mha*.hip (seld_mha_fwd_ex / seld_mha_bwd_ex, one head) on the same q, k, v
      with the same mask given as a (T, T) byte tensor.  The causal and band kernels of (a) do strictly less work than it,
      so `ok` is: the median of three measurements of the new kernel is no longer than the median of three of the old one,
      the two alternating, forward and backward separately.  A measurement is the mean over --reps launches between two
      events, after a warm-up of both;
  (c) --step K: the training step of bench.py's default workload (c3, its batch and synthetic data, recorded and replayed
      as bench.py does by default) with the blocks off and with --at_key_size=16 --at_value_size=64, K replays each, the
      two alternating twice.

Prints ONE JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((32, 16, 16, 512), (32, 16, 64, 512), (4, 16, 64, 4800), (4, 16, 16, 4800))        # (N, K, V, T)
MASKS = (("none", 0), ("causal", 0), ("band", 64))
AT_ON = dict(at_key_size=16, at_value_size=64)


def _mean_us(call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _keep(mask, W, T, dev):
    if mask == "none":
        return None
    t = torch.arange(T, device=dev)
    d = t.view(T, 1) - t.view(1, T)
    return ((d >= 0) if mask == "causal" else (d.abs() <= W)).to(torch.uint8).contiguous()


def core_rows(reps):
    import seld_amd
    H, L = seld_amd.hip_ops, seld_amd._lib
    lib, p = L.lib(), L.ptr
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(4)
    rows = []
    for N, K, V, T in SHAPES:
        qkv = torch.randn(N, 2 * K + V, T, generator=g).to(dev)
        dread = torch.randn(N, V, T, generator=g).to(dev)
        read, lse, dqkv = torch.empty_like(dread), torch.empty(N, T, device=dev), torch.empty_like(qkv)
        nb = lib.seld_at_bwd_workspace(N, T)
        ws = torch.empty(nb // 4, device=dev)
        st = L.current_stream()
        if K == V:
            q, k, v = (qkv[:, i * K:(i + 1) * K].contiguous() for i in range(3))
            out, lse2 = torch.empty_like(q), torch.empty(N, 1, T, device=dev)
            dq, dk, dv = (torch.empty_like(q) for _ in range(3))
        for mask, W in MASKS:
            kind = H.AT_MASKS[mask]
            calls = {
                "at_fwd": lambda: L.check(lib.seld_at_fwd(p(qkv), N, T, K, V, kind, W, None, p(read), p(lse), st), "seld_at_fwd"),
                "at_bwd": lambda: L.check(lib.seld_at_bwd(p(qkv), p(read), p(dread), p(lse), N, T, K, V, kind, W, None, p(dqkv),
                                                          p(ws), nb, st), "seld_at_bwd"),
            }
            if K == V:
                keep = _keep(mask, W, T, dev)
                strides = None if keep is None else (ctypes.c_int64 * 4)(0, 0, T, 1)
                calls["mha_fwd"] = lambda: L.check(lib.seld_mha_fwd_ex(p(q), p(k), p(v), N, T, T, 1, K, p(keep), strides, p(out),
                                                                       p(lse2), st), "seld_mha_fwd_ex")
                calls["mha_bwd"] = lambda: L.check(lib.seld_mha_bwd_ex(p(q), p(k), p(v), p(out), p(dread), p(lse2), N, T, T, 1, K,
                                                                       p(keep), strides, p(dq), p(dk), p(dv), p(ws), nb, st),
                                                   "seld_mha_bwd_ex")
            for _ in range(3):
                for c in calls.values():
                    c()
            torch.cuda.synchronize()
            us = {name: [] for name in calls}
            for _ in range(3):
                for name, c in calls.items():
                    us[name].append(_mean_us(c, reps))
            row = dict(N=N, K=K, V=V, T=T, mask=mask, band=W,
                       forms=[H.at_kernel_label(op, T, K, V) for op in ("fwd", "bwd_dq", "bwd_dkv")])
            for name, vals in us.items():
                row[name] = dict(us=round(statistics.median(vals), 1), us_all=[round(x, 1) for x in vals])
            if K == V:
                for leg in ("fwd", "bwd"):
                    row[f"at_{leg}"]["baseline"] = f"mha_{leg}"
                    if mask != "none":
                        row[f"at_{leg}"]["ok"] = bool(row[f"at_{leg}"]["us"] <= row[f"mha_{leg}"]["us"])
            rows.append(row)
    return rows


def train_step_ms(steps):
    """Median milliseconds of a replayed c3 training step with the blocks off and on (four measurements, alternating)."""
    import numpy as np
    import bench
    import seld_amd
    T, DP = seld_amd.train, seld_amd.dp
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["c3"]
    out = {False: [], True: []}
    for on in (False, True, False, True):
        np.random.seed(1)
        torch.manual_seed(1)
        model = seld_amd.model.SELD_Model(**bench.model_kwargs(w, 128), **(AT_ON if on else {})).to(dev).train()
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
        out[on].append(round(e0.elapsed_time(e1) / steps, 3))
        del runner, model, opt, sync
        torch.cuda.empty_cache()
    return dict(batch=w["batch"], steps=steps, mode="graph", at=AT_ON, at_off_ms=out[False], at_on_ms=out[True])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", type=int, default=0, metavar="K", help="also time K replayed training steps with AT off and on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("at_bench.py needs a HIP device")
    if a.reps < 5:
        raise SystemExit("at least 5 repetitions")
    rows = core_rows(a.reps)
    checked = [r[leg]["ok"] for r in rows for leg in ("at_fwd", "at_bwd") if "ok" in r[leg]]
    line = dict(tool="at_bench", reps=a.reps, all_ok=all(checked), rows=rows)
    if a.step:
        torch.cuda.empty_cache()
        line["train_step"] = train_step_ms(a.step)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
