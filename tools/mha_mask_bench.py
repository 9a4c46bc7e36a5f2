#!/usr/bin/env python3
"""Masked attention core (seld_mha_fwd_ex / _bwd_ex) against the unmasked cores, us per call.

Config-3 shape (N = 32, 8 heads x 48, T = 256): the packed and the unpacked unmasked cores, a (N, 1, 1, T) key-padding
mask and a (T, T) causal mask, forward and forward + backward; and B = 1, T = 2400 with a key-padding mask.  Random
data; all variants run in interleaved rounds in this one process, the median and min over rounds are reported.

    python tools/mha_mask_bench.py [--rounds 15] [--iters 20] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

H = seld_amd.hip_ops
dev = torch.device("cuda:0")


def variants():
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for tag, N, heads, hd, T in (("c3", 32, 8, 48, 256), ("clip", 1, 8, 48, 2400)):
        E = heads * hd
        q, k, v = ((torch.randn(N, E, T, device=dev, generator=g) * 0.5).requires_grad_(True) for _ in range(3))
        qkv = (torch.randn(N, 3 * E, T, device=dev, generator=g) * 0.5).requires_grad_(True)
        cot = torch.randn(N, E, T, device=dev, generator=g)
        kpad = torch.ones(N, 1, 1, T, dtype=torch.bool, device=dev)
        kpad[N // 2:, ..., T - T // 5:] = False
        causal = torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev))
        cores = {"packed": (lambda qkv=qkv, heads=heads: H.mha_core_packed(qkv, heads), (qkv,)),
                 "unpacked": (lambda q=q, k=k, v=v, heads=heads: H.mha_core(q, k, v, heads), (q, k, v)),
                 "key_padding": (lambda q=q, k=k, v=v, heads=heads, m=kpad: H.mha_core_ex(q, k, v, heads, m), (q, k, v)),
                 "causal": (lambda q=q, k=k, v=v, heads=heads, m=causal: H.mha_core_ex(q, k, v, heads, m), (q, k, v))}
        if tag == "clip":
            cores = {"key_padding": cores["key_padding"]}
        for name, (f, ins) in cores.items():
            def fwd(f=f):
                with torch.no_grad():
                    f()

            def fb(f=f, ins=ins, cot=cot):
                torch.autograd.grad(f(), ins, cot)
            out[f"{tag}.{name}.fwd"] = fwd
            out[f"{tag}.{name}.fwd_bwd"] = fb
    return out


def time_us(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    vs = variants()
    for f in vs.values():            # warm-up: library load, allocator
        f()
        f()
    torch.cuda.synchronize()
    samples = {k: [] for k in vs}
    for _ in range(a.rounds):
        for k, f in vs.items():
            samples[k].append(time_us(f, a.iters))
    res = {k: dict(median_us=round(statistics.median(s), 1), min_us=round(min(s), 1)) for k, s in samples.items()}
    for k, r in res.items():
        print(f"{k:28s} median {r['median_us']:8.1f} us   min {r['min_us']:8.1f} us")
    for kind in ("fwd", "fwd_bwd"):
        base = res[f"c3.unpacked.{kind}"]["median_us"]
        for m in ("key_padding", "causal"):
            print(f"c3 {kind}: {m} / unpacked = {res[f'c3.{m}.{kind}']['median_us'] / base:.3f}")
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, results=res))
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
