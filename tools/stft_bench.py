#!/usr/bin/env python3
"""Micro-benchmark of spectrum_fast at segment lengths other than the reference's 512 (csrc/stft_any.hip; HIP events,
same stream): a 60 s x 8 channel clip at the sample rate each length is a frame-aligned window for, hop N / 2, phase
on, the reference's cuts.  Bytes = input + output (the least the call has to move), over the event time.
   python tools/stft_bench.py [--iters 20] [--only 480,997]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

UF = seld_amd.utility_functions
HBM_TBS = 8.0                  # HBM3E peak of the MI355X
# (nperseg, sample rate, path)
LENGTHS = [(480, 24000, "smooth"), (882, 44100, "smooth"), (960, 24000, "smooth"), (1000, 40000, "smooth"),
           (1764, 44100, "smooth"), (2048, 48000, "smooth"), (4096, 48000, "smooth"),
           (997, 32000, "bluestein"), (4095, 48000, "bluestein"), (512, 32000, "radix-8 (reference length)")]


def timed(f, iters):
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    for N, sr, path in LENGTHS:
        if args.only and str(N) not in args.only.split(","):
            continue
        x = torch.randn(8, 60 * sr, device=dev, generator=gen)
        hop = N // 2
        out = UF.spectrum_fast(x, N, N - hop)
        nbytes = (x.numel() + out.numel()) * 4
        us = timed(lambda: UF.spectrum_fast(x, N, N - hop), args.iters)
        print(json.dumps(dict(nperseg=N, sr=sr, hop=hop, path=path, out=list(out.shape), mbytes=round(nbytes / 1e6, 1),
                              us=round(us, 1), gbs=round(nbytes / us / 1e3, 1),
                              hbm_share=round(nbytes / us / 1e6 / HBM_TBS, 3))), flush=True)


if __name__ == "__main__":
    main()
