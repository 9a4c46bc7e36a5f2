#!/usr/bin/env python3
"""Micro-benchmark of the 3-D convolutions (csrc/hc_conv3d.hip; HIP events, same stream): forward, input gradient and
accumulating weight + bias gradient at a few user-sized shapes, with F.conv3d / F.conv_transpose3d (and their
gradients) on the assembled real weight on the same device for context.  Algorithmic flops 2*N*Cout*Cin*kd*kh*kw per
output position of the convolution (per input position of the transposed one), all Hamilton blocks.
   python tools/conv3d_bench.py [--iters 20] [--only q_s1,dq]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402
from oracle.seld_oracle import assemble_conv_weight  # noqa: E402

H = seld_amd.hip_ops
PEAK_TFLOPS = 157.3            # fp32 MFMA peak of the MI355X
SHAPES = {
    "q_s1": dict(x=(8, 64, 16, 32, 32), cout=64, A=4, k=3, stride=1, pad=1),
    "q_s2": dict(x=(8, 64, 16, 32, 32), cout=64, A=4, k=3, stride=2, pad=1),
    "dq": dict(x=(4, 96, 8, 32, 64), cout=96, A=8, k=3, stride=1, pad=1),
    "q_tconv": dict(x=(8, 64, 8, 16, 16), cout=64, A=4, k=4, stride=2, pad=1, tconv=True),
}


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
    torch.backends.cudnn.allow_tf32 = False
    for name, s in SHAPES.items():
        if args.only and name not in args.only.split(","):
            continue
        A, cin, cout, k = s["A"], s["x"][1], s["cout"], (s["k"],) * 3
        tconv = s.get("tconv", False)
        x = torch.randn(s["x"], device=dev)
        ws = [torch.randn(((cin // A, cout // A) if tconv else (cout // A, cin // A)) + k, device=dev) * 0.05
              for _ in range(A)]
        bias = torch.randn(cout, device=dev)
        if tconv:
            desc, op = H.conv3d_transpose_desc(s["x"], cout, A, k, s["stride"], s["pad"], 0, 1)
        else:
            desc, op = H.make_conv3d_desc(s["x"], cout, A, k, s["stride"], s["pad"], 1), None
        y = H.conv3d_fwd(desc, op, x, ws, bias)
        gy = torch.randn_like(y)
        gw = [torch.zeros_like(w) for w in ws]
        gb = torch.zeros_like(bias)
        flops = H.conv3d_work(desc, op)[0]
        M = assemble_conv_weight(ws)
        xr = x.clone().requires_grad_(True)
        Mr = M.clone().requires_grad_(True)
        br = bias.clone().requires_grad_(True)
        if tconv:
            def aten():
                return F.conv_transpose3d(x, M, bias, s["stride"], s["pad"])

            def aten_graph():
                return F.conv_transpose3d(xr, Mr, br, s["stride"], s["pad"])
        else:
            def aten():
                return F.conv3d(x, M, bias, s["stride"], s["pad"])

            def aten_graph():
                return F.conv3d(xr, Mr, br, s["stride"], s["pad"])
        yr = aten_graph()
        fns = {"fwd": (H.conv3d_label(desc, op, 0), lambda: H.conv3d_fwd(desc, op, x, ws, bias)),
               "bwd_data": (H.conv3d_label(desc, op, 1), lambda: H.conv3d_bwd_data(desc, op, gy, ws, tuple(x.shape))),
               "bwd_weight+bias": (H.conv3d_label(desc, op, 2),
                                   lambda: H.conv3d_bwd_weight_acc(desc, op, x, gy, gw, gb)),
               "aten_fwd": ("F.conv_transpose3d" if tconv else "F.conv3d", aten),
               "aten_bwd_data": ("aten", lambda: torch.autograd.grad(yr, xr, gy, retain_graph=True)),
               "aten_bwd_weight+bias": ("aten", lambda: torch.autograd.grad(yr, (Mr, br), gy, retain_graph=True))}
        for which, (label, f) in fns.items():
            us = timed(f, args.iters)
            tf = flops / us / 1e6
            print(json.dumps(dict(shape=name, op=which, kernel=label, us=round(us, 1), tflops=round(tf, 1),
                                  peak_share=round(tf / PEAK_TFLOPS, 3))), flush=True)


if __name__ == "__main__":
    main()
