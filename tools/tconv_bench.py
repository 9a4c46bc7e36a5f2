#!/usr/bin/env python3
"""Micro-benchmark of the quaternion transposed convolution (csrc/hc_conv_transpose.hip; HIP events, same stream).
Forward: the stride-phase kernel against the mirrored-descriptor data gradient (seld_hc_conv_bwd_data_ex, transposed
weights in a workspace) plus a bias add; backward: input gradient and accumulating weight + bias gradient.
Algorithmic flops 2*N*Hin*Win*Cin*Cout*kh*kw (all 16 Hamilton blocks, SURVEY 8d's currency).
   python tools/tconv_bench.py [--iters 20] [--only up2d,up1d]"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

H = seld_amd.hip_ops
L = seld_amd._lib
PEAK_TFLOPS = 157.3            # fp32 MFMA peak of the MI355X
SHAPES = {
    "up2d": dict(x=(16, 64, 32, 128), cout=64, k=(4, 4), stride=2, pad=1),
    "up2d_freq": dict(x=(32, 192, 8, 512), cout=192, k=(4, 3), stride=(2, 1), pad=(1, 1)),
    "up1d": dict(x=(32, 192, 256), cout=192, k=(4,), stride=2, pad=1),
    "same1d": dict(x=(32, 192, 512), cout=192, k=(3,), stride=1, pad=1),
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
    lib = L.lib()
    for name, s in SHAPES.items():
        if args.only and name not in args.only.split(","):
            continue
        cin, cout = s["x"][1], s["cout"]
        x = torch.randn(s["x"], device=dev)
        ws = [torch.randn((cin // 4, cout // 4) + s["k"], device=dev) * 0.1 for _ in range(4)]
        bias = torch.randn(cout, device=dev)
        desc, out_pad = H.conv_transpose_desc(s["x"], cout, 4, s["k"], s["stride"], s["pad"], 0, 1)
        y = H.conv_transpose_fwd(desc, out_pad, x, ws, bias)
        gy = torch.randn_like(y)
        gw = [torch.zeros_like(w) for w in ws]
        gb = torch.zeros_like(bias)
        flops = H.conv_transpose_work(desc, out_pad)[0]
        # baseline: the transposed convolution as the data gradient of the mirrored convolution, then the bias
        mdesc = H.make_conv_desc(tuple(y.shape), cin, 4, s["k"], s["stride"], s["pad"], 1)
        nbytes = int(lib.seld_hc_conv_bwd_data_workspace(ctypes.byref(mdesc)))
        wsb = torch.empty((nbytes + 3) // 4, device=dev)
        y_m = torch.empty_like(y)
        bview = bias.view((1, cout) + (1,) * (y.dim() - 2))
        stream = L.current_stream()
        wp = L.ptr_array8(ws)

        def mirrored():
            L.check(lib.seld_hc_conv_bwd_data_ex(ctypes.byref(mdesc), L.ptr(x), wp, L.ptr(y_m), L.ptr(wsb), nbytes,
                                                 stream), "seld_hc_conv_bwd_data_ex")
            y_m.add_(bview)
        fns = {"fwd": lambda: H.conv_transpose_fwd(desc, out_pad, x, ws, bias),
               "fwd_mirrored_dgrad+bias": mirrored,
               "bwd_data": lambda: H.conv_transpose_bwd_data(desc, out_pad, gy, ws, tuple(x.shape)),
               "bwd_weight+bias": lambda: H.conv_transpose_bwd_weight_acc(desc, out_pad, x, gy, gw, gb)}
        labels = {"fwd": H.conv_transpose_label(desc, out_pad, 0), "bwd_data": H.conv_transpose_label(desc, out_pad, 1),
                  "bwd_weight+bias": H.conv_transpose_label(desc, out_pad, 2),
                  "fwd_mirrored_dgrad+bias": H._label(mdesc, 1)}
        for which, f in fns.items():
            us = timed(f, args.iters)
            tf = flops / us / 1e6
            print(json.dumps(dict(shape=name, op=which, kernel=labels[which], us=round(us, 1), tflops=round(tf, 1),
                                  peak_share=round(tf / PEAK_TFLOPS, 3))), flush=True)


if __name__ == "__main__":
    main()
