#!/usr/bin/env python3
"""Micro-benchmark of the quaternion rotation path (csrc/quat_rotation.hip; HIP events, same stream): the form kernel
and its gradient alone, in both layouts, and a rotation layer's forward / forward + backward against the Hamilton-product
layer with the same component weights (QuaternionConv, QuaternionLinearAutograd with rotation=False).
   python tools/rotation_bench.py [--iters 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

H = seld_amd.hip_ops
L = seld_amd._lib
Ql = seld_amd.quaternion.quaternion_layers
# component shape (A, B, *taps) and the batch / length of the layer runs
CONV = dict(w=(48, 48, 3), N=32, T=512)
LINEAR = dict(w=(96, 96), rows=4096)


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


def report(name, us, nbytes=None):
    r = dict(name=name, us=round(us, 2))
    if nbytes is not None:
        r["GB_s"] = round(nbytes / us / 1e3, 1)
    print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for layout, shape in ((L.SELD_ROT_LAYOUT_CONV, CONV["w"]), (L.SELD_ROT_LAYOUT_LINEAR, LINEAR["w"])):
        ws = [torch.randn(shape, device=dev) * 0.3 for _ in range(4)]
        for qformat in (False, True):
            K = H.rotation_form(layout, qformat, ws)
            dK = torch.randn_like(K)
            dws = [torch.empty_like(w) for w in ws]
            tag = f"layout{layout}_{'x'.join(map(str, shape))}_q{int(qformat)}"
            wbytes = 4 * 4 * ws[0].numel()
            report("form_" + tag, timed(lambda: H.rotation_form(layout, qformat, ws), args.iters),
                   wbytes + 4 * K.numel())
            report("form_bwd_" + tag, timed(lambda: H.rotation_form_bwd(layout, qformat, ws, dK, dws, False), args.iters),
                   2 * wbytes + 4 * K.numel())

    O, I, k = CONV["w"]
    layers = {
        "conv_rotation": (Ql.QuaternionConv(4 * I, 4 * O, k, 1, padding=1, bias=False, seed=1, operation="convolution1d",
                                            rotation=True), (CONV["N"], 3 * I, CONV["T"])),
        "conv_rotation_qformat": (Ql.QuaternionConv(4 * I, 4 * O, k, 1, padding=1, bias=False, seed=1,
                                                    operation="convolution1d", rotation=True, quaternion_format=True),
                                  (CONV["N"], 4 * I, CONV["T"])),
        "conv_hamilton": (Ql.QuaternionConv(4 * I, 4 * O, k, 1, padding=1, bias=False, seed=1,
                                            operation="convolution1d"), (CONV["N"], 4 * I, CONV["T"])),
    }
    I, O = LINEAR["w"]
    layers.update({
        "linear_rotation": (Ql.QuaternionLinearAutograd(4 * I, 4 * O, bias=False, seed=1, rotation=True),
                            (LINEAR["rows"], 3 * I)),
        "linear_hamilton": (Ql.QuaternionLinearAutograd(4 * I, 4 * O, bias=False, seed=1), (LINEAR["rows"], 4 * I)),
    })
    for name, (m, xs) in layers.items():
        m = m.to(dev)
        x = torch.randn(xs, device=dev, requires_grad=True)
        with torch.no_grad():
            report(name + "_fwd", timed(lambda: m(x), args.iters))
        gy = torch.randn_like(m(x))

        def fb():
            m(x).backward(gy)
        report(name + "_fwd_bwd", timed(fb, args.iters))


if __name__ == "__main__":
    main()
