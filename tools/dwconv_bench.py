#!/usr/bin/env python3
"""Micro-benchmark of the depthwise convolution (csrc/dwconv.hip; HIP events, warm-up, same stream): forward, input
gradient and weight + bias gradient (partials + fold), with torch's own depthwise convolution (F.conv*d(groups=C) and
aten.convolution_backward on the device) as the comparison row.  Bytes are algorithmic: forward and input gradient read
x (or dy) once and write y (or dx) once, plus the weights; the weight gradient reads x and dy once.  Rates are given as
a share of 6.3 TB/s (measured float4 copy on the MI355X) and of 8 TB/s (spec).
   python tools/dwconv_bench.py [--iters 20] [--only d2_3x3_s1,d1_k7]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

H = seld_amd.hip_ops
COPY_TBS, SPEC_TBS = 6.3, 8.0
SHAPES = {
    "d2_3x3_s1": dict(x=(32, 64, 128, 512), k=(3, 3), stride=1, pad=1),
    "d2_3x3_s2": dict(x=(32, 64, 128, 512), k=(3, 3), stride=2, pad=1),
    "d2_5x5_s1": dict(x=(32, 64, 128, 512), k=(5, 5), stride=1, pad=2),
    "d2_1x3": dict(x=(32, 192, 8, 512), k=(1, 3), stride=1, pad=(0, 1)),
    "d1_k3": dict(x=(32, 192, 512), k=(3,), stride=1, pad=1),
    "d1_k7": dict(x=(8, 256, 4800), k=(7,), stride=1, pad=3),
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


def row(name, op, us, nbytes):
    tbs = nbytes / (us * 1e-6) / 1e12
    return dict(shape=name, op=op, us=round(us, 1), MB=round(nbytes / 1e6, 1), TBs=round(tbs, 2),
                of_copy=round(tbs / COPY_TBS, 3), of_spec=round(tbs / SPEC_TBS, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rows = []
    for name, s in SHAPES.items():
        if args.only and name not in args.only.split(","):
            continue
        C = s["x"][1]
        x = torch.randn(s["x"], device=dev)
        w = torch.randn((C, 1) + s["k"], device=dev) * 0.3
        b = torch.randn(C, device=dev)
        desc = H.make_dwconv_desc(s["x"], C, s["k"], s["stride"], s["pad"], 1)
        y = H.dwconv_fwd(desc, x, w, b)
        dy = torch.randn_like(y)
        dw, db = torch.zeros_like(w), torch.zeros_like(b)
        bx, by, bw = 4.0 * x.numel(), 4.0 * y.numel(), 4.0 * w.numel()
        t = timed(lambda: H.dwconv_fwd(desc, x, w, b), args.iters)
        rows.append(dict(row(name, "forward", t, bx + by + bw), kernel=H.dwconv_label(desc, 0)))
        t = timed(lambda: H.dwconv_bwd_data(desc, dy, w, tuple(x.shape)), args.iters)
        rows.append(dict(row(name, "input_grad", t, bx + by + bw), kernel=H.dwconv_label(desc, 1)))
        t = timed(lambda: H.dwconv_bwd_weight_acc(desc, x, dy, dw, db), args.iters)
        rows.append(dict(row(name, "weight_grad", t, bx + by + bw), kernel=H.dwconv_label(desc, 2) + " + fold"))
        conv = F.conv2d if x.dim() == 4 else F.conv1d
        nd = x.dim() - 2
        st = [s["stride"]] * nd if isinstance(s["stride"], int) else list(s["stride"])
        pd = [s["pad"]] * nd if isinstance(s["pad"], int) else list(s["pad"])
        t = timed(lambda: conv(x, w, b, s["stride"], s["pad"], 1, C), args.iters)
        rows.append(dict(row(name, "torch_forward", t, bx + by + bw), kernel="F.conv%dd(groups=C)" % nd))
        cb = torch.ops.aten.convolution_backward
        t = timed(lambda: cb(dy, x, w, [C], st, pd, [1] * nd, False, [0] * nd, C, [True, False, False]), args.iters)
        rows.append(dict(row(name, "torch_input_grad", t, bx + by + bw), kernel="aten.convolution_backward"))
        t = timed(lambda: cb(dy, x, w, [C], st, pd, [1] * nd, False, [0] * nd, C, [False, True, True]), args.iters)
        rows.append(dict(row(name, "torch_weight_grad", t, bx + by + bw), kernel="aten.convolution_backward"))
        del x, y, dy
        torch.cuda.empty_cache()
    print(f"{'shape':10s} {'op':18s} {'us':>9s} {'MB':>8s} {'TB/s':>6s} {'/6.3':>6s} {'/8.0':>6s}  kernel")
    for r in rows:
        print(f"{r['shape']:10s} {r['op']:18s} {r['us']:9.1f} {r['MB']:8.1f} {r['TBs']:6.2f} {r['of_copy']:6.3f} "
              f"{r['of_spec']:6.3f}  {r['kernel']}")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
