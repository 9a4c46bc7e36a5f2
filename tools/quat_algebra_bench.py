#!/usr/bin/env python3
"""Micro-benchmark of the element-wise quaternion algebra (csrc/quat_algebra.hip; HIP events, warm-up, same stream):
every op, forward and backward, through hip_ops, beside the same formula written as plain torch ops on the device (the
composition the reference runs: component slices, products, torch.cat).  Bytes are algorithmic: every operand is read
or written once (forward product 3 tensors, its backward 5; vector modulus 1.25 forward, 2.25 backward; the forms
summed over dim 0 read the tensor once and write a result of 1/(4 dim0) of it).  Rates are given as a share of
6.3 TB/s (measured float4 copy on the MI355X).  Each row is measured --repeats times (default 2: the shared machines
move up to 25 % from run to run); both figures are printed.
   python tools/quat_algebra_bench.py [--iters 20] [--repeats 2] [--only s192x8x512]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

H = seld_amd.hip_ops
COPY_TBS = 6.3
SHAPES = {"s192x8x512": (32, 192, 8, 512), "s64x128x512": (32, 64, 128, 512), "s16384x768": (16384, 768)}


def comps(x):
    axis = x.dim() - 1 if x.dim() < 4 else 1
    return torch.chunk(x, 4, dim=axis)


# ---- the same formulas as plain torch ops -------------------------------------------------------------------------
def t_modulus(x, vector_form):
    r, i, j, k = comps(x)
    s = r * r + i * i + j * j + k * k
    return torch.sqrt(s) if vector_form else torch.sqrt(s.sum(dim=0))


def t_normalized(x, eps=1e-4):
    m = t_modulus(x, False)
    return x / (torch.cat([m] * 4, dim=-1 if x.dim() < 4 else 0).unsqueeze(0) + eps)


def t_unit(x):
    r, i, j, k = comps(x)
    n = torch.sqrt(r * r + i * i + j * j + k * k + 1e-4)
    return torch.cat([r / n, i / n, j / n, k / n], dim=1)


def t_exp(x):
    r, i, j, k = comps(x)
    n = torch.sqrt(i * i + j * j + k * k) + 1e-4
    e, s = torch.exp(r), torch.sin(n)
    return torch.cat([e * torch.cos(n), e * (i / n) * s, e * (j / n) * s, e * (k / n) * s], dim=1)


def t_hamilton(a, b):
    r0, i0, j0, k0 = comps(a)
    r1, i1, j1, k1 = comps(b)
    return torch.cat([r0 * r1 - i0 * i1 - j0 * j1 - k0 * k1, r0 * i1 + i0 * r1 + j0 * k1 - k0 * j1,
                      r0 * j1 - i0 * k1 + j0 * r1 + k0 * i1, r0 * k1 + i0 * j1 - j0 * i1 + k0 * r1], dim=1)


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
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quat_algebra_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rows = []
    for name, shape in SHAPES.items():
        if args.only and name not in args.only.split(","):
            continue
        x = torch.randn(shape, device=dev).requires_grad_(True)
        q1 = torch.randn(shape, device=dev).requires_grad_(True)
        T = 4.0 * x.numel()                       # bytes of one full tensor
        small = T / (4 * shape[0])                # bytes of a result summed over dim 0
        # op, hip function, torch function, inputs, forward bytes, backward bytes
        ops = [("modulus_vec", lambda a: H.quat_modulus(a, True), lambda a: t_modulus(a, True), (x,), 1.25 * T, 2.25 * T),
               ("modulus_sum", lambda a: H.quat_modulus(a, False), lambda a: t_modulus(a, False), (x,), T + small,
                2 * T + 2 * small),
               ("q_normalize", H.quat_unit, t_unit, (x,), 2 * T, 3 * T),
               ("quaternion_exp", H.quat_exp, t_exp, (x,), 2 * T, 3 * T),
               ("hamilton", H.hamilton_product, t_hamilton, (x, q1), 3 * T, 5 * T)]
        # get_normalized: the public functions take rank 2 and 3 only, hip_ops.quat_normalized any rank
        ops.insert(2, ("normalized", H.quat_normalized, t_normalized, (x,), 3 * T + 2 * small, 5 * T + 3 * small))
        for op, hip, ref, ins, fb, bb in ops:
            for impl, fn in (("hip", hip), ("torch", ref)):
                y = fn(*ins)
                cot = torch.randn_like(y)
                fwd, bwd = [], []
                for _ in range(args.repeats):
                    with torch.no_grad():
                        fwd.append(timed(lambda: fn(*ins), args.iters))
                    bwd.append(timed(lambda: torch.autograd.grad(y, ins, cot, retain_graph=True), args.iters))
                for which, us, nbytes in (("forward", fwd, fb), ("backward", bwd, bb)):
                    tbs = nbytes / (min(us) * 1e-6) / 1e12
                    rows.append(dict(shape=name, op=op, impl=impl, dir=which, us=[round(u, 1) for u in us],
                                     MB=round(nbytes / 1e6, 1), TBs=round(tbs, 2), of_copy=round(tbs / COPY_TBS, 3)))
                del y, cot
            torch.cuda.empty_cache()
        del x, q1
        torch.cuda.empty_cache()
    print(f"{'shape':12s} {'op':15s} {'dir':9s} {'impl':6s} {'us (each repeat)':>22s} {'MB':>8s} {'TB/s':>6s} {'/6.3':>6s}")
    for r in rows:
        us = " ".join(f"{u:9.1f}" for u in r["us"])
        print(f"{r['shape']:12s} {r['op']:15s} {r['dir']:9s} {r['impl']:6s} {us:>22s} {r['MB']:8.1f} {r['TBs']:6.2f} "
              f"{r['of_copy']:6.3f}")
    slower = [(a["shape"], a["op"], a["dir"]) for a in rows if a["impl"] == "hip" for b in rows
              if b["impl"] == "torch" and (a["shape"], a["op"], a["dir"]) == (b["shape"], b["op"], b["dir"])
              and min(a["us"]) > min(b["us"])]
    print("hip slower than the torch composition:", slower or "none")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
