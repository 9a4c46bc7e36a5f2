#!/usr/bin/env python3
"""Generate tests/golden/conv_geometry.npz by IMPORTING THE REFERENCE's quaternion and dual-quaternion convolutions.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_conv_geometry.py

Per case of FIXTURE_CASES (tests/golden/conv_geometry_cases.py): the reference's y, dx, dw0..dw{A-1} and dbias for the
closed-form inputs and cotangent; the real cases (algebra 1) are F.conv1d / F.conv2d, which is what the reference's real
model calls.  Computed in float64, stored as float32.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["SELD_REFERENCE"])

from dual_quaternion import dual_quaternion_ops as RDQ           # noqa: E402  (reference)
from quaternion import quaternion_ops as RQ                      # noqa: E402  (reference)

from tests.golden.conv_geometry_cases import FIXTURE_CASES, fixture_cotangent, fixture_inputs   # noqa: E402

META = dict(torch=torch.__version__, numpy=np.__version__,
            reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11")
DT = torch.float64


def reference_op(case, x, ws, bias):
    if case["algebra"] == 8:
        return RDQ.dual_quaternion_conv(x, *ws, bias, case["stride"], case["padding"], 1, case["dilation"])
    if case["algebra"] == 4:
        return RQ.quaternion_conv(x, *ws, bias, case["stride"], case["padding"], 1, case["dilation"])
    fn = F.conv1d if x.dim() == 3 else F.conv2d
    return fn(x, ws[0], bias, case["stride"], case["padding"], case["dilation"], 1)


def main():
    res = {}
    for case in FIXTURE_CASES:
        name = case["name"]
        x, ws, bias = fixture_inputs(case, DT)
        for t in [x] + ws + ([bias] if bias is not None else []):
            t.requires_grad_(True)
        y = reference_op(case, x, ws, bias)
        (y * fixture_cotangent(y.shape, DT)).sum().backward()
        res[name + ".y"] = y.detach().numpy()
        res[name + ".dx"] = x.grad.numpy()
        for i, w in enumerate(ws):
            res[f"{name}.dw{i}"] = w.grad.numpy()
        if bias is not None:
            res[name + ".dbias"] = bias.grad.numpy()
    out = {k: np.asarray(v, dtype=np.float32) for k, v in res.items()}
    out["meta"] = json.dumps(META)
    path = os.path.join(HERE, "conv_geometry.npz")
    np.savez_compressed(path, **out)
    print("wrote conv_geometry", len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
