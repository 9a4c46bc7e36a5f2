#!/usr/bin/env python3
"""Generate tests/golden/conv3d.npz by IMPORTING THE REFERENCE's 3-D convolutions.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_conv3d.py

Per case of CONV3D_CASES: the reference's y, dx, dw0..dw{A-1} and dbias for the closed-form inputs and cotangent.  Per
variant of ROT3D_CASES: y, dx, dr..dk, dbias.  Per seeded layer of LAYER3D_CASES: its state dict, y, dx and every
parameter's gradient.  Computed in float64, stored as float32.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["SELD_REFERENCE"])

from dual_quaternion import dual_quaternion_layers as RDL        # noqa: E402  (reference)
from dual_quaternion import dual_quaternion_ops as RDQ           # noqa: E402  (reference)
from quaternion import quaternion_layers as RL                   # noqa: E402  (reference)
from quaternion import quaternion_ops as RQ                      # noqa: E402  (reference)

from oracle.seld_oracle import closed_form_input                 # noqa: E402
from tests.golden.conv3d_cases import (CONV3D_CASES, LAYER3D_CASES, conv3d_cotangent, conv3d_inputs,  # noqa: E402
                                       rot3d_inputs, rot3d_variants)

META = dict(torch=torch.__version__, numpy=np.__version__,
            reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11")
DT = torch.float64


def reference_op(case, x, ws, bias):
    if case["kind"] == "tconv":
        return RQ.quaternion_transpose_conv(x, *ws, bias, case["stride"], case["padding"], case["output_padding"], 1,
                                            case["dilation"])
    if case["algebra"] == 8:
        return RDQ.dual_quaternion_conv(x, *ws, bias, case["stride"], case["padding"], 1, case["dilation"])
    return RQ.quaternion_conv(x, *ws, bias, case["stride"], case["padding"], 1, case["dilation"])


def reference_rot(case, x, ws, bias, qformat):
    if case["kind"] == "conv":
        return RQ.quaternion_conv_rotation(x, *ws, bias, case["stride"], case["padding"], 1, case["dilation"], qformat)
    return RQ.quaternion_transpose_conv_rotation(x, *ws, bias, case["stride"], case["padding"], case["output_padding"],
                                                 1, case["dilation"], qformat)


def _grads(res, name, y, x, named):
    (y * conv3d_cotangent(y.shape, DT)).sum().backward()
    res[name + ".y"] = y.detach().numpy()
    res[name + ".dx"] = x.grad.numpy()
    for key, t in named:
        res[f"{name}.{key}"] = t.grad.numpy()


def main():
    # the reference's quaternion_format branch pads with torch.zeros(shape): the default dtype must be the weights'
    torch.set_default_dtype(DT)
    res = {}
    for case in CONV3D_CASES:
        x, ws, bias = conv3d_inputs(case, DT)
        leaves = [x] + ws + ([bias] if bias is not None else [])
        for t in leaves:
            t.requires_grad_(True)
        named = [(f"dw{i}", w) for i, w in enumerate(ws)] + ([("dbias", bias)] if bias is not None else [])
        _grads(res, case["name"], reference_op(case, x, ws, bias), x, named)
    for case, name, qformat in rot3d_variants():
        x, ws, bias = rot3d_inputs(case, qformat, DT)
        for t in [x] + ws + [bias]:
            t.requires_grad_(True)
        named = [(f"d{c}", w) for c, w in zip("rijk", ws)] + [("dbias", bias)]
        _grads(res, name, reference_rot(case, x, ws, bias, qformat), x, named)
    keys = {}
    for c in LAYER3D_CASES:
        np.random.seed(c["np_seed"])
        mod = RDL if c["cls"].startswith("Dual") else RL
        layer = getattr(mod, c["cls"])(**c["kwargs"])
        name = c["name"]
        keys[name] = list(layer.state_dict().keys())
        for k, v in layer.state_dict().items():
            res[f"{name}.{k}"] = v.numpy()
        x = closed_form_input(c["x"], DT).requires_grad_(True)
        named = [(f"grad.{k}", p) for k, p in layer.named_parameters() if p.requires_grad]
        _grads(res, name, layer(x), x, named)
    out = {k: np.asarray(v, dtype=np.float32) for k, v in res.items()}
    out["meta"] = json.dumps(META)
    out["layer_keys"] = json.dumps(keys)
    np.savez_compressed(os.path.join(HERE, "conv3d.npz"), **out)
    print("wrote conv3d", len(out), "arrays", os.path.getsize(os.path.join(HERE, "conv3d.npz")), "bytes")


if __name__ == "__main__":
    main()
