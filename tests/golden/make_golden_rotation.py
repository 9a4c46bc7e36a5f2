#!/usr/bin/env python3
"""Generate tests/golden/rotation.npz by IMPORTING THE REFERENCE's quaternion rotation ops and layers.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rotation.py

Per variant of ROT_CASES (both quaternion_format values, with and without bias): the reference's y, dx, dr..dk and dbias
for the closed-form inputs and cotangent, computed in float64 and stored as float32.  Plus one seeded layer of each of
QuaternionConv, QuaternionTransposeConv and QuaternionLinearAutograd with rotation=True: its state dict, and y and the
gradients for the closed-form input.
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

from quaternion import quaternion_ops as RQ                    # noqa: E402  (reference)
from quaternion import quaternion_layers as RL                 # noqa: E402  (reference)

from oracle.seld_oracle import closed_form_input               # noqa: E402
from tests.golden.rotation_cases import LAYER_CASES, all_variants, rotation_cotangent, rotation_inputs   # noqa: E402

META = dict(torch=torch.__version__, numpy=np.__version__,
            reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11")
DT = torch.float64


def reference_op(case, x, ws, bias, qformat):
    if case["kind"] == "conv":
        return RQ.quaternion_conv_rotation(x, *ws, bias, case["stride"], case["padding"], 1, case["dilation"], qformat)
    if case["kind"] == "tconv":
        return RQ.quaternion_transpose_conv_rotation(x, *ws, bias, case["stride"], case["padding"],
                                                     case["output_padding"], 1, case["dilation"], qformat)
    return RQ.quaternion_linear_rotation(x, *ws, bias, qformat)


def main():
    # the reference's quaternion_format branch pads with torch.zeros(shape): the default dtype must be the weights'
    torch.set_default_dtype(DT)
    res = {}
    for case, name, qformat, has_bias in all_variants():
        x, ws, bias = rotation_inputs(case, qformat, has_bias, DT)
        leaves = [x] + ws + ([bias] if bias is not None else [])
        for t in leaves:
            t.requires_grad_(True)
        y = reference_op(case, x, ws, bias, qformat)
        (y * rotation_cotangent(y.shape, DT)).sum().backward()
        res[name + ".y"] = y.detach().numpy()
        res[name + ".dx"] = x.grad.numpy()
        for c, w in zip("rijk", ws):
            res[f"{name}.d{c}"] = w.grad.numpy()
        if bias is not None:
            res[name + ".dbias"] = bias.grad.numpy()
    keys = {}
    for c in LAYER_CASES:
        np.random.seed(c["np_seed"])
        layer = getattr(RL, c["cls"])(**c["kwargs"])
        name = c["name"]
        keys[name] = list(layer.state_dict().keys())
        for k, v in layer.state_dict().items():
            res[f"{name}.{k}"] = v.numpy()
        x = closed_form_input(c["x"], DT).requires_grad_(True)
        y = layer(x)
        (y * rotation_cotangent(y.shape, DT)).sum().backward()
        res[name + ".y"] = y.detach().numpy()
        res[name + ".dx"] = x.grad.numpy()
        for k, p in layer.named_parameters():
            res[f"{name}.grad.{k}"] = p.grad.numpy()
    out = {k: np.asarray(v, dtype=np.float32) for k, v in res.items()}
    out["meta"] = json.dumps(META)
    out["layer_keys"] = json.dumps(keys)
    np.savez_compressed(os.path.join(HERE, "rotation.npz"), **out)
    print("wrote rotation", len(out), "arrays")


if __name__ == "__main__":
    main()
