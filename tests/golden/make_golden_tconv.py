#!/usr/bin/env python3
"""Generate tests/golden/tconv.npz by IMPORTING THE REFERENCE's quaternion transposed convolution.

Runs only in the build container (needs the reference checkout, read-only), like make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tconv.py

Per case of TCONV_CASES: the reference's y, du, dw0..3 and dbias for the closed-form inputs and cotangent, computed in
float64 and stored as float32.  Plus one QuaternionTransposeConv built with its seeded initialisation: its weights, and
y for the closed-form input.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from quaternion import quaternion_ops as RQ                                   # noqa: E402  (reference)
from quaternion.quaternion_layers import QuaternionTransposeConv as RQTConv   # noqa: E402  (reference)

from oracle.seld_oracle import closed_form_input                              # noqa: E402
from tests.golden.tconv_cases import LAYER_CASE, TCONV_CASES, tconv_cotangent, tconv_inputs   # noqa: E402

META = dict(torch=torch.__version__, numpy=np.__version__,
            reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11")
DT = torch.float64


def main():
    res = {}
    for case in TCONV_CASES:
        name = case["name"]
        x, ws, bias = tconv_inputs(case, DT)
        x.requires_grad_(True)
        for w in ws:
            w.requires_grad_(True)
        if bias is not None:
            bias.requires_grad_(True)
        y = RQ.quaternion_transpose_conv(x, *ws, bias, case["stride"], case["padding"], case["output_padding"], 1,
                                         case["dilation"])
        (y * tconv_cotangent(y.shape, DT)).sum().backward()
        res[name + ".y"] = y.detach().numpy()
        res[name + ".du"] = x.grad.numpy()
        for i, w in enumerate(ws):
            res[f"{name}.dw{i}"] = w.grad.numpy()
        if bias is not None:
            res[name + ".dbias"] = bias.grad.numpy()
    c = LAYER_CASE
    np.random.seed(c["np_seed"])
    layer = RQTConv(c["in_channels"], c["out_channels"], c["kernel_size"], c["stride"], dilatation=c["dilatation"],
                    padding=c["padding"], output_padding=c["output_padding"], seed=c["seed"])
    for k, v in layer.state_dict().items():
        res["layer." + k] = v.numpy()
    with torch.no_grad():
        sd = {k: v.double() for k, v in layer.state_dict().items()}
        y = RQ.quaternion_transpose_conv(closed_form_input(c["x"], DT), sd["r_weight"], sd["i_weight"], sd["j_weight"],
                                         sd["k_weight"], sd["bias"], c["stride"], c["padding"], c["output_padding"], 1,
                                         c["dilatation"])
    res["layer.y"] = y.numpy()
    out = {k: np.asarray(v, dtype=np.float32) for k, v in res.items()}
    out["meta"] = json.dumps(META)
    out["layer_keys"] = json.dumps(list(layer.state_dict().keys()))
    np.savez_compressed(os.path.join(HERE, "tconv.npz"), **out)
    print("wrote tconv", {k: v.shape for k, v in out.items() if k not in ("meta", "layer_keys")})


if __name__ == "__main__":
    main()
