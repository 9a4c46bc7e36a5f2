#!/usr/bin/env python3
"""Generate tests/golden/depthwise.npz by IMPORTING THE REFERENCE's depthwise-separable layers.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_depthwise.py

Per case of DEPTHWISE_CASES, for the layer built under torch.manual_seed(seed): its state dict after construction; in
train mode for the closed-form input and cotangent: y, dx and every parameter's gradient, and the running statistics
after that one forward; then the output of an eval-mode forward.  Computed in float64, stored as float32.
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

from tests.golden.depthwise_cases import DEPTHWISE_CASES, depthwise_cotangent, depthwise_input  # noqa: E402

META = dict(torch=torch.__version__, numpy=np.__version__,
            reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11")
DT = torch.float64


def main():
    res, keys = {}, {}
    for c in DEPTHWISE_CASES:
        name = c["name"]
        torch.manual_seed(c["seed"])
        layer = getattr(RDL, "DepthwiseSeparableConv" + c["cls"])(*c["args"])
        keys[name] = list(layer.state_dict().keys())
        for k, v in layer.state_dict().items():
            res[f"{name}.init.{k}"] = v.numpy().copy()
        layer = layer.to(DT).train()
        x = depthwise_input(c, DT).requires_grad_(True)
        y = layer(x)
        (y * depthwise_cotangent(y.shape, DT)).sum().backward()
        res[name + ".y"] = y.detach().numpy()
        res[name + ".dx"] = x.grad.numpy()
        for k, p in layer.named_parameters():
            res[f"{name}.grad.{k}"] = p.grad.numpy()
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            res[f"{name}.train.bn.{k}"] = getattr(layer.bn, k).numpy()
        layer.eval()
        with torch.no_grad():
            res[name + ".y_eval"] = layer(x.detach()).numpy()
    out = {k: np.asarray(v, dtype=np.float32) for k, v in res.items()}
    out["meta"] = json.dumps(META)
    out["layer_keys"] = json.dumps(keys)
    np.savez_compressed(os.path.join(HERE, "depthwise.npz"), **out)
    print("wrote depthwise", len(out), "arrays", os.path.getsize(os.path.join(HERE, "depthwise.npz")), "bytes")


if __name__ == "__main__":
    main()
