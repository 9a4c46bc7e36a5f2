#!/usr/bin/env python3
"""Generate tests/golden/mha_mask.npz by IMPORTING THE REFERENCE's MultiHeadAttention.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mha_mask.py

Per case of MHA_MASK_CASES: y = mha(v, k, q, mask) for separate v, k, q, and for the closed-form cotangent the
gradients of v, k, q, of the four weights and of fc_out.bias.  Computed in float64, stored as float32.
"""
import importlib.machinery
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["SELD_REFERENCE"])
ti = types.ModuleType("torchinfo")             # stand-ins, as in make_golden.py: only used for a summary print / not at all
ti.summary = lambda *a, **k: None
sys.modules["torchinfo"] = ti
sys.modules["librosa"] = types.ModuleType("librosa")
for _m in ("torchinfo", "librosa"):
    sys.modules[_m].__spec__ = importlib.machinery.ModuleSpec(_m, None)

import model as RM                                               # noqa: E402  (reference)

from oracle.seld_oracle import closed_form_fill_                 # noqa: E402
from tests.golden.mha_mask_cases import MHA_MASK_CASES, mha_mask, mha_mask_cotangent, mha_mask_inputs  # noqa: E402

META = dict(torch=torch.__version__, numpy=np.__version__,
            reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11")
DT = torch.float64


def main():
    res = {}
    for c in MHA_MASK_CASES:
        name = c["name"]
        mha = RM.MultiHeadAttention(c["E"], c["heads"]).to(DT)
        closed_form_fill_(list(mha.state_dict().items()), amp=0.6)
        v, k, q = (t.requires_grad_(True) for t in mha_mask_inputs(c, DT))
        y = mha(v, k, q, mha_mask(c))
        (y * mha_mask_cotangent(y.shape, DT)).sum().backward()
        res[name + ".y"] = y.detach().numpy()
        res[name + ".dv"], res[name + ".dk"], res[name + ".dq"] = v.grad.numpy(), k.grad.numpy(), q.grad.numpy()
        res[name + ".dwv"] = mha.values.weight.grad.numpy()
        res[name + ".dwk"] = mha.keys.weight.grad.numpy()
        res[name + ".dwq"] = mha.queries.weight.grad.numpy()
        res[name + ".dwo"] = mha.fc_out.weight.grad.numpy()
        res[name + ".dbo"] = mha.fc_out.bias.grad.numpy()
    out = {k: np.asarray(v, dtype=np.float32) for k, v in res.items()}
    out["meta"] = json.dumps(META)
    np.savez_compressed(os.path.join(HERE, "mha_mask.npz"), **out)
    print("wrote mha_mask", len(out), "arrays", os.path.getsize(os.path.join(HERE, "mha_mask.npz")), "bytes")


if __name__ == "__main__":
    main()
