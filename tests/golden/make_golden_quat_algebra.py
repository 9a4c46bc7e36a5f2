#!/usr/bin/env python3
"""Generate tests/golden/quat_algebra.npz by IMPORTING THE REFERENCE's quaternion_ops and dual_quaternion_ops.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_quat_algebra.py

Per case of QUAT_ALGEBRA_CASES the reference's function is called in float64 on the closed-form input(s); for the
closed-form cotangent the fixture stores, as float32, y, dx (the gradient of the first argument) and, for the product,
dq1.  A case the reference raises on stores nothing; `meta` lists those cases with the exception's type name.  The
archive is written with fixed timestamps, so that regenerating it gives the same bytes.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["SELD_REFERENCE"])

from dual_quaternion import dual_quaternion_ops as RD            # noqa: E402  (reference)
from quaternion import quaternion_ops as RQ                      # noqa: E402  (reference)

from tests.golden.quat_algebra_cases import QUAT_ALGEBRA_CASES, quat_cotangent, quat_inputs  # noqa: E402

META = dict(torch=torch.__version__, numpy=np.__version__,
            reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11")
DT = torch.float64


def main():
    res, refused = {}, {}
    for c in QUAT_ALGEBRA_CASES:
        name = c["name"]
        fn = getattr(RQ if c["module"] == "Q" else RD, c["op"])
        args = [a.requires_grad_(True) for a in quat_inputs(c, DT)]
        try:
            y = fn(*args, **c["kwargs"])
        except Exception as e:          # noqa: BLE001  (which inputs the reference refuses, and how, is the record)
            refused[name] = type(e).__name__
            continue
        (y * quat_cotangent(c, y.shape, DT)).sum().backward()
        res[name + ".y"] = y.detach().numpy()
        res[name + ".dx"] = args[0].grad.numpy()
        if len(args) == 2:
            res[name + ".dq1"] = args[1].grad.numpy()
        for k in [k for k in res if k.startswith(name + ".")]:
            assert np.isfinite(res[k]).all(), k
    for c in QUAT_ALGEBRA_CASES:
        assert (c["name"] + ".y" in res) != (c["name"] in refused), c["name"]
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in res.items()}
    out["meta"] = np.asarray(json.dumps(dict(META, refused=refused), sort_keys=True))
    path = os.path.join(HERE, "quat_algebra.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, out[k], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print("wrote quat_algebra", len(out), "arrays", os.path.getsize(path), "bytes; refused:", refused)


if __name__ == "__main__":
    main()
