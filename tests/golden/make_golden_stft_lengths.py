#!/usr/bin/env python3
"""Generate tests/golden/stft_lengths.npz by IMPORTING THE REFERENCE's spectrum_fast.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stft_lengths.py

Per case of STFT_LENGTH_CASES: the reference's output for the seeded input, in the reference's own dtype (float32 for
float32 input, float64 otherwise).  The reference imports torchinfo and librosa at module level without using them
on this path; empty stand-in modules are registered as in make_golden.py.
"""
import importlib.machinery
import json
import os
import sys
import types

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["SELD_REFERENCE"])
ti = types.ModuleType("torchinfo")
ti.summary = lambda *a, **k: None
sys.modules["torchinfo"] = ti
sys.modules["librosa"] = types.ModuleType("librosa")
for _m in ("torchinfo", "librosa"):
    sys.modules[_m].__spec__ = importlib.machinery.ModuleSpec(_m, None)

import utility_functions as RUF                                          # noqa: E402  (reference)

from tests.golden.stft_lengths_cases import STFT_LENGTH_CASES, stft_input, stft_kwargs   # noqa: E402

META = dict(numpy=np.__version__, scipy=scipy.__version__,
            reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11")


def main():
    out = {}
    for case in STFT_LENGTH_CASES:
        y = RUF.spectrum_fast(stft_input(case), **stft_kwargs(case))
        out[case["name"]] = np.asarray(y)
    out["meta"] = json.dumps(META)
    path = os.path.join(HERE, "stft_lengths.npz")
    np.savez_compressed(path, **out)
    print("wrote stft_lengths", {k: (v.shape, str(v.dtype)) for k, v in out.items() if k != "meta"},
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
