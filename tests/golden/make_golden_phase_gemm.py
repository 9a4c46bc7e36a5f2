"""Writes tests/golden/phase_gemm_bits.json: the SHA-256 of the output bytes of every launch of
tests/golden/phase_gemm_cases.py (the ten transposed 2-D forwards and the true 3-D launches) and the kernel label of
each, on the MI355X.

The fixture pins the bits of hc_tconv_kernel, hc_conv3d_fwd_kernel and hc_conv3d_phase_kernel: it is written ONCE, by
the library of the commit that precedes a change to their body, and tests/test_gpu_phase_gemm.py holds every later
build to it.  Re-run it only when a change of the summation order is intended, with SELD_HIP_LIB naming the library
of the commit that precedes the change and that commit's id on the command line:

    SELD_HIP_LIB=/path/to/parent/libseld_hip.so python tests/golden/make_golden_phase_gemm.py --commit <id> [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "phase_gemm_bits.json")
PKG = "sound-event-localization-and-detection_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="commit whose library is loaded")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from tests.golden import phase_gemm_cases as C
    H = importlib.import_module(PKG).hip_ops
    dev = torch.device("cuda:0")
    doc = {"written_by": f"the library of commit {args.commit}", "device": torch.cuda.get_device_name(0),
           "twin": {}, "c3": {}}
    for case in C.TWIN_CASES:
        label, y2, y3 = C.run_twin(H, case, dev)
        torch.cuda.synchronize()
        doc["twin"][case["name"]] = {"label": label, "sha256": C.digest(y2), "equals_depth_1": torch.equal(y2, y3.view(y2.shape))}
    for case in C.C3_CASES:
        label, y = C.run_c3(H, case, dev)
        torch.cuda.synchronize()
        doc["c3"][case["name"]] = {"label": label, "sha256": C.digest(y)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(args.out, len(doc["twin"]), "+", len(doc["c3"]), "launches;",
          sum(not v["equals_depth_1"] for v in doc["twin"].values()), "twin cases differ at depth 1")


if __name__ == "__main__":
    main()
