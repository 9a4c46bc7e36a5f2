"""Writes tests/golden/hc_conv_bits.json: the kernel labels and the SHA-256 of the output bytes of every launch of
tests/golden/hc_conv_bits_cases.py, on the MI355X.

The fixture pins the bits of hc_conv_kernel, hc_conv_vec_kernel and hc_conv_smallk_kernel: it is written ONCE, by the
library of the commit that precedes a change to them or to what they share, and tests/test_gpu_hc_conv_bits.py holds every
later build to it.  Re-run it only when a change of the summation order is intended, with SELD_HIP_LIB naming the library
of the commit that precedes the change and that commit's id on the command line:

    SELD_HIP_LIB=/path/to/parent/libseld_hip.so python tests/golden/make_golden_hc_conv_bits.py --commit <id> [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "hc_conv_bits.json")
PKG = "sound-event-localization-and-detection_amd"
SWITCHES = ("SELD_CONV_NO_HCQ", "SELD_CONV_CFG", "SELD_CONV_NO_SMALLK")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="commit whose library is loaded")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from tests.golden import hc_conv_bits_cases as C
    from tests.test_hc_exact_host import library_labels
    P = importlib.import_module(PKG)
    dev = torch.device("cuda:0")
    assert P.hip_ops.STATS_REPLICAS == C.STATS_REPLICAS
    doc = {"written_by": f"the library of commit {args.commit}", "device": torch.cuda.get_device_name(0), "cases": {}}
    for case in C.CASES:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(case["env"])
        P._lib.reload_env()
        P.hip_ops._drop_kernel_choice_caches()
        labels = library_labels(P, case)
        assert labels == case["labels"], (case["name"], labels)
        doc["cases"][case["name"]] = {"labels": {str(w): v for w, v in labels.items() if w < 2},
                                      "sha256": {n: C.digest(v) for n, v in C.run_case(P, case, dev).items()}}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(args.out, len(doc["cases"]), "cases,", sum(len(v["sha256"]) for v in doc["cases"].values()), "digests")


if __name__ == "__main__":
    main()
