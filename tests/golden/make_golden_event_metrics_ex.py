#!/usr/bin/env python3
"""Generate tests/golden/event_metrics_ex.npz by IMPORTING THE REFERENCE's metrics.py and Dcase21_metrics.py and calling
them on the cases of event_metrics_ex_cases.py (the recipe of make_golden_event_metrics.py, whose stand-ins it uses):

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_event_metrics_ex.py

Per scoring case, under `<name>.`:
  dcase        _TP _FP _FN _S _D _I _Nref _DE_TP _DE_FP _DE_FN of one SELDMetrics after segment_labels + update_seld_scores
               on every recording;  total_DE its _total_DE;  scores its compute_seld_scores()
  sed          TP, FP, FN of sed_score_computation (it looks at the class alone, so it takes rows of either width)
  lsd          TP, FP, FN of location_sensitive_detection, for Cartesian cases
  total_DE_tol what the device's total_DE may differ by: max(1e-12 total_DE, the sum of pair_tolerance over the scored
               pairs) (tests/event_metrics_ex_helpers.py)
and under `assign.cart.` / `assign.sph.`: cost, row, col (81, 8; padded with 0 / -1 / -1), pairs (81) and tol (81, 8) of
least_distance_between_gt_pred on assign_problems(), one problem per (g, q) in 0 .. 8.

Conditions, checked on the reference's own numbers; a case that violates one is an error here (pick another seed):
  * every scored association leads the next best by at least 1e-6 degrees, by enumeration of all pairings.  In the "ties"
    cases cells built from duplicated rows tie on purpose: there every pairing within 1e-6 of the best must give every
    reference track the same distance.
  * every track average is at least 1e-3 degrees away from doa_threshold.
  * in the "general" cases every scored pair is between 1 and 179 degrees apart.
The numpy restatement of tests/event_metrics_ex_helpers.py must agree with the reference on every case as well.
The archive is written with fixed timestamps, so that regenerating it gives the same bytes.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import event_metrics_ex_helpers as XH  # noqa: E402
from tests.event_metrics_helpers import detection_counts, seld_scores  # noqa: E402
from tests.golden.event_metrics_ex_cases import EVENT_METRIC_EX_CASES, assign_problems, frame_dict  # noqa: E402
from tests.golden.make_golden_event_metrics import import_reference  # noqa: E402


def main():
    stubbed = []
    RM = import_reference("metrics", stubbed)
    RD = import_reference("Dcase21_metrics", stubbed)
    out = {}
    for c in EVENT_METRIC_EX_CASES:
        name = c["name"] + "."
        info = {}
        mine_dc, mine_de = XH.score_case(c, info)
        XH.check_conditions(c, info)
        em = RD.SELDMetrics(doa_threshold=c["doa_threshold"], nb_classes=c["nb_classes"])
        lsd, sed = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
        for p, t in zip(c["pred"], c["true"]):
            sed += RM.sed_score_computation(p, t, c["n_frames"], c["spatial_threshold"])[:3]
            assert detection_counts(p, t, c["n_frames"], c["spatial_threshold"])[1] == \
                list(RM.sed_score_computation(p, t, c["n_frames"], c["spatial_threshold"])[:3]), c["name"]
            if c["coords"] == 3:
                lsd += RM.location_sensitive_detection(p, t, c["n_frames"], c["spatial_threshold"])[:3]
            em.update_seld_scores(RD.segment_labels(frame_dict(p), c["n_frames"], c["fpb"]),
                                  RD.segment_labels(frame_dict(t), c["n_frames"], c["fpb"]))
        dc = [int(v) for v in (em._TP, em._FP, em._FN, em._S, em._D, em._I, em._Nref, em._DE_TP, em._DE_FP, em._DE_FN)]
        de = float(em._total_DE)
        scores = [float(v) for v in em.compute_seld_scores()]
        tol = XH.total_de_tolerance(de, info.get("angles", []))
        assert mine_dc == dc, (c["name"], mine_dc, dc)
        assert abs(mine_de - de) <= tol, (c["name"], mine_de, de)
        assert np.allclose(seld_scores(dc, de), scores, rtol=1e-12, atol=1e-12), c["name"]
        out[name + "dcase"] = np.asarray(dc, dtype=np.int64)
        out[name + "sed"] = sed
        if c["coords"] == 3:
            out[name + "lsd"] = lsd
        out[name + "total_DE"] = np.asarray([de])
        out[name + "total_DE_tol"] = np.asarray([tol])
        out[name + "scores"] = np.asarray(scores)
        print(f"{c['name']:15s} rows {sum(len(p) for p in c['pred'])}/{sum(len(t) for t in c['true'])} dcase {dc} DE {de:.6f} "
              f"tol {tol:.2e} lead {info.get('lead', np.inf):.2e} gap {info.get('gap', np.inf):.2e} ties {info.get('ties', 0)} "
              f"cell {info.get('cell', 0)} pairs {len(info.get('angles', []))}")
    for tag, spherical in (("cart", False), ("sph", True)):
        gt, pred, gn, qn = assign_problems(spherical)
        cost, row, col = np.zeros((81, 8)), np.full((81, 8), -1, dtype=np.int32), np.full((81, 8), -1, dtype=np.int32)
        tol, pairs = np.zeros((81, 8)), np.zeros(81, dtype=np.int32)
        for b in range(81):
            g, q = int(gn[b]), int(qn[b])
            cst, r, cl = RD.least_distance_between_gt_pred(gt[b, :g], pred[b, :q])
            n = min(g, q)
            assert len(cst) == len(r) == len(cl) == n and list(r) == sorted(r), (tag, b)
            if n:
                m = XH.cost_matrix(gt[b, :g], pred[b, :q])
                rws, cols, lead, tie = XH.best_assignment(m)
                assert tie is None and lead >= XH.LEAD, (tag, b, lead)
                assert rws == list(r) and cols == list(cl), (tag, b)
                assert cst.min() >= 1.0 and cst.max() <= 179.0, (tag, b, cst)
            cost[b, :n], row[b, :n], col[b, :n], pairs[b] = cst, r, cl, n
            tol[b, :n] = [XH.pair_tolerance(a) for a in cst]
        for k, a in (("cost", cost), ("row", row), ("col", col), ("pairs", pairs), ("tol", tol)):
            out[f"assign.{tag}.{k}"] = a
        print(f"assign.{tag}: 81 problems, {int(pairs.sum())} pairs")
    out["meta"] = np.asarray(json.dumps(dict(numpy=np.__version__, scipy=__import__("scipy").__version__, stand_ins=stubbed,
                                             reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11"),
                                        sort_keys=True))
    path = os.path.join(HERE, "event_metrics_ex.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k], order="C"), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print("wrote event_metrics_ex", len(out), "arrays", os.path.getsize(path), "bytes; stand-ins:", stubbed)


if __name__ == "__main__":
    main()
