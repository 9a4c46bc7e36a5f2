#!/usr/bin/env python3
"""Generate tests/golden/class_metrics.npz by IMPORTING THE REFERENCE's metrics.py and Dcase21_metrics.py and calling them,
recording by recording and class by class, on the cases of event_metrics_cases.py, event_metrics_ex_cases.py and
class_metrics_cases.py (the recipe of make_golden_event_metrics.py, whose stand-ins it uses):

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_class_metrics.py

Per case and recording, under `<name>.`:
  all     (R, 16) int64   row "all": the reference on that recording alone, in EVENT_METRIC_COUNTERS order -- TP, FP, FN of
                          location_sensitive_detection (Cartesian cases), the ten SELDMetrics counters after segment_labels +
                          update_seld_scores, TP, FP, FN of sed_score_computation.  -1: not recorded (the detection part of
                          a case it answers with KeyError; the Euclidean counters of spherical rows)
  all_de  (R,)            its _total_DE
  cls     (R, C, 10)      the ten SELDMetrics counters of every class row: segment_labels + a SELDMetrics on the two lists
                          filtered to that class (association, Nref and the block count are class-wise, so this is the
                          class's share, and S, D, I come out class-wise by definition)
  cls_de  (R, C)          their _total_DE
Checked here: the numpy restatement of tests/class_metrics_ref.py agrees with all of it (integers exactly, total_DE within
its tolerance) and keeps its sum invariant; associations lead by 1e-9 and track averages stay 1e-9 away from the threshold
(the "ties" cases tie on purpose, harmlessly); and in case by_five the class-wise S differs from the cross-class one.
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

from tests import class_metrics_ref as CR  # noqa: E402
from tests import event_metrics_ex_helpers as XH  # noqa: E402
from tests.event_metrics_helpers import detection_counts  # noqa: E402
from tests.golden.class_metrics_cases import ALL_CASES  # noqa: E402
from tests.golden.event_metrics_ex_cases import frame_dict  # noqa: E402
from tests.golden.make_golden_event_metrics import import_reference  # noqa: E402


def dcase_of(RD, pred, true, case):
    em = RD.SELDMetrics(doa_threshold=case["doa_threshold"], nb_classes=case["nb_classes"])
    em.update_seld_scores(RD.segment_labels(frame_dict(pred), case["n_frames"], case["fpb"]),
                          RD.segment_labels(frame_dict(true), case["n_frames"], case["fpb"]))
    return ([int(v) for v in (em._TP, em._FP, em._FN, em._S, em._D, em._I, em._Nref, em._DE_TP, em._DE_FP, em._DE_FN)],
            float(em._total_DE))


def main():
    stubbed = []
    RM = import_reference("metrics", stubbed)
    RD = import_reference("Dcase21_metrics", stubbed)
    out = {}
    for c in ALL_CASES:
        name, C, R = c["name"] + ".", c["nb_classes"], len(c["pred"])
        info = {}
        for p, t in zip(c["pred"], c["true"]):
            XH.dcase_counts(p, t, c["n_frames"], c["fpb"], C, c["doa_threshold"], info)
        assert info.get("bad_ties", 0) == 0 and info.get("gap", np.inf) > 1e-9, (c["name"], info.get("gap"))
        assert c["kind"] == "ties" or (info.get("ties", 0) == 0 and info.get("lead", np.inf) > 1e-9), (c["name"], info.get("lead"))
        all_c, all_de = np.full((R, 16), -1, dtype=np.int64), np.zeros(R)
        cls_c, cls_de = np.zeros((R, C, 10), dtype=np.int64), np.zeros((R, C))
        for r, (p, t) in enumerate(zip(c["pred"], c["true"])):
            pa, ta = (a if a.shape[0] else np.array([]) for a in (p, t))
            if c["lsd"]:
                if c["coords"] == 3:
                    all_c[r, 0:3] = RM.location_sensitive_detection(pa, ta, c["n_frames"], c["spatial_threshold"])[:3]
                try:
                    all_c[r, 13:16] = RM.sed_score_computation(pa, ta, c["n_frames"], c["spatial_threshold"])[:3]
                except ZeroDivisionError:       # raised after the counting: the counters come from the class-only restatement
                    assert t.shape[0] == 0 or p.shape[0] == 0
                    all_c[r, 13:16] = detection_counts(p, t, c["n_frames"], c["spatial_threshold"])[1]
            else:
                try:
                    RM.location_sensitive_detection(pa, ta, c["n_frames"], c["spatial_threshold"])
                    raise AssertionError("expected KeyError")
                except KeyError:
                    pass
            all_c[r, 3:13], all_de[r] = dcase_of(RD, p, t, c)
            for k in range(C):
                cls_c[r, k], cls_de[r, k] = dcase_of(RD, p[p[:, 1] == k], t[t[:, 1] == k], c)
        mine_c, mine_de, tol = CR.table(c)
        known = all_c >= 0
        assert (mine_c[:, C + 1][known] == all_c[known]).all(), (c["name"], mine_c[:, C + 1], all_c)
        assert (mine_c[:, :C, 3:13] == cls_c).all(), c["name"]
        assert (np.abs(mine_de[:, C + 1] - all_de) <= tol[:, C + 1]).all() and (np.abs(mine_de[:, :C] - cls_de) <= tol[:, :C]).all()
        assert (mine_c[:, :C + 1][..., list(CR.SUMMED)].sum(1) == mine_c[:, C + 1][..., list(CR.SUMMED)]).all(), c["name"]
        assert (cls_c[..., [0, 1, 2, 6, 7, 8, 9]].sum(1) == all_c[:, [3, 4, 5, 9, 10, 11, 12]]).all(), c["name"]
        if c["name"] == "by_five":                  # without this no test could tell the two definitions of S apart
            assert cls_c[..., 3].sum() != all_c[:, 6].sum(), "by_five: class-wise and cross-class S agree"
        out[name + "all"], out[name + "all_de"], out[name + "cls"], out[name + "cls_de"] = all_c, all_de, cls_c, cls_de
        print(f"{c['name']:20s} R {R} C {C} all {all_c.sum(0).tolist()} S by class {int(cls_c[..., 3].sum())} "
              f"DE {all_de.sum():.6f} lead {info.get('lead', np.inf):.2e} gap {info.get('gap', np.inf):.2e}")
    out["meta"] = np.asarray(json.dumps(dict(numpy=np.__version__, scipy=__import__("scipy").__version__, stand_ins=stubbed,
                                             reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11"),
                                        sort_keys=True))
    path = os.path.join(HERE, "class_metrics.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k], order="C"), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print("wrote class_metrics", len(out), "arrays", os.path.getsize(path), "bytes; stand-ins:", stubbed)


if __name__ == "__main__":
    main()
