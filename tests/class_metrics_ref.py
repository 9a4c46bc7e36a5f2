"""A numpy restatement of the breakdown table of hip_ops.score_events_by (include/seld_hip.h), written from its definition
on top of tests/event_metrics_ex_helpers.py: per recording, rows 0 .. C - 1 the classes, row C "other", row C + 1 "all";
16 counters in EVENT_METRIC_COUNTERS order and total_DE.

  * DCASE counters (3..12) and total_DE of a class row: the block metrics of the two lists filtered to that class, which
    also yields the class-wise S, D, I; of row "all": the block metrics of the whole lists (S, D, I across classes).
  * detection counters (0..2 with the distance threshold, 13..15 on the class alone), row by row: a prediction adds 1 to
    the FP of its class, 2 where its frame has no reference row at all; a reference adds 2 to the FN of its class where
    its frame has no prediction row at all, else TP + 1 and FP - 1 when a prediction of its class matches, FN + 1 when not.
    Rows whose frame is no integer in [0, n_frames) take no part.  Row "all" is the sum of the rows.
Also the tolerance of every total_DE entry (total_de_tolerance over the pairs scored for it)."""
import numpy as np

from tests import event_metrics_ex_helpers as XH

N = 16
DETECTION = (0, 1, 2, 13, 14, 15)
SUMMED = tuple(k for k in range(N) if k not in (6, 7, 8))      # counters whose row "all" is the sum of rows 0 .. C


def _whole_in(v, lo, hi):
    return (v >= lo) & (v < hi) & (v == np.floor(v))


def detection_rows(pred, true, n_frames, C, spatial_threshold):
    """(C + 1, 16) int64: the detection counters of one recording attributed to class rows (the others zero)."""
    out = np.zeros((C + 1, N), dtype=np.int64)
    cart = pred.shape[1] == 5
    p, t = (r[_whole_in(r[:, 0], 0, n_frames)] for r in (pred, true))
    row_of = lambda c: int(c) if _whole_in(c, 0, C) else C      # noqa: E731
    for e in p:
        add = 1 if (t[:, 0] == e[0]).any() else 2
        out[row_of(e[1]), 14] += add
        if cart:
            out[row_of(e[1]), 1] += add
    for e in t:
        row, mates = row_of(e[1]), p[p[:, 0] == e[0]]
        if len(mates) == 0:
            out[row, 15] += 2
            if cart:
                out[row, 2] += 2
            continue
        same = mates[:, 1] == e[1]
        hits = [(13, bool(same.any()))]
        if cart:
            hits.append((0, bool((same & (np.sqrt(((mates[:, 2:] - e[2:]) ** 2).sum(1)) < spatial_threshold)).any())))
        for k, hit in hits:                             # k: the TP of the triple
            if hit:
                out[row, k] += 1
                out[row, k + 1] -= 1
            else:
                out[row, k + 2] += 1
    return out


def recording_table(pred, true, case):
    """((C + 2, 16) int64, (C + 2,) float64 total_DE, (C + 2,) float64 tolerance) of one recording."""
    C = case["nb_classes"]
    cnt, de, tol = np.zeros((C + 2, N), dtype=np.int64), np.zeros(C + 2), np.zeros(C + 2)
    cnt[:C + 1] = detection_rows(pred, true, case["n_frames"], C, case["spatial_threshold"])
    cnt[C + 1, list(DETECTION)] = cnt[:C + 1][:, list(DETECTION)].sum(0)
    for c in list(range(C)) + ([C + 1] if C else []):
        if c < C:                                       # the lists filtered to the class, relabelled as the only class 0
            p, t = (np.concatenate((r[r[:, 1] == c][:, :1], np.zeros((int((r[:, 1] == c).sum()), 1)), r[r[:, 1] == c][:, 2:]), 1)
                    for r in (pred, true))
            nb = 1
        else:
            p, t, nb = pred, true, C
        info = {}
        dc, total = XH.dcase_counts(p, t, case["n_frames"], case["fpb"], nb, case["doa_threshold"], info)
        cnt[c, 3:13], de[c] = dc, total
        tol[c] = XH.total_de_tolerance(total, info.get("angles", []))
    return cnt, de, tol


def table(case):
    """(counters (R, C + 2, 16), total_de (R, C + 2), tolerance (R, C + 2)) of a case."""
    parts = [recording_table(p, t, case) for p, t in zip(case["pred"], case["true"])]
    return tuple(np.stack([part[k] for part in parts]) for k in range(3))
