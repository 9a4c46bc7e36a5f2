"""Host arithmetic on the breakdown tables of hip_ops.score_events_by / metrics_accumulate_by: per-class scores,
class-wise macro averages and leave-one-recording-out (jackknife) estimates.  Plain numpy on small arrays; no device work.

A table is (counters (R, C + 2, 16) int64 in hip_ops.EVENT_METRIC_COUNTERS order, total_de (R, C + 2) float64): rows
0 .. C - 1 the classes, row C "other", row C + 1 "all" (include/seld_hip.h).  Device tensors are read back once.
Out of scope here: confusion matrices across classes, per-class thresholds, t-based confidence intervals (scipy is not a
dependency: the jackknife returns bias and standard error, and the caller picks a quantile)."""
import sys

import numpy as np

eps = np.finfo(float).eps

__all__ = ["totals", "class_scores", "macro_scores", "jackknife", "macro_score_vector"]


def _host(counters, total_de):
    c = counters.detach().cpu().numpy() if hasattr(counters, "detach") else np.asarray(counters)
    d = total_de.detach().cpu().numpy() if hasattr(total_de, "detach") else np.asarray(total_de)
    c, d = c.astype(np.int64, copy=False), d.astype(np.float64, copy=False)
    if c.ndim < 2 or c.shape[-1] != 16 or c.shape[-2] < 2 or d.shape != c.shape[:-1]:
        raise ValueError(f"class_metrics: tables of shapes {c.shape} and {d.shape}; expected (.., C + 2, 16) and (.., C + 2)")
    return c, d


def totals(counters, total_de):
    """The table summed over its recordings: ((C + 2, 16) int64, (C + 2,) float64).  Row "all" of the result is what
    score_events / metrics_accumulate put into their accumulators for the same input.  A table that is summed already is
    returned as it is."""
    c, d = _host(counters, total_de)
    return (c, d) if c.ndim == 2 else (c.reshape(-1, *c.shape[-2:]).sum(0), d.reshape(-1, d.shape[-1]).sum(0))


def _prf(tp, fp, fn):
    """Precision, recall and F1 as metrics.py writes them (compute_f_score: epsilon in every denominator)."""
    e = sys.float_info.epsilon
    precision = tp / (tp + fp + e)
    recall = tp / (tp + fn + e)
    return precision, recall, 2 * ((precision * recall) / (precision + recall + e))


def class_scores(counters, total_de):
    """Per class (arrays of C entries, in a dict):
      precision, recall, f1              of the distance-thresholded detection (counters 0..2), metrics.py's formulas
      sed_precision, sed_recall, sed_f1  of the class-only detection (counters 13..15)
      ER, F, LE, LR                      SELDMetrics.compute_seld_scores on the class's DCASE counters (S, D, I class-wise);
                                         LE = 180 where the class has no matched track (DE_TP == 0)
      Nref                               reference tracks of the class, summed over the blocks"""
    c, d = totals(counters, total_de)
    c, d = c[:-2].astype(np.float64), d[:-2]
    out = {}
    out["precision"], out["recall"], out["f1"] = _prf(c[:, 0], c[:, 1], c[:, 2])
    out["sed_precision"], out["sed_recall"], out["sed_f1"] = _prf(c[:, 13], c[:, 14], c[:, 15])
    out["ER"] = (c[:, 6] + c[:, 7] + c[:, 8]) / (c[:, 9] + eps)
    out["F"] = c[:, 3] / (eps + c[:, 3] + 0.5 * (c[:, 4] + c[:, 5]))
    out["LE"] = np.where(c[:, 10] != 0, d / (c[:, 10] + eps), 180.0)
    out["LR"] = c[:, 10] / (eps + c[:, 10] + c[:, 12])
    out["Nref"] = c[:, 9].astype(np.int64)
    return out


def early_stopping_metric(sed_error, doa_error):
    return np.mean([sed_error[0], 1 - sed_error[1], doa_error[0] / 180, 1 - doa_error[1]])


def macro_scores(counters, total_de, over="reference"):
    """Class-wise macro averages: dict(ER, F, LE, LR, early_stopping_metric, classes).  over='reference': the mean over the
    classes the reference holds (Nref > 0), as DCASE 2022 reports; over='all': over all C classes.  With no class to
    average over (an empty reference), ER, F, LE, LR are those of a class without events: 0, 0, 180, 0."""
    if over not in ("reference", "all"):
        raise ValueError(f"macro_scores: over must be 'reference' or 'all', got {over!r}")
    s = class_scores(counters, total_de)
    keep = s["Nref"] > 0 if over == "reference" else np.ones(s["Nref"].shape, dtype=bool)
    if keep.any():
        out = {k: float(np.mean(s[k][keep])) for k in ("ER", "F", "LE", "LR")}
    else:
        out = dict(ER=0.0, F=0.0, LE=180.0, LR=0.0)
    out["early_stopping_metric"] = float(early_stopping_metric([out["ER"], out["F"]], [out["LE"], out["LR"]]))
    out["classes"] = int(keep.sum())
    return out


def macro_score_vector(counters, total_de, over="reference"):
    """macro_scores as the vector [ER, F, LE, LR, early_stopping_metric]: a `score` for jackknife."""
    m = macro_scores(counters, total_de, over)
    return np.array([m["ER"], m["F"], m["LE"], m["LR"], m["early_stopping_metric"]])


def jackknife(counters, total_de, score=macro_score_vector):
    """Leave-one-recording-out estimates of `score`, a function of totals ((C + 2, 16), (C + 2,)) returning a vector.
    Returns dict(estimate: score of all R recordings, leave_one_out (R, n): score of the totals minus each recording's
    slab, bias: (R - 1) (mean_i theta_(i) - theta), stderr: sqrt((R - 1) / R * sum_i (theta_(i) - mean)^2)).  R >= 2."""
    c, d = _host(counters, total_de)
    if c.ndim != 3 or c.shape[0] < 2:
        raise ValueError(f"jackknife: needs the tables of at least two recordings, got counters of shape {c.shape}")
    R = c.shape[0]
    tc, td = c.sum(0), d.sum(0)
    theta = np.atleast_1d(np.asarray(score(tc, td), dtype=np.float64))
    loo = np.stack([np.atleast_1d(np.asarray(score(tc - c[r], td - d[r]), dtype=np.float64)) for r in range(R)])
    mean = loo.mean(0)
    return dict(estimate=theta, leave_one_out=loo, bias=(R - 1) * (mean - theta),
                stderr=np.sqrt((R - 1) / R * ((loo - mean) ** 2).sum(0)))
