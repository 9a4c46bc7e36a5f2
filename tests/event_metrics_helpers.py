"""A numpy restatement of event-list scoring, working on rows [frame, class, x, y, z]: what location_sensitive_detection,
sed_score_computation and segment_labels + SELDMetrics.update_seld_scores count, written from their definition.  It also
reports how close a case comes to a decision boundary, which the fixture generator bounds."""
import itertools
import sys

import numpy as np

EPS = np.finfo(float).eps
DCASE_NAMES = ("TP", "FP", "FN", "S", "D", "I", "Nref", "DE_TP", "DE_FP", "DE_FN")


def angular_distance(a, b):
    """Degrees between two Cartesian vectors, each normalised with 1e-10 under its root."""
    a, b = a / np.sqrt(a[0] ** 2 + a[1] ** 2 + a[2] ** 2 + 1e-10), b / np.sqrt(b[0] ** 2 + b[1] ** 2 + b[2] ** 2 + 1e-10)
    return np.arccos(np.clip(a[0] * b[0] + a[1] * b[1] + a[2] * b[2], -1, 1)) * 180 / np.pi


def detection_counts(pred, true, n_frames, spatial_threshold, margins=None):
    """([TP, FP, FN] with the distance threshold, [TP, FP, FN] on the class alone) of one recording."""
    out = np.zeros((2, 3), dtype=np.int64)
    for rec in (pred, true):
        f = rec[:, 0]
        if ((f < 0) | (f >= n_frames) | (f != np.floor(f))).any():
            raise KeyError(float(f[(f < 0) | (f >= n_frames) | (f != np.floor(f))][0]))
    for frame in np.union1d(pred[:, 0], true[:, 0]):
        p, t = pred[pred[:, 0] == frame], true[true[:, 0] == frame]
        if len(t) == 0:
            out[:, 1] += 2 * len(p)
        elif len(p) == 0:
            out[:, 2] += 2 * len(t)
        else:
            same = t[:, None, 1] == p[None, :, 1]
            dist = np.sqrt(((t[:, None, 2:] - p[None, :, 2:]) ** 2).sum(-1))
            if margins is not None and same.any():
                margins["spatial"] = min(margins["spatial"], np.abs(dist[same] - spatial_threshold).min())
            for k, hit in enumerate(((same & (dist < spatial_threshold)).any(1), same.any(1))):
                m = int(hit.sum())
                out[k] += (m, len(p) - m, len(t) - m)
    return out[0].tolist(), out[1].tolist()


def best_assignment(cost):
    """(rows, columns) of the cheapest pairing of min(g, q) references with predictions, and its lead over the runner-up."""
    g, q = cost.shape
    cands = []
    if g <= q:
        for cols in itertools.permutations(range(q), g):
            cands.append((sum(cost[i, c] for i, c in enumerate(cols)), list(range(g)), list(cols)))
    else:
        for rws in itertools.permutations(range(g), q):
            cands.append((sum(cost[r, j] for j, r in enumerate(rws)), list(rws), list(range(q))))
    cands.sort(key=lambda c: c[0])
    lead = cands[1][0] - cands[0][0] if len(cands) > 1 else np.inf
    return cands[0][1], cands[0][2], lead


def dcase_counts(pred, true, n_frames, fpb, nb_classes, doa_threshold, margins=None):
    """(the ten SELDMetrics counters in DCASE_NAMES order, _total_DE) of one recording."""
    c = dict.fromkeys(DCASE_NAMES, 0)
    total_de = 0.0
    for b in range(int(np.ceil(n_frames / float(fpb)))):
        loc_fn = loc_fp = 0
        for cls in range(nb_classes):
            sides = []
            for rec in (true, pred):
                r = rec[(rec[:, 0] >= b * fpb) & (rec[:, 0] < (b + 1) * fpb) & (rec[:, 0] == np.floor(rec[:, 0])) & (rec[:, 1] == cls)]
                sides.append({f: r[r[:, 0] == f][:, 2:] for f in np.unique(r[:, 0])})
            gt, pr = sides
            nb_gt = max(len(v) for v in gt.values()) if gt else 0
            nb_pred = max(len(v) for v in pr.values()) if pr else 0
            c["Nref"] += nb_gt
            if gt and pr:
                tracks = {}
                for f in sorted(set(gt) & set(pr)):
                    cost = np.array([[angular_distance(a, q) for q in pr[f]] for a in gt[f]])
                    rws, cols, lead = best_assignment(cost)
                    if margins is not None:
                        margins["assignment"] = min(margins["assignment"], lead)
                    for r_, c_ in zip(rws, cols):
                        tracks.setdefault(r_, []).append(cost[r_, c_])
                if not tracks:
                    loc_fn += nb_pred
                    c["FN"] += nb_pred
                    c["DE_FN"] += nb_pred
                else:
                    for dists in tracks.values():
                        avg = sum(dists) / len(dists)
                        if margins is not None:
                            margins["doa"] = min(margins["doa"], abs(avg - doa_threshold))
                        total_de += avg
                        c["DE_TP"] += 1
                        if avg <= doa_threshold:
                            c["TP"] += 1
                        else:
                            loc_fp += 1
                            c["FP"] += 1
                    if nb_pred > nb_gt:
                        loc_fp += nb_pred - nb_gt
                        c["FP"] += nb_pred - nb_gt
                        c["DE_FP"] += nb_pred - nb_gt
                    elif nb_pred < nb_gt:
                        loc_fn += nb_gt - nb_pred
                        c["FN"] += nb_gt - nb_pred
                        c["DE_FN"] += nb_gt - nb_pred
            elif gt:
                loc_fn += nb_gt
                c["FN"] += nb_gt
                c["DE_FN"] += nb_gt
            elif pr:
                loc_fp += nb_pred
                c["FP"] += nb_pred
                c["DE_FP"] += nb_pred
        c["S"] += min(loc_fp, loc_fn)
        c["D"] += max(0, loc_fn - loc_fp)
        c["I"] += max(0, loc_fp - loc_fn)
    return [c[k] for k in DCASE_NAMES], total_de


def seld_scores(d, total_de):
    """compute_seld_scores: (ER, F, LE, LR) from the ten counters."""
    c = dict(zip(DCASE_NAMES, d))
    return [(c["S"] + c["D"] + c["I"]) / float(c["Nref"] + EPS), c["TP"] / (EPS + c["TP"] + 0.5 * (c["FP"] + c["FN"])),
            total_de / float(c["DE_TP"] + EPS) if c["DE_TP"] else 180, c["DE_TP"] / (EPS + c["DE_TP"] + c["DE_FN"])]


def f_score(TP, FP, FN):
    precision = TP / (TP + FP + sys.float_info.epsilon)
    recall = TP / (TP + FN + sys.float_info.epsilon)
    return 2 * ((precision * recall) / (precision + recall + sys.float_info.epsilon))


def score_case(case, margins=None):
    """A whole case: dict(lsd, sed (None for a case without detection part), dcase, total_DE, scores)."""
    lsd, sed = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
    dc, de = np.zeros(10, dtype=np.int64), 0.0
    for p, t in zip(case["pred"], case["true"]):
        if case["lsd"]:
            a, b = detection_counts(p, t, case["n_frames"], case["spatial_threshold"], margins)
            lsd += a
            sed += b
        d, e = dcase_counts(p, t, case["n_frames"], case["fpb"], case["nb_classes"], case["doa_threshold"], margins)
        dc += d
        de += e
    return dict(lsd=lsd.tolist() if case["lsd"] else None, sed=sed.tolist() if case["lsd"] else None, dcase=dc.tolist(),
                total_DE=de, scores=seld_scores(dc.tolist(), de))


def offsets_of(lists):
    return np.concatenate(([0], np.cumsum([len(r) for r in lists]))).astype(np.int64)


def stable_by_frame(rec):
    return rec[np.argsort(rec[:, 0], kind="stable")]


def rebuild_segments(index, keys, counts, entries):
    """The nested dictionary of segment_labels from its flattened record (make_golden_event_metrics.flatten_segments)."""
    out = {b: {} for b in range(int(index[0, 0]))}
    k = e = 0
    for b, c, n in index[1:].tolist():
        ks, vals = [], []
        for _ in range(n):
            ks.append(int(keys[k]))
            vals.append([[float(x), float(y), float(z), int(ev)] for x, y, z, ev in entries[e:e + counts[k]].tolist()])
            e += int(counts[k])
            k += 1
        out[b].setdefault(c, []).append([ks, vals])
    return out
