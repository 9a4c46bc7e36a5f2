"""A numpy restatement of the DCASE21 block metrics for rows of either width ([frame, class, x, y, z] or [frame, class,
azimuth, elevation] in degrees) and any number of events in a cell, with the quantities the extended fixture's generator
bounds: the lead of every association over its runner-up (by enumeration), the distance of every track average from the
threshold, the angle of every scored pair."""
import itertools

import numpy as np

from tests.event_metrics_helpers import DCASE_NAMES

EPS = np.finfo(float).eps
LEAD = 1e-6             # degrees by which an association must lead the next one
THRESHOLD_GAP = 1e-3    # degrees between a track average and doa_threshold
_MAPS = {}


def cost_matrix(gt, pr):
    """(g, q) degrees between reference and predicted DOAs: three entries Cartesian, two entries spherical in RADIANS;
    the reference's two distance functions."""
    a, b = gt[:, None, :], pr[None, :, :]
    if gt.shape[1] == 3:
        na = np.sqrt(a[..., 0] ** 2 + a[..., 1] ** 2 + a[..., 2] ** 2 + 1e-10)
        nb = np.sqrt(b[..., 0] ** 2 + b[..., 1] ** 2 + b[..., 2] ** 2 + 1e-10)
        d = (a[..., 0] / na) * (b[..., 0] / nb) + (a[..., 1] / na) * (b[..., 1] / nb) + (a[..., 2] / na) * (b[..., 2] / nb)
    else:
        d = np.sin(a[..., 1]) * np.sin(b[..., 1]) + np.cos(a[..., 1]) * np.cos(b[..., 1]) * np.cos(np.abs(a[..., 0] - b[..., 0]))
    return np.arccos(np.clip(d, -1, 1)) * 180 / np.pi


def _maps(g, q):
    """Every pairing of min(g, q) references with predictions as (rows (M, n), cols (M, n)), rows ascending in each."""
    if (g, q) not in _MAPS:
        if g <= q:
            cols = np.array(list(itertools.permutations(range(q), g)), dtype=np.int64).reshape(-1, g)
            rows = np.broadcast_to(np.arange(g), cols.shape)
        else:
            picks = [(rs, cs) for rs in itertools.combinations(range(g), q) for cs in itertools.permutations(range(q))]
            rows = np.array([p[0] for p in picks], dtype=np.int64).reshape(-1, q)
            cols = np.array([p[1] for p in picks], dtype=np.int64).reshape(-1, q)
        _MAPS[(g, q)] = (rows, cols)
    return _MAPS[(g, q)]


def best_assignment(cost):
    """(rows, cols, lead, tie): the cheapest pairing; its lead in degrees over the cheapest pairing that is not within LEAD
    of it (inf when there is none); tie: None when no other pairing is within LEAD, else whether every pairing within LEAD
    gives every reference track the same distance (True: the choice among them cannot be seen in any result)."""
    g, q = cost.shape
    rows, cols = _maps(g, q)
    totals = cost[rows, cols].sum(1)
    order = np.argsort(totals, kind="stable")
    best = order[0]
    near = totals <= totals[best] + LEAD
    far = totals[~near]
    lead = float(far.min() - totals[best]) if far.size else np.inf
    tie = None
    if near.sum() > 1:
        per_track = np.full((int(near.sum()), g), -1.0)
        idx = np.nonzero(near)[0]
        per_track[np.arange(idx.size)[:, None], rows[idx]] = cost[rows[idx], cols[idx]]
        tie = bool((per_track == per_track[0]).all())
    return rows[best].tolist(), cols[best].tolist(), lead, tie


def dcase_counts(pred, true, n_frames, fpb, nb_classes, doa_threshold, info=None):
    """(the ten SELDMetrics counters in DCASE_NAMES order, _total_DE) of one recording; rows of 5 or 4 columns.  `info`
    (a dict) collects: angles (every scored pair's distance), lead (the smallest lead of an association), ties / bad_ties
    (cells whose best pairings tie harmlessly / visibly), gap (the smallest |track average - doa_threshold|), cell (the
    most events of a scored cell)."""
    c = dict.fromkeys(DCASE_NAMES, 0)
    total_de = 0.0
    spherical = pred.shape[1] == 4
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
            if info is not None:
                info["cell"] = max(info.get("cell", 0), nb_gt, nb_pred)
            c["Nref"] += nb_gt
            if gt and pr:
                tracks = {}
                for f in sorted(set(gt) & set(pr)):
                    a, p = (gt[f] * np.pi / 180., pr[f] * np.pi / 180.) if spherical else (gt[f], pr[f])
                    cost = cost_matrix(a, p)
                    rws, cols, lead, tie = best_assignment(cost)
                    if info is not None:
                        info["lead"] = min(info.get("lead", np.inf), lead)
                        info["ties"] = info.get("ties", 0) + (tie is True)
                        info["bad_ties"] = info.get("bad_ties", 0) + (tie is False)
                        info.setdefault("angles", []).extend(float(cost[r_, c_]) for r_, c_ in zip(rws, cols))
                    for r_, c_ in zip(rws, cols):
                        tracks.setdefault(r_, []).append(cost[r_, c_])
                if not tracks:
                    loc_fn += nb_pred
                    c["FN"] += nb_pred
                    c["DE_FN"] += nb_pred
                else:
                    for dists in tracks.values():
                        avg = sum(dists) / len(dists)
                        if info is not None:
                            info["gap"] = min(info.get("gap", np.inf), abs(avg - doa_threshold))
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


def pair_tolerance(angle):
    """Degrees a scored pair's distance may differ between two correct fp64 evaluations.  16 ulp of error in the clipped
    cosine (five transcendental calls and the arithmetic at 1-2 ulp each) carried through acos, whose slope is 1 / sin;
    within a degree of 0 or 180 the cosine may land an ulp on either side of +-1 and acos turns that into sqrt(32 eps)."""
    if 1.0 <= angle <= 179.0:
        return 16 * EPS / np.sin(angle * np.pi / 180) * 180 / np.pi
    return np.sqrt(32 * EPS) * 180 / np.pi


def total_de_tolerance(total_de, angles):
    return max(1e-12 * total_de, sum(pair_tolerance(a) for a in angles))


def score_case(case, info=None):
    dc, de = np.zeros(10, dtype=np.int64), 0.0
    for p, t in zip(case["pred"], case["true"]):
        d, e = dcase_counts(p, t, case["n_frames"], case["fpb"], case["nb_classes"], case["doa_threshold"], info)
        dc += d
        de += e
    return dc.tolist(), de


def check_conditions(case, info):
    """The generator's conditions on a scored case (AssertionError with the figures otherwise)."""
    name = case["name"]
    assert info.get("bad_ties", 0) == 0, (name, "an association ties visibly")
    if case["kind"] == "ties":
        assert info.get("ties", 0) >= 2, (name, "no tie cells")
    else:
        assert info.get("ties", 0) == 0, (name, "an association is not unique", info.get("ties"))
    assert info.get("lead", np.inf) >= LEAD, (name, "lead", info.get("lead"))
    assert info.get("gap", np.inf) >= THRESHOLD_GAP, (name, "threshold gap", info.get("gap"))
    if case["kind"] == "general":
        angles = info.get("angles", [])
        assert angles and min(angles) >= 1.0 and max(angles) <= 179.0, (name, "pair angles", min(angles), max(angles))
    assert info.get("cell", 0) <= case["max_tracks"], (name, "cell", info.get("cell"))
