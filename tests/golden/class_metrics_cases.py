"""Cases of the breakdown by recording and class (hip_ops.score_events_by / metrics_accumulate_by) beyond the two existing
case tables, which the fixture generator (make_golden_class_metrics.py) and the tests run over as well.  Pure data + seeded
inputs.  A case is a dict in the form of event_metrics_ex_cases: name, coords, max_tracks, n_frames, fpb, nb_classes,
doa_threshold, spatial_threshold, lsd, and `pred` / `true`, one (E, 5) float64 array per recording.

The smallest inputs at which the breakdown can go wrong: several recordings (slab indexing), among them an empty one, one
with classes outside [0, C) on both sides (row "other"), one with a negative class FP, and one with a block in which class A
has only a missed reference and class B only a false prediction -- there the class-wise S, D, I (D_A = 1, I_B = 1) and the
cross-class ones of row "all" (S = 1) differ; the same lists in reverse order; no class at all; 64 classes."""
import numpy as np

from tests.golden.event_metrics_cases import CASE_IDS, E0, EVENT_METRIC_CASES, _events, _near, _overlap_block, _xyz
from tests.golden.event_metrics_ex_cases import EVENT_METRIC_EX_CASES

SUB_A, SUB_B = 2, 7          # the classes of the substitution block of recording 3 (frames 10 .. 19)


def _case(name, pred, true, n_frames=30, nb_classes=14):
    return dict(name=name, kind="general", coords=3, max_tracks=3, pred=pred, true=true, n_frames=n_frames, fpb=10,
                nb_classes=nb_classes, doa_threshold=20.0, spatial_threshold=2.0, lsd=True)


def _five():
    """(pred, true) of five recordings of 30 frames."""
    # 1: classes 14 and 20 beside 3 and 13, on both sides
    P1, T1 = _overlap_block(140, [1, 12, 27], [[(1, 1), (1, 1), (2, 1), (1, 2)]], 30, cls_of=lambda k: (3, 14, 20, 13)[k])
    # 2: c_negative_fp's configuration: two references of one class near one prediction
    ref = _xyz(3, 1)
    P2 = _events([5], [6], ref)
    T2 = _events([5, 5], [6, 6], np.concatenate((_near(ref, 4, 0.1), _near(ref, 5, 0.1))))
    # 3: block 1 holds a missed reference of class A and a false prediction of class B, nothing else; blocks 0 and 2 a match
    near = _xyz(150, 2)
    P3 = np.concatenate((_events([4], [1], near[:1]), _events([13], [SUB_B], _xyz(151, 1)), _events([25], [9], near[1:])))
    T3 = np.concatenate((_events([4], [1], _near(near[:1], 152, 0.05)), _events([12], [SUB_A], _xyz(153, 1)),
                         _events([25], [9], _near(near[1:], 154, 0.05))))
    # 4: overlapping tracks over two blocks
    P4, T4 = _overlap_block(160, [0, 3, 9, 10, 11, 29], [[(1, 1), (2, 1)], [(1, 2), (2, 2)], [(3, 3), (0, 1), (1, 0)]], 30,
                            spread=0.4)
    return [E0, P1, P2, P3, P4], [E0, T1, T2, T3, T4]


def build_cases():
    P, T = _five()
    cases = [_case("by_five", P, T), _case("by_five_reversed", P[::-1], T[::-1]),
             _case("by_no_class", P[1:4], T[1:4], nb_classes=0)]
    # 64 classes: events in classes 0, 31, 62, 63 and, outside, 64
    P64, T64 = _overlap_block(170, [2, 15, 16, 28], [[(1, 1), (2, 1), (1, 2), (2, 2), (1, 1)]], 30,
                              cls_of=lambda k: (0, 31, 62, 63, 64)[k], spread=0.4)
    cases.append(_case("by_64_classes", [P64, E0], [T64, E0], nb_classes=64))
    return cases


CLASS_METRIC_CASES = build_cases()


def _as_ex(c):
    return dict(c, kind="general", coords=3, max_tracks=3)


# every case the fixture holds: the two existing tables (in the ex form), then the new cases
ALL_CASES = [_as_ex(c) for c in EVENT_METRIC_CASES] + [dict(c, lsd=True) for c in EVENT_METRIC_EX_CASES] + CLASS_METRIC_CASES
ALL_IDS = [c["name"] for c in ALL_CASES]
assert len(set(ALL_IDS)) == len(ALL_IDS) and CASE_IDS[0] in ALL_IDS


def refused_lists():
    """(pred, true) of one recording whose frame 3 holds four predictions of class 2: refused under max_tracks = 3."""
    four = _events([3, 3, 3, 3, 7], [2, 2, 2, 2, 5], _xyz(180, 5))
    return [four], [_events([3, 7], [2, 5], _xyz(181, 2))]
