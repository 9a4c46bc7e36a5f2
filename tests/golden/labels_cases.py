"""Case table of the target encoding and segmentation (csv_to_matrix_task2, segment_task2, segment_waveforms,
utility_functions.py:212-342 of the reference), shared by the fixture generator (make_golden_labels.py, runs against the
reference) and the tests.  Pure data + seeded inputs: the draws are decode_cases.uniform (a counter hash in integer
arithmetic), the label files are text built from them with fixed formats, so every numpy version gives the same bytes."""
import numpy as np

from tests.golden.decode_cases import uniform

# 14 class names of our own; the reference takes any {name: id} dictionary
CLASS_NAMES = [f"sound_{k:02d}" for k in range(14)]
CSV_HEADER = "File,Start,End,Class,X,Y,Z"


def class_dict(names=CLASS_NAMES):
    return {n: i for i, n in enumerate(names)}


def _row(start, end, k, x, y, z, time_fmt="%.3f"):
    return ",".join(["rec", time_fmt % start, time_fmt % end, CLASS_NAMES[k], "%.6f" % x, "%.6f" % y, "%.6f" % z])


def _random_rows(seed, count, dur, classes=14):
    """`count` events: starts uniform in [0, dur - 2), lengths 0.05 .. 6 s, coordinates in (-2, 2)."""
    u = uniform(seed, (count, 6))
    rows = []
    for a in u:
        start = a[0] * (dur - 2.0)
        end = min(start + 0.05 + a[1] * 5.95, dur)
        rows.append(_row(start, end, int(a[2] * classes), *(4.0 * a[3:6] - 2.0)))
    return rows


# kind: how the label file is made (see encode_csv); dur / step / max_loc / no_overlaps: the reference's arguments;
# raises: the exception the reference is expected to raise ("" for none), which the generator checks and records.
ENCODE_CASES = [
    # the challenge's regime: 60 s, 600 frames, 14 x 3 slots, about 60 events
    dict(name="random_60", kind="random", seed=41, count=60, dur=60, step=0.1, max_loc=2.0, no_overlaps=False, raises=""),
    dict(name="random_60_single", kind="random", seed=41, count=60, dur=60, step=0.1, max_loc=2.0, no_overlaps=True, raises=""),
    # a scale that is no power of two: the division rounds, and float32 output rounds once more
    dict(name="maxloc_1p7", kind="random", seed=42, count=40, dur=30, step=0.1, max_loc=1.7, no_overlaps=False, raises=""),
    # three simultaneous events of one class with staggered edges: every slot filled, slot = order in the file
    dict(name="three_same", kind="three_same", seed=43, dur=60, step=0.1, max_loc=2.0, no_overlaps=False, raises=""),
    dict(name="three_same_single", kind="three_same", seed=43, dur=60, step=0.1, max_loc=2.0, no_overlaps=True, raises=""),
    # an event that ends at `dur`, one that covers the whole recording
    dict(name="ends_at_dur", kind="ends_at_dur", seed=44, dur=60, step=0.1, max_loc=2.0, no_overlaps=False, raises=""),
    # starts and ends exactly on .05 ticks: round() is half to even on a quotient that is rarely an exact tie
    dict(name="ticks", kind="ticks", seed=45, dur=60, step=0.1, max_loc=2.0, no_overlaps=False, raises=""),
    # four simultaneous events of one class: the reference raises IndexError
    dict(name="four_same", kind="four_same", seed=46, dur=60, step=0.1, max_loc=2.0, no_overlaps=False, raises="IndexError"),
    dict(name="four_same_single", kind="four_same", seed=46, dur=60, step=0.1, max_loc=2.0, no_overlaps=True, raises="IndexError"),
    # a label file with a header and no event
    dict(name="empty", kind="empty", seed=47, dur=60, step=0.1, max_loc=2.0, no_overlaps=False, raises=""),
    # another frame grid: 20 s at 0.2 s
    dict(name="step_0p2", kind="random", seed=48, count=15, dur=20, step=0.2, max_loc=2.0, no_overlaps=False, raises=""),
]
ENCODE_IDS = [c["name"] for c in ENCODE_CASES]

TICKS = [(0.05, 0.15), (0.25, 0.35), (1.05, 2.45), (2.55, 2.65), (3.15, 3.25), (10.05, 10.95), (20.35, 20.45), (59.85, 59.95),
         (33.349, 33.351), (7.45, 7.55), (0.95, 1.05), (45.65, 47.75)]


def encode_csv(case):
    """The label file of a case as text (str)."""
    kind, seed, dur = case["kind"], case["seed"], case["dur"]
    if kind == "random":
        rows = _random_rows(seed, case["count"], dur)
    elif kind in ("three_same", "four_same"):
        u = 4.0 * uniform(seed, (8, 3)) - 2.0
        rows = [_row(1.0, 3.0, 5, *u[0]), _row(1.5, 2.5, 5, *u[1]), _row(2.0, 4.0, 5, *u[2]),      # class 5: staggered
                _row(2.2, 2.4, 6, *u[3]), _row(0.0, 0.5, 5, *u[4]),                                 # neighbours
                _row(10.0, 12.0, 13, *u[5]), _row(10.0, 12.0, 13, *u[6]), _row(10.0, 12.0, 13, *u[7])]
        if kind == "four_same":
            rows.insert(3, _row(2.1, 2.3, 5, 0.5, -0.5, 0.25))
    elif kind == "ends_at_dur":
        u = 4.0 * uniform(seed, (3, 3)) - 2.0
        rows = [_row(55.0, 60.0, 0, *u[0]), _row(0.0, 60.0, 3, *u[1]), _row(59.95, 60.0, 13, *u[2])]
    elif kind == "ticks":
        u = 4.0 * uniform(seed, (len(TICKS), 3)) - 2.0
        rows = [_row(a, b, (3 * i) % 14, *u[i], time_fmt="%.3f" if i != 8 else "%.4f") for i, (a, b) in enumerate(TICKS)]
    elif kind == "empty":
        rows = []
    else:
        raise KeyError(kind)
    return "\n".join([CSV_HEADER] + rows) + "\n"


def ramp(shape, dtype, start=1.0):
    """Distinct, exactly representable values 1, 2, 3, ... in row-major order (no zero: padding stays recognisable)."""
    return (np.arange(int(np.prod(shape)), dtype=np.float64) + start).reshape(shape).astype(dtype)


# fn: the reference function; predictors / target: shapes; the rest: its arguments.  raises: what the reference is expected to
# do ("" = returns); ragged: the reference returns target chunks of different lengths, which this package refuses.
SEGMENT_CASES = [
    dict(name="task2_4800", fn="segment_task2", predictors=(2, 3, 4800), target=(600, 168), p_dtype="float32",
         t_dtype="float32", kw=dict(), raises="", ragged=False),
    dict(name="task2_1237", fn="segment_task2", predictors=(2, 3, 1237), target=(155, 168), p_dtype="float64",
         t_dtype="float64", kw=dict(), raises="", ragged=False),
    dict(name="task2_1237_f32", fn="segment_task2", predictors=(2, 3, 1237), target=(155, 20), p_dtype="float32",
         t_dtype="float64", kw=dict(), raises="", ragged=False),
    dict(name="task2_counts_differ", fn="segment_task2", predictors=(2, 3, 1000), target=(600, 8), p_dtype="float32",
         t_dtype="float32", kw=dict(), raises="ValueError", ragged=False),
    dict(name="task2_overlap_1", fn="segment_task2", predictors=(2, 3, 1100), target=(140, 12), p_dtype="float32",
         t_dtype="float32", kw=dict(overlap=1.0), raises="", ragged=False),
    dict(name="task2_other_lengths", fn="segment_task2", predictors=(1, 5, 333), target=(84, 7), p_dtype="float64",
         t_dtype="float32", kw=dict(predictors_len_segment=64, target_len_segment=16, overlap=0.25), raises="", ragged=False),
    dict(name="task2_ragged_target", fn="segment_task2", predictors=(1, 1, 800), target=(90, 4), p_dtype="float32",
         t_dtype="float32", kw=dict(), raises="", ragged=True),
    dict(name="waves_divides", fn="segment_waveforms", predictors=(4, 1000), target=(2, 1000), p_dtype="float32",
         t_dtype="float32", kw=dict(length=250), raises="", ragged=False),
    dict(name="waves_ragged_tail", fn="segment_waveforms", predictors=(4, 1000), target=(4, 1000), p_dtype="float32",
         t_dtype="float64", kw=dict(length=300), raises="", ragged=False),
    dict(name="waves_odd", fn="segment_waveforms", predictors=(3, 1001), target=(1, 1001), p_dtype="float64",
         t_dtype="float32", kw=dict(length=77), raises="", ragged=False),
]
SEGMENT_IDS = [c["name"] for c in SEGMENT_CASES]


def segment_inputs(case):
    """(predictors, target) of a case as numpy arrays; the target's values continue after the predictors'."""
    p = ramp(case["predictors"], case["p_dtype"])
    t = ramp(case["target"], case["t_dtype"], start=0.5)
    return p, t
