"""Case table of the event decoding (gen_submission_list_task2 / gen_submission_list_task2_OLD, utility_functions.py:158-210
of the reference), shared by the fixture generator (make_golden_decode.py, runs against the reference) and the tests.
Pure data + seeded inputs: the draws are a counter hash (splitmix64) in integer arithmetic, so every numpy version gives
the same arrays."""
import numpy as np

_M64 = (1 << 64) - 1


def uniform(seed, shape):
    """float64 uniforms in [0, 1) with 24 random bits each (exact in float32), a pure function of (seed, position)."""
    count = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0xD1B54A32D192ED03) & _M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) / float(1 << 24)).reshape(shape)


# kind: how `sed` is made (see decode_inputs); T frames; classes x overlaps slots; dtype of both inputs; max_loc_value.
# "active" is the fraction of slots switched on where the kind takes one.
DECODE_CASES = [
    # the network's regime: sigmoid outputs at the 14 x 3 layout and the full 600 frames
    dict(name="sigmoid_600", kind="sigmoid", T=600, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=11, active=0.03),
    dict(name="sparse_600", kind="sigmoid", T=600, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=12, active=0.01),
    dict(name="dense_21", kind="dense", T=21, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=13),
    # exact ties (half to even) and their float32 neighbours
    dict(name="ties", kind="ties", T=9, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=14),
    dict(name="ties_f64", kind="ties", T=9, classes=14, overlaps=3, dtype="float64", max_loc=2.0, seed=14),
    # negative activities; frames whose rounded values cancel to zero are dropped
    dict(name="negatives", kind="negatives", T=12, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=15),
    # all-zero frames at the start, in the middle (across a 64-frame boundary) and at the end
    dict(name="zero_frames", kind="zero_frames", T=150, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=16, active=0.06),
    # no event at all: the reference returns np.array([]), shape (0,)
    dict(name="no_events", kind="none", T=20, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=17),
    # a scale that is not a power of two pins where the multiply is rounded
    dict(name="maxloc_1p7", kind="sigmoid", T=50, classes=14, overlaps=3, dtype="float32", max_loc=1.7, seed=18, active=0.1),
    dict(name="float64_1p7", kind="sigmoid", T=50, classes=14, overlaps=3, dtype="float64", max_loc=1.7, seed=18, active=0.1),
    # other layouts: one event per class; 64 slots, the widest supported
    dict(name="c5_o1", kind="sigmoid", T=33, classes=5, overlaps=1, dtype="float32", max_loc=2.0, seed=19, active=0.3),
    dict(name="c16_o4", kind="sigmoid", T=130, classes=16, overlaps=4, dtype="float32", max_loc=2.0, seed=20, active=0.08),
    dict(name="c16_o4_dense", kind="dense", T=3, classes=16, overlaps=4, dtype="float64", max_loc=0.3, seed=21),
    # lengths: one frame; a length that is no multiple of 8 or 64 and crosses four 64-frame boundaries
    dict(name="one_frame", kind="dense", T=1, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=22),
    dict(name="frames_257", kind="sigmoid", T=257, classes=14, overlaps=3, dtype="float32", max_loc=2.0, seed=23, active=0.05),
]
CASE_IDS = [c["name"] for c in DECODE_CASES]

TIE_VALUES = [0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997, 0.50000006, 1.4999999, 1.5000001, -0.50000006, 3.5, 0.0]


def decode_inputs(case):
    """(sed (T, n), doa (T, 3n)) of a case as numpy arrays of the case's dtype."""
    T, n = case["T"], case["classes"] * case["overlaps"]
    dt = np.dtype(case["dtype"])
    u = uniform(case["seed"], (T, n))
    doa = (2.0 * uniform(case["seed"] + 1000, (T, 3 * n)) - 1.0).astype(dt)
    kind = case["kind"]
    if kind == "sigmoid":                       # a fraction `active` of the slots above 0.5, all values inside (0, 1)
        a = case["active"]
        sed = np.where(u < a, 0.5 + 0.5 * (u / a) * 0.999 + 0.0005, 0.5 * (u - a) / (1.0 - a) * 0.999)
    elif kind == "dense":                       # every slot on, also through 1.5 .. 2.49 -> 2
        sed = 0.51 + 1.9 * u
    elif kind == "none":                        # everything at or below one half, which rounds to even = 0
        sed = 0.5 * u
        sed[3, 5] = 0.5
        sed[7, 0] = -0.5
    elif kind == "ties":                        # frame f, slot j: the tie values in turn; frame 8 holds 0.5 / -0.5 only
        idx = (np.arange(T)[:, None] * 5 + np.arange(n)[None, :]) % len(TIE_VALUES)
        sed = np.asarray(TIE_VALUES, dtype=np.float64)[idx]
        sed[8] = np.where(np.arange(n) % 2 == 0, 0.5, -0.5)
    elif kind == "negatives":
        sed = 0.4 * u                           # off
        sed[0, 4], sed[0, 9] = -1.0, 1.0        # cancels to zero: the frame is dropped although two slots are on
        sed[1, 4], sed[1, 9], sed[1, 20] = -1.0, 1.0, 0.7            # sums to 1: three rows
        sed[2, 0] = -0.6                        # rounds to -1: on
        sed[3, 7], sed[3, 8] = -2.4, 1.6        # -2 + 2 = 0: dropped
        sed[4, 41], sed[4, 0] = -0.8, -0.9      # -2: two rows
        sed[5, 1], sed[5, 2], sed[5, 3] = 1.2, 0.8, -2.5             # 1 + 1 - 2 = 0: dropped
        sed[6, 1], sed[6, 2], sed[6, 3] = 1.2, 0.8, -3.5             # 1 + 1 - 4 = -2: three rows
        sed[8, 13] = 2.5                        # rounds to 2: on
        sed[9, 13], sed[9, 14] = -0.5, -0.4     # both round to -0: off
        sed[11, 40], sed[11, 41] = 3.0, -3.0    # dropped, last frame
    elif kind == "zero_frames":
        a = case["active"]
        sed = np.where(u < a, 0.75, 0.25 * u)
        for lo, hi in ((0, 3), (60, 70), (127, 129), (T - 4, T)):
            sed[lo:hi] = 0.0
        sed[3, 0] = sed[59, 41] = sed[70, 1] = sed[T - 5, 20] = 0.9          # the zero runs' neighbours hold events
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(sed.astype(dt)), np.ascontiguousarray(doa)
