"""The numpy statement of track post-processing (include/seld_hip.h, "Track post-processing"): the rules of
seld_smooth_tracks and the event list of seld_track_events_*, written with plain loops over columns and runs, sums in
float64; the error bound of the run DOAs; and the planted and random cases of tests/test_smooth_host.py and
tests/test_gpu_smooth.py.  Clarity over speed."""
import functools

import numpy as np

MAX_MEDIAN = 31
MAX_FRAMES = 16384
DOA_MODES = ("frame", "mean", "weighted")
IDENTITY = dict(median=1, on=0.5, off=0.5, min_frames=1, max_gap=0)


def runs_of(flag):
    """[(start, end, value)] of the maximal runs of a 1-D boolean array, end exclusive, in order."""
    flag = np.asarray(flag, dtype=bool)
    cuts = np.flatnonzero(flag[1:] != flag[:-1]) + 1
    starts = np.concatenate(([0], cuts))
    ends = np.concatenate((cuts, [flag.shape[0]]))
    return [(int(s), int(e), bool(flag[s])) for s, e in zip(starts, ends)]


def median_column(x, median):
    """Median over frames t - h .. t + h of a 1-D array, indices clamped to the array: an element of the window."""
    h = (median - 1) // 2
    T = x.shape[0]
    frames = np.clip(np.arange(T)[:, None] + np.arange(-h, h + 1)[None, :], 0, T - 1)      # (T, median): row t is t's window
    return np.sort(x[frames], axis=1)[:, h]


def bound(ref, run_len, peak):
    """|out - ref| allowed for a run's DOA: each of the two double sums is within run_len * 2^-53 of exact, relatively
    (non-negative weights, any order), on the kernel's side and on this reference's; then one division and one rounding
    to fp32."""
    return 2.0 ** -24 * np.abs(ref) + 4.0 * run_len * 2.0 ** -53 * peak


def event_bound(ref, run_len, peak, max_loc_value):
    """|x - ref| allowed for a coordinate of seld_track_events_write: the double sum, one division and one multiply."""
    return 4.0 * run_len * 2.0 ** -53 * peak * abs(max_loc_value) + 2.0 ** -52 * np.abs(ref)


def smooth(sed, doa, *, median=1, on=0.5, off=0.5, min_frames=1, max_gap=0, doa_mode="frame"):
    """dict(prob, sed, doa (float64: the unrounded run DOAs, the input elsewhere), runs, filled, short, kept, dropped).

    sed (R, T, n), doa (R, T, 3n) float32.  runs: [(r, j, start, end, peak)] of the surviving events in row order, peak
    the largest |d| among the run's DOAs.  Counters, from these rules alone: `filled` gaps, runs dropped for being
    `short`, runs of p > off `kept` and `dropped` by the `on` rule.  `on` and `off` are compared in fp32 as the kernel
    takes them."""
    sed, doa = np.asarray(sed, np.float32), np.asarray(doa, np.float32)
    R, T, n = sed.shape
    assert doa.shape == (R, T, 3 * n) and median % 2 == 1 and 1 <= median <= MAX_MEDIAN and doa_mode in DOA_MODES
    on32, off32 = np.float32(on), np.float32(off)
    prob = np.empty_like(sed)
    out_sed = np.zeros_like(sed)
    out_doa = doa.astype(np.float64)
    runs, filled, short, kept, dropped = [], 0, 0, 0, 0
    for r in range(R):
        for j in range(n):
            p = sed[r, :, j] if median == 1 else median_column(sed[r, :, j], median)
            prob[r, :, j] = p
            a = np.zeros(T, dtype=bool)
            for s, e, v in runs_of(p > off32):                      # 2. hysteresis
                if v and (p[s:e] > on32).any():
                    a[s:e] = True
                    kept += 1
                elif v:
                    dropped += 1
            for s, e, v in runs_of(a):                              # 3. gap fill (on a1: the list is taken first)
                if not v and s > 0 and e < T and e - s <= max_gap:
                    a[s:e] = True
                    filled += 1
            for s, e, v in runs_of(a):                              # 4. minimum duration
                if v and e - s < min_frames:
                    a[s:e] = False
                    short += 1
            out_sed[r, :, j] = a
            for s, e, v in runs_of(a):
                if not v:
                    continue
                d = doa[r, s:e, 3 * j:3 * j + 3].astype(np.float64)
                runs.append((r, j, s, e, float(np.abs(d).max())))
                if doa_mode != "frame":
                    w = np.ones(e - s) if doa_mode == "mean" else p[s:e].astype(np.float64)
                    out_doa[r, s:e, 3 * j:3 * j + 3] = (w[:, None] * d).sum(0) / w.sum()
    return dict(prob=prob, sed=out_sed, doa=out_doa, runs=runs, filled=filled, short=short, kept=kept, dropped=dropped)


def events(sed, doa, max_loc_value=2., overlaps=3):
    """(rows (E, 8) float64, rec_offsets (R + 1) int64, [(run length, peak)] per row): every maximal run of sed > 0.5 of
    a column as {recording, class, slot, onset, offset, x, y, z}, recording-major, then column, then onset."""
    sed, doa = np.asarray(sed, np.float32), np.asarray(doa, np.float32)
    R, T, n = sed.shape
    rows, offsets, info = [], [0], []
    for r in range(R):
        for j in range(n):
            for s, e, v in runs_of(sed[r, :, j] > np.float32(0.5)):
                if v:
                    d = doa[r, s:e, 3 * j:3 * j + 3].astype(np.float64)
                    rows.append([r, j // overlaps, j % overlaps, s, e] + list(d.sum(0) / (e - s) * max_loc_value))
                    info.append((e - s, float(np.abs(d).max())))
        offsets.append(len(rows))
    return np.asarray(rows, np.float64).reshape(-1, 8), np.asarray(offsets, np.int64), info


# ---- planted cases: one per rule, small enough to read -------------------------------------------------------------------
LEVELS = {".": 0.1, "a": 0.25, "q": 0.25, "o": 0.5, "m": 0.6, "b": 0.75, "Q": 0.75, "X": 0.9}


def _columns(*texts):
    """(1, T, n) float32 of n strings over LEVELS, one per column."""
    return np.stack([np.array([LEVELS[c] for c in text], np.float32) for text in texts], axis=1)[None]


def _bits(*texts):
    return np.stack([np.array([c == "1" for c in text], np.float32) for text in texts], axis=1)[None]


def _ramp_doa(T, n):
    """doa[0, t, 3j + a] = t + 10 j + 100 a: exact in fp32, and so is every mean of consecutive frames used below."""
    t, j, a = np.arange(T)[:, None, None], np.arange(n)[None, :, None], np.arange(3)[None, None, :]
    return (t + 10 * j + 100 * a).astype(np.float32).reshape(1, T, 3 * n)


def planted_cases():
    """[dict(name, sed, doa, params, want_sed, want_prob or None, want_doa or None)]: every expected output is literal."""
    cases = []

    def add(name, texts, want, want_doa=None, want_prob=None, doa=None, **params):
        sed = _columns(*texts)
        T, n = sed.shape[1:]
        assert 12 <= T <= 20 and 1 <= n <= 3 and all(len(w) == T for w in want)
        cases.append(dict(name=name, sed=sed, doa=_ramp_doa(T, n) if doa is None else doa, params=dict(IDENTITY, **params),
                          want_sed=_bits(*want), want_prob=want_prob, want_doa=want_doa))

    # a dip of max_gap frames is filled, one of max_gap + 1 is not; the gaps at either end are never filled
    add("gap_fill", ["..XX..XX...XX."],
        ["..111111...11."], max_gap=2)
    add("gap_at_the_ends", [".XX.....XX.."],
        [".111111111.."], max_gap=5)
    # runs of min_frames - 1 go, at a recording's ends as anywhere else; a run of min_frames stays
    add("min_frames", ["XX..XXX...XX"],
        ["....111....."], min_frames=3)
    add("runs_touching_the_ends", ["XX....XX...XX"],
        ["11....11...11"], min_frames=2)
    # a run between off and on is kept, whole, iff one frame is above on
    add("hysteresis", ["..mmm..mXm..mm"],
        [".......111...."], on=0.8, off=0.4)
    # the gap is filled before the duration is taken: two runs of 2 joined over a gap of 1 survive min_frames = 4
    add("fill_then_duration", ["..XX.XX....."],
        ["..11111....."], min_frames=4, max_gap=1)
    add("duration_without_fill", ["..XX.XX....."],
        ["............"], min_frames=4)
    # strict comparisons: b = 0.75 is not above on = 0.75 (but above off), a = 0.25 is not above off = 0.25
    add("at_the_thresholds", ["..bbb..aXa..obX."],
        ["........1...111."], on=0.75, off=0.25)
    # median of 3: a spike goes, a dip is bridged
    add("median_3", ["..X..XX.XX.."],
        [".....11111.."], median=3,
        want_prob=_columns(".....XXXXX.."))
    # a window wider than the recording: frame 0 and frame 11 are replicated 16 - t and t + 5 times among 31 values, the
    # ten frames between count once: 21 values of 0.9 against 10 of 0.1 at every frame
    add("median_wider_than_T", ["X..........X"],
        ["111111111111"], median=31, want_prob=_columns("XXXXXXXXXXXX"))
    # one DOA per event: the mean of t + 10 j + 100 a over the event's frames; column 1 is silent; other frames copy
    T = 12
    doa = _ramp_doa(T, 3)
    want = doa.astype(np.float64).copy()
    for j, s, e in ((0, 2, 6), (2, 0, 2), (2, 10, 12)):
        want[0, s:e, 3 * j:3 * j + 3] = (s + e - 1) / 2 + 10 * j + 100 * np.arange(3)
    add("mean_doa", ["..XXXX......", "............", "XX........XX"],
        ["..1111......", "............", "11........11"], want_doa=("mean", want))
    # weighted by the activity: p = 0.25 and 0.75 over d = (0, 1, -2) and (4, 1, 2) give (3, 1, 1)
    doa = np.full((1, T, 3), 7.0, np.float32)
    doa[0, 4], doa[0, 5] = (0, 1, -2), (4, 1, 2)
    want = doa.astype(np.float64).copy()
    want[0, 4:6] = (3, 1, 1)
    add("weighted_doa", ["....qQ......"],
        ["....11......"], want_doa=("weighted", want), doa=doa, on=0.125, off=0.125)
    return cases


# ---- random cases --------------------------------------------------------------------------------------------------------
RANDOM_R = (1, 3)
RANDOM_N = (1, 3, 42, 64)
# 769: the first T at which a thread of the kernel's 256 takes 5 consecutive frames instead of 3 (257: 3 instead of 1)
RANDOM_T = (1, 2, 5, 63, 64, 65, 255, 257, 600, 769, 1025)
MEDIANS = (1, 3, 7, 31)


def settings_for(T):
    """The settings of the other four parameters the random cases cycle through at T frames."""
    return (dict(on=0.5, off=0.5, min_frames=1, max_gap=0),                 # off = on
            dict(on=0.75, off=0.25, min_frames=3, max_gap=2),
            dict(on=0.5, off=0.0, min_frames=2, max_gap=1),                 # off = 0
            dict(on=0.625, off=0.375, min_frames=1, max_gap=T + 5),         # max_gap >= T
            dict(on=0.5625, off=0.4375, min_frames=T + 1, max_gap=1),       # min_frames > T
            dict(on=0.6875, off=0.4375, min_frames=4, max_gap=3))


def random_track(R, T, n, seed):
    """sed: a smoothed mean-reverting random walk around 0.5 plus a little noise, quantised to multiples of 1/16 in [0, 1] (ties and at-threshold values
    occur, runs of many lengths occur); doa uniform in (-1, 1).  numpy's PCG64 streams are stable across versions."""
    rng = np.random.default_rng(seed)
    steps = rng.normal(0.0, 0.08, (R, T + 3, n))
    walk = np.empty_like(steps)
    level = rng.normal(0.0, 0.3, (R, n))
    for t in range(T + 3):                                      # mean-reverting: it stays around 0.5 at any T
        level = 0.96 * level + steps[:, t]
        walk[:, t] = level
    smooth_walk = sum(walk[:, k:k + T] for k in range(4)) / 4 + rng.normal(0.0, 0.05, (R, T, n))
    sed = np.clip(np.rint((0.5 + smooth_walk) * 16) / 16, 0.0, 1.0).astype(np.float32)
    doa = rng.uniform(-1.0, 1.0, (R, T, 3 * n)).astype(np.float32)
    return sed, doa


def random_specs(T):
    """[dict(shape, seed, params, doa_mode)] at T frames: every (R, n), the medians, settings and DOA modes taken in turn
    so that each occurs with each shape class over the list."""
    specs = []
    settings = settings_for(T)
    k = RANDOM_T.index(T) if T in RANDOM_T else len(RANDOM_T)
    for R in RANDOM_R:
        for n in RANDOM_N:
            specs.append(dict(shape=(R, T, n), seed=1000 * T + 10 * n + R,
                              params=dict(settings[k % len(settings)], median=MEDIANS[(k // 2 + k) % len(MEDIANS)]),
                              doa_mode=DOA_MODES[1 + k % 2]))
            k += 1
    return specs


def longest_spec():
    return dict(shape=(1, MAX_FRAMES, 3), seed=7, params=dict(on=0.75, off=0.25, min_frames=60, max_gap=40, median=31),
                doa_mode="weighted")


@functools.lru_cache(maxsize=None)
def _random_case(shape, seed, params, doa_mode):
    sed, doa = random_track(*shape, seed)
    return dict(shape=shape, sed=sed, doa=doa, params=dict(params), doa_mode=doa_mode,
                ref=smooth(sed, doa, doa_mode=doa_mode, **dict(params)))


def random_case(spec):
    """The spec's track and its reference (computed once per process, shared, not to be written to)."""
    return _random_case(spec["shape"], spec["seed"], tuple(sorted(spec["params"].items())), spec["doa_mode"])
