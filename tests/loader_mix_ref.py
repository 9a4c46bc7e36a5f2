"""Host reference of the gather that mixes two clips, seld_gather_rows_mix, and of seld_target_occupancy, written from the
text of include/seld_hip.h over tests/loader_rot_ref.py and tests/loader_polar_ref.py (the Philox words, the masks and the
comparison on the complex value are theirs).  numpy only: no torch, no GPU.

The stored fp32 values are taken as exact.  In float64, per pair (magnitude channel c, phase channel c + C / 2) and (f, t),
for the sample A and its partner B with the gain g:

    m_S = x_S[m] * sd_m + mean_m      phi_S = x_S[p] * sd_p + mean_p      z_S = m_S e^(i phi_S)        S = A, B
    z' = z_A + g z_B

The kernel writes magnitude and phase of z', standardised again.  As in the polar reference `gather_mix` returns the
COMPLEX value z' (at the positions of both channels of the pair) and the tests compare on it; with it the weight

    Wt = ((|m_A| + |mean_m|) + g (|m_B| + |mean_m|)) * (1 + pi + |mean_p|)

that the error bound K * 2^-24 * Wt + TINY of tests/test_gpu_loader_mix.py scales with, and `exact`: True where the kernel
only moves bits or writes `fill` (there `ref` holds the float32 value).  `mix_x_f32` restates the kernel with every
operation rounded to fp32; its distance from the float64 reference over the inputs of the GPU tests, measured on the CPU
(`measured_cpu_ratio`), sets K.  The merged targets (`merge_targets`) and the occupancy table (`occupancy`) are exact."""
import functools

import numpy as np

from tests import philox_ref as PH
from tests.loader_aug_ref import int_below
from tests.loader_polar_ref import CASES, NO_STATS, STATS, _fma, _stats64      # noqa: F401  (CASES, STATS: the GPU tests' shapes)
from tests.loader_rot_ref import TINY, U24, _masks, bits_equal, words          # noqa: F401

f32 = np.float32
MIX_KEY = 0x9E3779B97F4A7C15
# the error bound of the GPU tests: 4 times the largest ratio `measured_cpu_ratio` finds, rounded up to a power of two
# (tests/test_loader_mix_host.py asserts that this is so); the margin is for the device's sincosf and atan2f
K = 8
T_OUT = 3                                               # frames of a target row in the GPU tests


# ---- the draw ---------------------------------------------------------------------------------------------------------------
def mix_draw(seed, epoch, p, n_index, p_mix, gain_lo, gain_hi):
    """(partner position or -1, gain as fp32) of the sample at position p: the words of group 0 under the key
    seed ^ MIX_KEY."""
    if not (p_mix > 0 and n_index > 1):
        return -1, f32(0)
    w = words((int(seed) ^ MIX_KEY) & PH.MASK64, epoch, p, 0)
    if not bool(PH.u01(np.uint32(w[1])) < f32(p_mix)):
        return -1, f32(0)
    p2 = (p + 1 + int_below(w[0], n_index - 1)) % n_index
    g = _fma(PH.u01(np.uint32(w[2])), f32(f32(gain_hi) - f32(gain_lo)), f32(gain_lo))
    return p2, f32(g)


# ---- targets ------------------------------------------------------------------------------------------------------------------
def active(y, overlaps):
    """bool (..., classes, overlaps): activity > 0.5 in fp32 (a NaN is inactive) of targets (..., 4 * classes * overlaps)."""
    n_sed = y.shape[-1] // 4
    with np.errstate(invalid="ignore"):
        return (np.asarray(y, dtype=f32)[..., :n_sed] > f32(0.5)).reshape(y.shape[:-1] + (n_sed // overlaps, overlaps))


def occupancy(y_all, overlaps):
    """uint8 (n, classes): the largest number of active slots of a class in one frame of a row."""
    a = active(np.asarray(y_all).reshape(y_all.shape[0], -1, y_all.shape[-1]), overlaps)
    return a.sum(-1).max(1).astype(np.uint8)


def merge_targets(ya, yb, overlaps):
    """The targets of a mixed sample from those of A and B (T_out, 4 * n_sed): per (frame, class) A's active slots in slot
    order, then B's; the first `overlaps` entries fill the class's slots (activity and location as bits), the slots
    behind the list are +0."""
    ya, yb = np.asarray(ya, dtype=f32), np.asarray(yb, dtype=f32)
    n_sed = ya.shape[-1] // 4
    out = np.zeros_like(ya)
    aa, ab = active(ya, overlaps), active(yb, overlaps)
    for fr in range(ya.shape[0]):
        for c in range(n_sed // overlaps):
            entries = [(ya, c * overlaps + o) for o in range(overlaps) if aa[fr, c, o]]
            entries += [(yb, c * overlaps + o) for o in range(overlaps) if ab[fr, c, o]]
            for k, (src, s) in enumerate(entries[:overlaps]):
                d = c * overlaps + k
                out[fr, d] = src[fr, s]
                out[fr, n_sed + 3 * d:n_sed + 3 * d + 3] = src[fr, n_sed + 3 * s:n_sed + 3 * s + 3]
    return out


def fits(occ, r, r2, overlaps):
    """The occupancy test of the kernel: no class holds more events in the two clips than it has slots."""
    return bool((occ[r].astype(int) + occ[r2].astype(int) <= overlaps).all())


# ---- predictors ---------------------------------------------------------------------------------------------------------------
def polar64(x, stats):
    """(M, P): float64 magnitude and phase (C / 2, ...) of stored predictors (C, ...)."""
    mean_m, sd_m, mean_p, sd_p = _stats64(stats)
    x64 = np.asarray(x, dtype=np.float64)
    h = x64.shape[0] // 2
    return x64[:h] * sd_m + mean_m, x64[h:] * sd_p + mean_p


def mix_x(xa, xb, g, stats=None):
    """(ref float64 (NaN: compare on z), z complex128, weight, exact) of A (C, F, T) mixed with g times B: every channel
    takes part."""
    mean_m, _, mean_p, _ = _stats64(stats)
    g = float(f32(g))
    Ma, Pa = polar64(xa, stats)
    Mb, Pb = polar64(xb, stats)
    z = Ma * np.exp(1j * Pa) + g * (Mb * np.exp(1j * Pb))
    wt = ((np.abs(Ma) + abs(mean_m)) + g * (np.abs(Mb) + abs(mean_m))) * (1 + np.pi + abs(mean_p))
    shape = np.asarray(xa).shape
    return np.full(shape, np.nan), np.concatenate([z, z]), np.concatenate([wt, wt]), np.zeros(shape, dtype=bool)


def mix_x_f32(xa, xb, g, stats=None):
    """What the kernel stores for a mixed sample, every operation of include/seld_hip.h rounded to fp32 (numpy's fp32 sin,
    cos, arctan2 and sqrt in place of the device's): float32 (C, F, T)."""
    xa, xb, g = np.asarray(xa, dtype=f32), np.asarray(xb, dtype=f32), f32(g)
    h = xa.shape[0] // 2
    mean_m, sd_m, mean_p, sd_p = (f32(v) for v in (NO_STATS if stats is None else stats))
    re, im = [], []
    for x in (xa, xb):
        m, phi = x[:h], x[h:]
        if stats is not None:
            m, phi = _fma(m, sd_m, mean_m), _fma(phi, sd_p, mean_p)
        re.append((m * np.cos(phi).astype(f32)).astype(f32))
        im.append((m * np.sin(phi).astype(f32)).astype(f32))
    r, i = _fma(g, re[1], re[0]), _fma(g, im[1], im[0])
    mag = np.sqrt(_fma(i, i, (r * r).astype(f32))).astype(f32)
    phi = np.arctan2(i, r).astype(f32)
    if stats is not None:
        mag, phi = ((mag - mean_m).astype(f32) / sd_m).astype(f32), ((phi - mean_p).astype(f32) / sd_p).astype(f32)
    return np.concatenate([mag, phi]).astype(f32)


def complex_of(out, stats):
    """The complex value a stored output (..., C, F, T) holds, at both channels of every pair, from its destandardised
    magnitude and phase in float64: (z, M, P) laid out like `out`."""
    mean_m, sd_m, mean_p, sd_p = _stats64(stats)
    o64 = np.asarray(out, dtype=np.float64)
    h = o64.shape[-3] // 2
    M, P = o64[..., :h, :, :] * sd_m + mean_m, o64[..., h:, :, :] * sd_p + mean_p
    z = M * np.exp(1j * P)
    return np.concatenate([z, z], -3), np.concatenate([M, M], -3), np.concatenate([P, P], -3)


def gather_mix(x_all, y_all, index, first, count, out_x, out_y, *, seed, epoch, overlaps, stats=None, p_mix=0.0, mix_gain=(0.5, 1.0),
               partners=None, gains=None, occ=None, n_fmask=0, f_max=0, n_tmask=0, t_max=0, fill=0.0, restate=False):
    """What the call leaves in copies of the batch buffers: dict(rows=, x=dict(ref, z, weight, exact[, f32]), y=float32).
    rows[b]: None for an invalid row, else dict(p2 (the partner position or -1), g, r2 (the partner's row, -1 when it is
    invalid or nothing was drawn), refused (drawn with a valid partner, not mixed for occupancy), mixed).  `restate`: x
    also gets `f32`, the fp32 restatement of the whole batch.  Rows >= count keep what the buffers held."""
    out = {}
    if out_x is not None:
        ref = np.array(out_x, dtype=f32).astype(np.float64)
        out["x"] = dict(ref=ref, z=np.zeros(ref.shape, dtype=np.complex128), weight=np.zeros_like(ref), exact=np.ones(ref.shape, dtype=bool))
        if restate:
            out["x"]["f32"] = np.array(out_x, dtype=f32)
    if out_y is not None:
        out["y"] = np.array(out_y, dtype=f32)
    n = (x_all if x_all is not None else y_all).shape[0]
    rows = []
    for b in range(count):
        p = first + b
        r = int(index[p]) if 0 <= p < len(index) else -1
        if not 0 <= r < n:
            if "x" in out:
                out["x"]["ref"][b] = 0
                if restate:
                    out["x"]["f32"][b] = 0
            if "y" in out:
                out["y"][b] = 0
            rows.append(None)
            continue
        if partners is not None:
            p2, g = int(partners[b]), f32(gains[b])
        else:
            p2, g = mix_draw(seed, epoch, p, len(index), p_mix, *mix_gain)
        r2 = int(index[p2]) if 0 <= p2 < len(index) else -1
        r2 = r2 if 0 <= r2 < n else -1
        refused = r2 >= 0 and occ is not None and not fits(occ, r, r2, overlaps)
        mixed = r2 >= 0 and not refused
        rows.append(dict(p2=p2, g=g, r2=r2, refused=refused, mixed=mixed))
        if "x" in out:
            x = np.asarray(x_all[r], dtype=f32)
            if mixed:
                got = list(mix_x(x, x_all[r2], g, stats))
            else:
                got = [x.astype(np.float64), np.zeros(x.shape, dtype=np.complex128), np.zeros(x.shape), np.ones(x.shape, dtype=bool)]
            F, T = x.shape[1:]
            hit = np.zeros(x.shape, dtype=bool)
            for lo, width in _masks(words(seed, epoch, p, 1), n_fmask, f_max, F):
                hit[:, lo:lo + width, :] = True
            for lo, width in _masks(words(seed, epoch, p, 2), n_tmask, t_max, T):
                hit[:, :, lo:lo + width] = True
            got[0][hit], got[1][hit], got[2][hit], got[3][hit] = np.float64(f32(fill)), 0.0, 0.0, True
            for key, v in zip(("ref", "z", "weight", "exact"), got):
                out["x"][key][b] = v
            if restate:
                o = mix_x_f32(x, x_all[r2], g, stats) if mixed else x.copy()
                o[hit] = f32(fill)
                out["x"]["f32"][b] = o
        if "y" in out:
            y = np.asarray(y_all[r], dtype=f32)
            out["y"][b] = merge_targets(y, y_all[r2], overlaps) if mixed else y
    return dict(rows=rows, **out)


def error_ratio(got, side, stats):
    """max over the mixed positions of |z(got) - z'| / (2^-24 * Wt + TINY / K): at most K when the bound holds.  0 when
    nothing was mixed."""
    inexact = ~side["exact"]
    if not inexact.any():
        return 0.0
    z, _, _ = complex_of(got, stats)
    return float((np.abs(z - side["z"])[inexact] / (U24 * side["weight"][inexact] + TINY / K)).max())


# ---- the inputs of the GPU tests (here, so that the host test can measure the CPU restatement over them) ----------------
EXPLICIT_GAINS = (0.5, 1.0, 0.75, 2.0, 1.0, 0.5, 1.25)


def explicit_pairs(n):
    """(partner row, gain) of every row for the calls with explicit partners: row r takes row r + 1 (the last one row 0)."""
    return [((r + 1) % n, f32(EXPLICIT_GAINS[r % len(EXPLICIT_GAINS)])) for r in range(n)]


@functools.lru_cache(maxsize=None)
def inputs(name, stats_i):
    """x stored fp32 (n, C, F, T) of a case of loader_polar_ref.CASES: magnitudes |N(0, 1)| * 3, phases uniform in (-pi, pi],
    standardised with STATS[stats_i] in fp32.  Engineered bins in every row and pair at f = 0, for the partners of
    `explicit_pairs`: t = 0: z_B = -z_A / g (the sum cancels); t = 1: both magnitudes 0; t = 2: the phase exactly fp32 pi."""
    n, C, F, T = CASES[name][0]
    stats = STATS[stats_i]
    h = C // 2
    rng = np.random.default_rng(1000 + n * C + F * T + stats_i)
    x = np.empty((n, C, F, T), dtype=f32)
    x[:, :h] = np.abs(rng.standard_normal((n, h, F, T))) * 3
    x[:, h:] = -rng.uniform(-np.pi, np.pi, (n, h, F, T))                      # (-pi, pi]
    for r, (r2, g) in enumerate(explicit_pairs(n)[:-1]):                      # a chain: row r + 1 cancels row r
        x[r2, :h, 0, 0] = x[r, :h, 0, 0] / g
        x[r2, h:, 0, 0] = np.where(x[r, h:, 0, 0] > 0, x[r, h:, 0, 0] - f32(np.pi), x[r, h:, 0, 0] + f32(np.pi))
    x[:, :h, 0, 1] = 0
    x[:, h:, 0, 2] = f32(np.pi)
    if stats is not None:
        mean_m, sd_m, mean_p, sd_p = (f32(v) for v in stats)
        x[:, :h] = (x[:, :h] - mean_m) / sd_m
        x[:, h:] = (x[:, h:] - mean_p) / sd_p
    x.setflags(write=False)
    return x


# per overlaps and row (mod 7) the events of every class in the fullest frame
_EVENTS = {3: ((0, 0), (1, 1), (2, 1), (3, 0), (1, 2), (0, 3), (1, 0)),
           2: ((0, 0, 0), (1, 0, 1), (2, 1, 0), (0, 1, 1), (1, 2, 0), (0, 0, 2), (1, 1, 0))}


@functools.lru_cache(maxsize=None)
def targets(n, overlaps):
    """fp32 (n, T_OUT, 24): 6 slots, classes = 6 / overlaps.  Row r holds up to _EVENTS[overlaps][r % 7] events per class:
    exactly that many in frame 0, at most that many in the others, in slots drawn at random (so not a prefix), with activities 1, 0.75 or 0.501; inactive slots hold 0, 0.5, 0.25
    or, once per row, a NaN, and locations that are not 0, which a merge must not carry along."""
    n_sed, classes = 6, 6 // overlaps
    rng = np.random.default_rng(77 + n + overlaps)
    y = np.empty((n, T_OUT, 4 * n_sed), dtype=f32)
    y[..., n_sed:] = rng.standard_normal((n, T_OUT, 3 * n_sed))
    for r in range(n):
        for c in range(classes):
            most = _EVENTS[overlaps][r % 7][c]
            for fr in range(T_OUT):
                k = most if fr == 0 else int(rng.integers(0, most + 1))
                on = rng.permutation(overlaps)[:k]
                slot = y[r, fr, c * overlaps:(c + 1) * overlaps]
                slot[:] = rng.choice(np.array([0.0, 0.5, 0.25], dtype=f32), overlaps)
                slot[on] = rng.choice(np.array([1.0, 0.75, 0.501], dtype=f32), k)
        idle = np.argwhere(~(y[r, :, :n_sed] > 0.5))
        if len(idle):
            fr, s = idle[int(rng.integers(len(idle)))]
            y[r, fr, s] = np.nan
    y.setflags(write=False)
    return y


DRAWN = dict(seed=5, p_mix=0.6, positions=12, epochs=(0, 1), mix_gain=(0.5, 1.0))      # the drawn test of the GPU suite


def drawn_rows(n, overlaps, epoch):
    """The `rows` of the drawn test's reference for one epoch, targets alone (the decisions do not depend on the predictors)."""
    y = targets(n, overlaps)
    index = np.array([p % n for p in range(DRAWN["positions"])])
    ref = gather_mix(None, y, index, 0, len(index), None, np.zeros((len(index),) + y.shape[1:], f32), seed=DRAWN["seed"], epoch=epoch,
                     overlaps=overlaps, p_mix=DRAWN["p_mix"], mix_gain=DRAWN["mix_gain"], occ=occupancy(y, overlaps))
    return ref["rows"]


def measured_cpu_ratio():
    """The largest `error_ratio` of the fp32 restatement over every case and statistics set of the GPU tests, with the
    explicit partners and with drawn ones: numpy on the CPU."""
    worst = 0.0
    for name, ((n, C, F, T), _, _) in CASES.items():
        for si, stats in enumerate(STATS):
            x = inputs(name, si)
            pairs = explicit_pairs(n)
            for kw in (dict(partners=[r2 for r2, _ in pairs], gains=[g for _, g in pairs]), dict(p_mix=1.0)):
                ref = gather_mix(x, None, np.arange(n), 0, n, np.zeros_like(x), None, seed=3, epoch=0, overlaps=3, stats=stats,
                                 restate=True, **kw)
                worst = max(worst, error_ratio(ref["x"]["f32"], ref["x"], stats))
    return worst
