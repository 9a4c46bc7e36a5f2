"""Host reference of whole-recording inference, seld_window_batch and seld_ensemble_combine, written from the text of
include/seld_hip.h.  numpy only: no torch, no GPU.  window_batch moves data, flips signs and adds one fp32 constant, so it
is float32 and comparable bit for bit; combine is float64, the yardstick of the kernel's fp32 sums.

    members m = (r * S + s) * K + k;  a table row = src[C], flip[C], axis[3], sign[3];  no table: the identity, K = 1
    forward (training) label map of a row:   location'[a] = sign[a] * location[axis[a]]
"""
import itertools

import numpy as np

from tests.loader_aug_ref import flipop

AMBIGUOUS = 1e-4
EPS = 2.0 ** -24


def rows_of(table):
    """(K, axis (K, 3), sign (K, 3)) of a table or None."""
    if table is None:
        return 1, np.array([[0, 1, 2]]), np.array([[1, 1, 1]])
    table = np.asarray(table)
    C = (table.shape[1] - 6) // 2
    return table.shape[0], table[:, 2 * C:2 * C + 3], table[:, 2 * C + 3:]


def window_batch(x, out, *, seg_len, hop, segments, table=None, first=0, count=None):
    """A copy of the batch buffer out (B, C, F, seg_len) after the call on recordings x (R, C, F, L)."""
    x = np.asarray(x, dtype=np.float32)
    out = np.array(out, dtype=np.float32)
    R, C, F, L = x.shape
    K = 1 if table is None else len(table)
    count = min(out.shape[0], R * segments * K - first) if count is None else count
    for b in range(count):
        m = first + b
        k, rs = m % K, m // K
        s, r = rs % segments, rs // segments
        t0 = s * hop
        win = np.zeros((C, F, seg_len), dtype=np.float32)
        live = max(0, min(seg_len, L - t0))
        win[:, :, :live] = x[r, :, :, t0:t0 + live]
        if table is not None:
            row = np.asarray(table)[k]
            win = np.stack([flipop(int(row[C + c]) & 3, win[int(row[c])]) for c in range(C)])
        out[b] = win
    return out


def transform_doa(doa, axis, sign):
    """The training transform of a row on (..., 3) locations: location'[a] = sign[a] * location[axis[a]]."""
    return np.stack([sign[a] * doa[..., int(axis[a])] for a in range(3)], axis=-1)


def untransform_doa(doa, axis, sign):
    """Its inverse, as the header states it: q[axis[a]] = sign[a] * doa[a]."""
    q = np.zeros_like(doa)
    for a in range(3):
        q[..., int(axis[a])] = sign[a] * doa[..., a]
    return q


def anchors(S, T_out, hop_out, frames, win):
    """(s_star (frames,), the anchor window of every frame, -1 where none covers it; cover (frames,), windows covering)."""
    best = np.full(frames, -np.inf)
    s_star = np.full(frames, -1)
    cover = np.zeros(frames, dtype=np.int64)
    for s in range(S):                                      # ascending: `>` keeps the lowest s of equals
        t = s * hop_out + np.arange(T_out)
        ok = t < frames
        t, w = t[ok], np.asarray(win, dtype=np.float64)[ok]
        cover[t] += 1
        up = w > best[t]
        best[t[up]] = w[up]
        s_star[t[up]] = s
    return s_star, cover


def combine(sed, doa, *, recordings, segments, hop_out, frames, classes, overlaps, win, table=None, align=True):
    """dict(sed (R, frames, n), doa (R, frames, 3n) float64, perm (M, T_out, classes) int32, members (frames,) the N of the
    bound, ambiguous_members (M, T_out, classes) bool: the member's second-best permutation costs within AMBIGUOUS of its
    best, ambiguous (R, frames, classes) bool: the cell has such a member)."""
    R, S, O = recordings, segments, overlaps
    K, axis, sign = rows_of(table)
    T_out = sed.shape[1]
    n = classes * O
    p = np.asarray(sed, dtype=np.float64).reshape(R, S, K, T_out, classes, O)
    d = np.asarray(doa, dtype=np.float64).reshape(R, S, K, T_out, classes, O, 3)
    q = np.stack([untransform_doa(d[:, :, k], axis[k], sign[k].astype(np.float64)) for k in range(K)], axis=2)
    win = np.asarray(win, dtype=np.float64)
    s_star, cover = anchors(S, T_out, hop_out, frames, win)
    perms = np.array(list(itertools.permutations(range(O))))                 # lexicographic
    do_align = align and O > 1

    acc_p = np.zeros((R, frames, classes, O))
    acc_q = np.zeros((R, frames, classes, O, 3))
    wsum = np.zeros(frames)
    perm = np.full((R, S, K, T_out, classes), -1, dtype=np.int32)
    ambiguous = np.zeros((R, frames, classes), dtype=bool)
    ambiguous_members = np.zeros((R, S, K, T_out, classes), dtype=bool)
    covered = np.flatnonzero(s_star >= 0)
    pA = np.zeros((R, frames, classes, O))
    qA = np.zeros((R, frames, classes, O, 3))
    pA[:, covered] = p[:, s_star[covered], 0, covered - s_star[covered] * hop_out]
    qA[:, covered] = q[:, s_star[covered], 0, covered - s_star[covered] * hop_out]
    for s in range(S):
        j = np.arange(T_out)
        t = s * hop_out + j
        j, t = j[t < frames], t[t < frames]
        for k in range(K):
            pm, qm = p[:, s, k, j], q[:, s, k, j]                           # (R, nj, classes, O[, 3])
            if do_align:
                costs = np.stack([((pm[..., pi] - pA[:, t]) ** 2).sum(-1) + ((qm[..., pi, :] - qA[:, t]) ** 2).sum((-1, -2))
                                  for pi in perms])
                best = np.argmin(costs, axis=0)                             # the first of equals
                ordered = np.sort(costs, axis=0)
                ambiguous_members[:, s, k, j] = (ordered[1] - ordered[0]) < AMBIGUOUS
                ambiguous[:, t] |= ambiguous_members[:, s, k, j]
                pick = perms[best]                                          # (R, nj, classes, O)
                pm = np.take_along_axis(pm, pick, axis=-1)
                qm = np.take_along_axis(qm, pick[..., None], axis=-2)
                perm[:, s, k, j] = best
            else:
                perm[:, s, k, j] = 0
            w = win[j][None, :, None, None]
            acc_p[:, t] += w * pm
            acc_q[:, t] += w[..., None] * qm
            wsum[t] += win[j]
    out_p = np.zeros_like(acc_p)
    out_q = np.zeros_like(acc_q)
    out_p[:, covered] = acc_p[:, covered] / wsum[covered][None, :, None, None]
    out_q[:, covered] = acc_q[:, covered] / wsum[covered][None, :, None, None, None]
    return dict(sed=out_p.reshape(R, frames, n), doa=out_q.reshape(R, frames, 3 * n),
                perm=perm.reshape(R * S * K, T_out, classes), members=cover * K, ambiguous=ambiguous,
                ambiguous_members=ambiguous_members.reshape(R * S * K, T_out, classes))


def bound(members, peak):
    """|out - ref| <= (2N + 4) * 2^-24 * max|v| per frame: N products, two N-term fp32 sums (numerator and weights),
    one division, the inputs' own rounding to fp32 included in the 4.  members (frames,) -> (1, frames, 1)."""
    return ((2 * np.asarray(members) + 4) * EPS * peak)[None, :, None]


def window_weights(kind, T_out):
    j = np.arange(T_out)
    return np.ones(T_out, np.float32) if kind == "uniform" else np.minimum(j + 1, T_out - j).astype(np.float32)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def hand_table(K, C=4):
    """K rows over C channels whose axis maps include both 3-cycles (the presets only swap x and y)."""
    maps = [([0, 1, 2], [1, 1, 1]), ([2, 0, 1], [-1, 1, -1]), ([1, 2, 0], [1, -1, -1]), ([0, 2, 1], [-1, -1, 1])]
    rows = [list(range(C)) + [0] * C + list(maps[k % 4][0]) + list(maps[k % 4][1]) for k in range(K)]
    return np.asarray(rows, dtype=np.int32)


# (R, S, K, T_out, hop_out, frames, classes, O)
PLANTED_SHAPES = [(1, 1, 1, 8, 8, 8, 14, 3), (2, 4, 16, 8, 4, 19, 14, 3), (2, 3, 8, 8, 8, 24, 14, 2),
                  (1, 5, 16, 8, 3, 20, 1, 3), (1, 2, 4, 8, 4, 12, 14, 1), (1, 18, 16, 64, 32, 600, 14, 3)]
RANDOM_SHAPES = [(2, 4, 16, 8, 4, 19, 14, 3), (1, 18, 16, 64, 32, 600, 14, 3)]
# chosen from seeds 0..11 by the reference alone (tests/test_ensemble_host.py asserts it): no ambiguous member at the small
# shape, 17 of 258048 at the large one
RANDOM_SEEDS = {RANDOM_SHAPES[0]: 4, RANDOM_SHAPES[1]: 0}


def table_for(K, foa_transforms):
    """The table a case of K members per window uses: None, the 3-cycle rows, or the 8 / 16 presets."""
    if K == 1:
        return None
    if K == 16:
        return foa_transforms(mics=1, phase=True)
    if K == 8:
        return foa_transforms(mics=2, elevation=False)
    return hand_table(K)


def planted(shape, table, seed=0):
    """dict(sed (M, T_out, n), doa (M, T_out, 3n) float32, truth_sed (R, frames, n), truth_doa (R, frames, 3n) float64 in the
    ANCHOR's slot order for the window weights `win` given later through `truth_for`, ...).  A field (R, frames, classes,
    O): the slots of a cell are +-0.8 times DISTINCT unit axes plus jitter <= 0.05, activities in {0.1, 0.5, 0.9}; a
    member is the field plus noise <= 0.01 per value, its slots shuffled independently per (m, j, c), then transformed
    by its row.  The right pairing of two members costs <= 12 * 0.02^2 = 0.0048, a wrong one >= 2 * (0.8 * sqrt(2) -
    2 * 0.06 * sqrt(3))^2 > 0.4: no cell is ambiguous.  Positions past `frames` hold noise."""
    R, S, K, T_out, hop_out, frames, classes, O = shape
    rng = np.random.default_rng(seed + 17 * sum(shape))
    _, axis, sign = rows_of(table)
    act = rng.choice([0.1, 0.5, 0.9], size=(R, frames, classes, O))
    which = np.argsort(rng.random((R, frames, classes, 3)), axis=-1)[..., :O]              # distinct axes of a cell
    loc = np.zeros((R, frames, classes, O, 3))
    np.put_along_axis(loc, which[..., None], 0.8 * rng.choice([-1.0, 1.0], size=(R, frames, classes, O, 1)), axis=-1)
    loc += rng.uniform(-0.05, 0.05, size=loc.shape)
    sed = rng.uniform(0.0, 1.0, size=(R, S, K, T_out, classes, O))
    doa = rng.uniform(-1.0, 1.0, size=(R, S, K, T_out, classes, O, 3))
    shuffle = np.argsort(rng.random((R, S, K, T_out, classes, O)), axis=-1)                # member slot i holds field slot shuffle[i]
    for s in range(S):
        j = np.arange(T_out)
        t = s * hop_out + j
        j, t = j[t < frames], t[t < frames]
        for k in range(K):
            sh = shuffle[:, s, k, j]
            pm = np.take_along_axis(act[:, t], sh, axis=-1) + rng.uniform(-0.01, 0.01, size=sh.shape)
            qm = np.take_along_axis(loc[:, t], sh[..., None], axis=-2) + rng.uniform(-0.01, 0.01, size=sh.shape + (3,))
            sed[:, s, k, j] = pm
            doa[:, s, k, j] = transform_doa(qm, axis[k], sign[k].astype(np.float64))
    n = classes * O
    return dict(sed=sed.reshape(R * S * K, T_out, n).astype(np.float32), doa=doa.reshape(R * S * K, T_out, 3 * n).astype(np.float32),
                act=act, loc=loc, shuffle=shuffle)


def truth_for(case, shape, win):
    """The field in the anchor's slot order: (truth_sed (R, frames, n), truth_doa (R, frames, 3n)); uncovered frames zero."""
    R, S, K, T_out, hop_out, frames, classes, O = shape
    s_star, _ = anchors(S, T_out, hop_out, frames, win)
    t = np.flatnonzero(s_star >= 0)
    sh = case["shuffle"][:, s_star[t], 0, t - s_star[t] * hop_out]
    ts = np.zeros((R, frames, classes, O))
    td = np.zeros((R, frames, classes, O, 3))
    ts[:, t] = np.take_along_axis(case["act"][:, t], sh, axis=-1)
    td[:, t] = np.take_along_axis(case["loc"][:, t], sh[..., None], axis=-2)
    return ts.reshape(R, frames, classes * O), td.reshape(R, frames, 3 * classes * O)


def uniform_members(shape, seed):
    """sed in (0, 1), doa in (-1, 1), float32."""
    R, S, K, T_out, _, _, classes, O = shape
    rng = np.random.default_rng(seed)
    n = classes * O
    return (rng.uniform(0.0, 1.0, size=(R * S * K, T_out, n)).astype(np.float32),
            rng.uniform(-1.0, 1.0, size=(R * S * K, T_out, 3 * n)).astype(np.float32))
