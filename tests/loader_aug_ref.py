"""Host reference of the augmented minibatch gather, seld_gather_rows_aug, written from the text of include/seld_hip.h
over tests/philox_ref.py.  numpy only: no torch, no GPU.  The kernel moves data, flips signs and adds one fp32
constant, so everything here is float32 and comparable bit for bit.

    counter = (uint64)epoch << 34 | (uint64)p << 2 | g   (mod 2^64),  key = seed,  words w[0..3] = (c0, c1, c2, c3)
    int(w, n) = ((uint64)w * n) >> 32          coin(w) = u01(w) < float32(p_swap)
    g = 0: transform iff K > 0 and coin(w[1]); k = int(w[0], K)
    g = 1: frequency masks, mask m: width = int(w[2m], f_max + 1), first = int(w[2m + 1], F - width + 1)
    g = 2: time masks, the same over T with t_max
"""
import numpy as np

from tests import philox_ref as P

PI_F = np.float32(np.pi)


def words(seed, epoch, p, group):
    """The four uint32 words of group `group` of the sample at position p in epoch `epoch`."""
    counter = ((int(epoch) << 34) | (int(p) << 2) | int(group)) & P.MASK64
    return [int(w) for w in P.philox4x32_10(np.uint64(counter), np.uint64(int(seed) & P.MASK64))[0]]


def int_below(w, n):
    return (int(w) * int(n)) >> 32


def _masks(w, n, max_width, size):
    out = []
    for m in range(n):
        width = int_below(w[2 * m], max_width + 1)
        out.append((int_below(w[2 * m + 1], size - width + 1), width))
    return out


def draws(seed, epoch, p, K, p_swap, n_fmask, f_max, F, n_tmask, t_max, T):
    """dict(k=transform index or None, fmasks=[(first, width)], tmasks=[(first, width)]) of one sample."""
    w = words(seed, epoch, p, 0)
    k = None
    if K > 0 and P.u01(np.uint32(w[1])) < np.float32(p_swap):
        k = int_below(w[0], K)
    return dict(k=k, fmasks=_masks(words(seed, epoch, p, 1), n_fmask, f_max, F),
                tmasks=_masks(words(seed, epoch, p, 2), n_tmask, t_max, T))


def flipop(flip, v):
    v = np.asarray(v, dtype=np.float32)
    if flip == 1:
        return np.negative(v)
    if flip == 2:
        return np.where(v <= 0, v + PI_F, v - PI_F).astype(np.float32)
    return v.copy()


def transform_x(x, row):
    """x (C, F, T) float32 under the table row (src[C], flip[C], axis[3], sign[3])."""
    C = x.shape[0]
    return np.stack([flipop(int(row[C + c]), x[int(row[c])]) for c in range(C)])


def transform_y(y, row, C):
    """y (..., 4 * n_sed) float32: location (s, a) <- float32(sign[a]) * location (s, axis[a]); activity copied."""
    n_sed = y.shape[-1] // 4
    axis, sign = row[2 * C:2 * C + 3], row[2 * C + 3:2 * C + 6]
    out = y.copy()
    for a in range(3):
        out[..., n_sed + a::3] = np.float32(sign[a]) * y[..., n_sed + int(axis[a])::3]
    return out


def augment_sample(x, y, seed, epoch, p, table, p_swap, n_fmask, f_max, n_tmask, t_max, fill):
    """(x', y') of the sample at position p.  x (C, F, T) or None, y (T_out, 4 * n_sed) or None, table (K, 2C + 6) or None."""
    K = 0 if table is None else len(table)
    C = x.shape[0] if x is not None else (np.asarray(table).shape[1] - 6) // 2 if K else 1
    F, T = (x.shape[1], x.shape[2]) if x is not None else (max(f_max, 1), max(t_max, 1))
    d = draws(seed, epoch, p, K, p_swap, n_fmask, f_max, F, n_tmask, t_max, T)
    if d["k"] is not None:
        row = np.asarray(table)[d["k"]]
        x = None if x is None else transform_x(x, row)
        y = None if y is None else transform_y(y, row, C)
    if x is not None:
        x = x.copy()
        for first, width in d["fmasks"]:
            x[:, first:first + width, :] = np.float32(fill)
        for first, width in d["tmasks"]:
            x[:, :, first:first + width] = np.float32(fill)
    return x, (None if y is None else y.copy())


def gather_aug(x_all, y_all, index, first, count, out_x, out_y, *, seed, epoch, table=None, p_swap=0.0, n_fmask=0,
               f_max=0, n_tmask=0, t_max=0, fill=0.0):
    """What the call leaves in copies of the batch buffers out_x (B, C, F, T) / out_y (B, T_out, 4 * n_sed): rows b < count
    hold the augmented sample index[first + b]; a position outside `index` or an index outside [0, n) gives zeros, not
    augmented; rows >= count keep what they held."""
    out_x = None if out_x is None else np.array(out_x, dtype=np.float32)
    out_y = None if out_y is None else np.array(out_y, dtype=np.float32)
    n = (x_all if x_all is not None else y_all).shape[0]
    for b in range(count):
        p = first + b
        r = int(index[p]) if 0 <= p < len(index) else -1
        if not 0 <= r < n:
            for out in (out_x, out_y):
                if out is not None:
                    out[b] = 0
            continue
        x, y = augment_sample(None if x_all is None else np.asarray(x_all[r], dtype=np.float32),
                              None if y_all is None else np.asarray(y_all[r], dtype=np.float32),
                              seed, epoch, p, table, p_swap, n_fmask, f_max, n_tmask, t_max, fill)
        if out_x is not None:
            out_x[b] = x
        if out_y is not None:
            out_y[b] = y
    return out_x, out_y
