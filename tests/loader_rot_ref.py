"""Host reference of the gather with a rotation of the sound field, seld_gather_rows_rot, written from the text of
include/seld_hip.h over tests/loader_aug_ref.py (the words, the integers and the masks are the augmented gather's).
numpy only: no torch, no GPU.  The arithmetic is float64, from the fp32 value 2 * u01(w[0]) on:

    g = 3: w = words(seed, epoch, p, 3); rotated iff u01(w[1]) < float32(p_rot)
           t = float32(2) * u01(w[0]);  c = cos(pi * t), s = sin(pi * t)            (float64)
           mirror = rot_mirror and w[2] >> 31;  zflip = rot_zflip and w[3] >> 31
           R = diag(1, -1 if mirror else 1, -1 if zflip else 1) @ [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    x'[c_a] = sum_j R[a][j] x[c_j] per triple;  location'(s, a) = sum_j R[a][j] location(s, j);  then the masks

Besides the float64 result, `gather_rot` returns for every element the sum  sum_j |R[a][j]| |v_j|  (`weight`) and
sum_j |v_j|  (`plain`) that the two error bounds of tests/test_gpu_loader_rot.py scale with, and `exact`: True where the
kernel only moves bits or writes `fill` (there weight and plain are 0 and the float64 value is a float32)."""
import numpy as np

from tests import philox_ref as P
from tests.loader_aug_ref import _masks, int_below, words      # noqa: F401  (int_below: for the tests that import this module)

U24 = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)


def rotation(seed, epoch, p, p_rot, rot_mirror=True, rot_zflip=True):
    """dict(rotate, mirror, zflip, t (the fp32 value 2u), R (3, 3) float64) of the sample at position p."""
    w = words(seed, epoch, p, 3)
    rotate = bool(P.u01(np.uint32(w[1])) < np.float32(p_rot))
    t = np.float32(2) * np.float32(P.u01(np.uint32(w[0])))
    c, s = np.cos(np.pi * np.float64(t)), np.sin(np.pi * np.float64(t))
    mirror, zflip = bool(rot_mirror) and bool(w[2] >> 31), bool(rot_zflip) and bool(w[3] >> 31)
    R = np.diag([1.0, -1.0 if mirror else 1.0, -1.0 if zflip else 1.0]) @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return dict(rotate=rotate, mirror=mirror, zflip=zflip, t=t, R=R)


def rotated_flags(seed, epoch, positions, p_rot):
    """u01(w[1]) < p_rot for an array of positions at once."""
    counters = (np.uint64(int(epoch) & 0x3FFFFFFF) << np.uint64(34)) | (np.asarray(positions, dtype=np.uint64) << np.uint64(2)) | np.uint64(3)
    w = P.philox4x32_10(counters, np.uint64(int(seed) & P.MASK64))
    return P.u01(w[:, 1]) < np.float32(p_rot)


def rotate_x(x, R, triples):
    """(x' float64, weight, plain, exact) of x (C, F, T) float32 under R."""
    x64 = x.astype(np.float64)
    out, weight, plain = x64.copy(), np.zeros_like(x64), np.zeros_like(x64)
    exact = np.ones(x.shape, dtype=bool)
    for tri in triples:
        v = x64[list(tri)]
        for a in range(3):
            out[tri[a]] = np.einsum('j,j...->...', R[a], v)
            weight[tri[a]] = np.einsum('j,j...->...', np.abs(R[a]), np.abs(v))
            plain[tri[a]] = np.abs(v).sum(0)
            exact[tri[a]] = False
    return out, weight, plain, exact


def rotate_y(y, R):
    """The same of y (T_out, 4 * n_sed) float32: the location columns n_sed + 3 * s + a are mixed, the activity is copied."""
    n_sed = y.shape[-1] // 4
    y64 = y.astype(np.float64)
    out, weight, plain = y64.copy(), np.zeros_like(y64), np.zeros_like(y64)
    exact = np.ones(y.shape, dtype=bool)
    loc = y64[..., n_sed:].reshape(y.shape[:-1] + (n_sed, 3))
    out[..., n_sed:] = np.einsum('aj,...j->...a', R, loc).reshape(y.shape[:-1] + (3 * n_sed,))
    weight[..., n_sed:] = np.einsum('aj,...j->...a', np.abs(R), np.abs(loc)).reshape(y.shape[:-1] + (3 * n_sed,))
    plain[..., n_sed:] = np.repeat(np.abs(loc).sum(-1), 3, axis=-1)
    exact[..., n_sed:] = False
    return out, weight, plain, exact


def gather_rot(x_all, y_all, index, first, count, out_x, out_y, *, seed, epoch, triples, p_rot=0.0, rot_mirror=True,
               rot_zflip=True, matrices=None, n_fmask=0, f_max=0, n_tmask=0, t_max=0, fill=0.0):
    """What the call leaves in copies of the batch buffers, as dict(x=, y=) of dict(ref float64, weight, plain, exact), and
    rows=[None for an invalid row, else the `rotation` dict (rotate True and R = matrices[b] with explicit matrices)].
    Rows >= count keep what the buffers held; invalid rows are zero; both count as exact."""
    sides = {}
    for name, out in (("x", out_x), ("y", out_y)):
        if out is not None:
            ref = np.array(out, dtype=np.float32).astype(np.float64)
            sides[name] = dict(ref=ref, weight=np.zeros_like(ref), plain=np.zeros_like(ref), exact=np.ones(ref.shape, dtype=bool))
    n = (x_all if x_all is not None else y_all).shape[0]
    rows = []
    for b in range(count):
        p = first + b
        r = int(index[p]) if 0 <= p < len(index) else -1
        if not 0 <= r < n:
            for side in sides.values():
                side["ref"][b] = 0
            rows.append(None)
            continue
        if matrices is not None:
            d = dict(rotate=True, mirror=None, zflip=None, t=None, R=np.asarray(matrices[b], dtype=np.float32).astype(np.float64).reshape(3, 3))
        else:
            d = rotation(seed, epoch, p, p_rot, rot_mirror, rot_zflip)
        rows.append(d)
        if "x" in sides:
            x = np.asarray(x_all[r], dtype=np.float32)
            if d["rotate"]:
                got = rotate_x(x, d["R"], triples)
            else:
                got = (x.astype(np.float64), np.zeros(x.shape), np.zeros(x.shape), np.ones(x.shape, dtype=bool))
            got = [g.copy() for g in got]
            F, T = x.shape[1:]
            hit = np.zeros(x.shape, dtype=bool)
            for lo, width in _masks(words(seed, epoch, p, 1), n_fmask, f_max, F):
                hit[:, lo:lo + width, :] = True
            for lo, width in _masks(words(seed, epoch, p, 2), n_tmask, t_max, T):
                hit[:, :, lo:lo + width] = True
            got[0][hit], got[1][hit], got[2][hit], got[3][hit] = np.float64(np.float32(fill)), 0.0, 0.0, True
            for key, g in zip(("ref", "weight", "plain", "exact"), got):
                sides["x"][key][b] = g
        if "y" in sides:
            y = np.asarray(y_all[r], dtype=np.float32)
            if d["rotate"]:
                got = rotate_y(y, d["R"])
            else:
                got = (y.astype(np.float64), np.zeros(y.shape), np.zeros(y.shape), np.ones(y.shape, dtype=bool))
            for key, g in zip(("ref", "weight", "plain", "exact"), got):
                sides["y"][key][b] = g
    return dict(rows=rows, **sides)


def bits_equal(got, ref64):
    """got (float32) and the float32 the reference holds compare equal as BITS (a signed zero keeps its sign)."""
    return np.asarray(got, dtype=np.float32).view(np.uint32) == ref64.astype(np.float32).view(np.uint32)
