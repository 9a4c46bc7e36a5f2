"""Host reference of the rotating gather for magnitude-phase predictors, seld_gather_rows_polar, written from the text of
include/seld_hip.h over tests/loader_rot_ref.py (the draw of R, the Philox words, the masks and the label rotation are
the rotated gather's).  numpy only: no torch, no GPU.

The stored fp32 values are taken as exact.  In float64, per group (mx, my, mz, px, py, pz) and (f, t):

    m_j = x[m_j] * sd_m + mean_m      phi_j = x[p_j] * sd_p + mean_p      z_j = m_j e^(i phi_j)        j = x, y, z
    z'_a = sum_j R[a][j] z_j                                                                           a = 0, 1, 2

The kernel writes magnitude and phase of z'_a, standardised again.  A phase is ill conditioned where the magnitude is
small and wraps at +-pi, so `gather_polar` returns the COMPLEX value z'_a (at the positions of both channels m_a and
p_a) and the tests compare on it; with it the weight

    Wt_a = (sum_j |R[a][j]| (|m_j| + |mean_m|)) * (1 + pi + |mean_p|)

that the error bound K * 2^-24 * Wt + TINY of tests/test_gpu_loader_polar.py scales with, and `exact`: True where the
kernel only moves bits or writes `fill` (there `ref` holds the float32 value).  `rotate_x_f32` restates the kernel with
every operation rounded to fp32; the distance of that restatement from the float64 reference over the inputs of the GPU
tests, measured on the CPU (`measured_cpu_ratio`), sets K."""
import functools

import numpy as np

from tests.loader_rot_ref import TINY, U24, _masks, bits_equal, rotate_y, rotated_flags, rotation, words   # noqa: F401

f32 = np.float32
NO_STATS = (0.0, 1.0, 0.0, 1.0)
# the error bound of the GPU tests: 4 times the largest ratio `measured_cpu_ratio` finds, rounded up to a power of two
# (tests/test_loader_polar_host.py asserts that this is so); the margin is for the device's sincosf and atan2f, which
# are a few ulp looser than numpy's
K = 8


def _stats64(stats):
    """(mean_m, sd_m, mean_p, sd_p) as the float64 values of the fp32 numbers the kernel reads; None: (0, 1, 0, 1)."""
    return tuple(float(f32(v)) for v in (NO_STATS if stats is None else stats))


def destandardise(x, groups, stats):
    """(M, P): float64 magnitude and phase (n_groups, 3, ...) of the group channels of x (C, ...)."""
    mean_m, sd_m, mean_p, sd_p = _stats64(stats)
    x64 = np.asarray(x, dtype=np.float64)
    M = np.stack([x64[list(g[:3])] for g in groups]) * sd_m + mean_m
    P = np.stack([x64[list(g[3:])] for g in groups]) * sd_p + mean_p
    return M, P


def rotate_x(x, R, groups, stats=None):
    """(ref float64, z complex128, weight, exact) of x (C, F, T) under R: z and weight at both channels of every
    (group, axis), ref = x elsewhere."""
    mean_m, _, mean_p, _ = _stats64(stats)
    x64 = np.asarray(x, dtype=np.float64)
    ref, z, weight = x64.copy(), np.zeros(x64.shape, dtype=np.complex128), np.zeros_like(x64)
    exact = np.ones(x64.shape, dtype=bool)
    M, P = destandardise(x, groups, stats)
    R = np.asarray(R, dtype=np.float64)
    for g, grp in enumerate(groups):
        zj = M[g] * np.exp(1j * P[g])
        for a in range(3):
            za = np.einsum('j,j...->...', R[a], zj)
            wa = np.einsum('j,j...->...', np.abs(R[a]), np.abs(M[g]) + abs(mean_m)) * (1 + np.pi + abs(mean_p))
            for c in (grp[a], grp[3 + a]):
                z[c], weight[c], exact[c], ref[c] = za, wa, False, np.nan
    return ref, z, weight, exact


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64; the sum is rounded to float64 and then to fp32."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def rotate_x_f32(x, R, groups, stats=None):
    """What the kernel stores for a rotated sample, every operation of include/seld_hip.h rounded to fp32 (numpy's fp32
    sin, cos, arctan2 and sqrt in place of the device's): float32 (C, F, T)."""
    x = np.asarray(x, dtype=f32)
    out = x.copy()
    R = np.asarray(R, dtype=np.float64).astype(f32)
    mean_m, sd_m, mean_p, sd_p = (f32(v) for v in (NO_STATS if stats is None else stats))
    for grp in groups:
        re, im = [], []
        for j in range(3):
            m, phi = x[grp[j]], x[grp[3 + j]]
            if stats is not None:
                m, phi = _fma(m, sd_m, mean_m), _fma(phi, sd_p, mean_p)
            re.append((m * np.cos(phi).astype(f32)).astype(f32))
            im.append((m * np.sin(phi).astype(f32)).astype(f32))
        for a in range(3):
            ra = _fma(R[a, 2], re[2], _fma(R[a, 1], re[1], (R[a, 0] * re[0]).astype(f32)))
            ia = _fma(R[a, 2], im[2], _fma(R[a, 1], im[1], (R[a, 0] * im[0]).astype(f32)))
            mag = np.sqrt(_fma(ia, ia, (ra * ra).astype(f32))).astype(f32)
            phi = np.arctan2(ia, ra).astype(f32)
            if stats is not None:
                mag, phi = ((mag - mean_m).astype(f32) / sd_m).astype(f32), ((phi - mean_p).astype(f32) / sd_p).astype(f32)
            out[grp[a]], out[grp[3 + a]] = mag, phi
    return out


def complex_of(out, groups, stats):
    """The complex value a stored output (..., C, F, T) holds at both channels of every (group, axis), from its
    destandardised magnitude and phase in float64; (z, M, P) with M and P laid out like z (0 outside the groups)."""
    mean_m, sd_m, mean_p, sd_p = _stats64(stats)
    o64 = np.asarray(out, dtype=np.float64)
    z, Ms, Ps = np.zeros(o64.shape, dtype=np.complex128), np.zeros_like(o64), np.zeros_like(o64)
    for grp in groups:
        for a in range(3):
            M, P = o64[..., grp[a], :, :] * sd_m + mean_m, o64[..., grp[3 + a], :, :] * sd_p + mean_p
            for c in (grp[a], grp[3 + a]):
                z[..., c, :, :], Ms[..., c, :, :], Ps[..., c, :, :] = M * np.exp(1j * P), M, P
    return z, Ms, Ps


def gather_polar(x_all, y_all, index, first, count, out_x, out_y, *, seed, epoch, groups, stats=None, p_rot=0.0, rot_mirror=True,
                 rot_zflip=True, matrices=None, n_fmask=0, f_max=0, n_tmask=0, t_max=0, fill=0.0, restate=False):
    """What the call leaves in copies of the batch buffers: dict(rows=, x=dict(ref, z, weight, exact[, f32]), y=dict(ref,
    weight, plain, exact)) in the manner of loader_rot_ref.gather_rot.  `restate`: x also gets `f32`, the fp32
    restatement of the whole batch."""
    sides = {}
    if out_x is not None:
        ref = np.array(out_x, dtype=f32).astype(np.float64)
        sides["x"] = dict(ref=ref, z=np.zeros(ref.shape, dtype=np.complex128), weight=np.zeros_like(ref), exact=np.ones(ref.shape, dtype=bool))
        if restate:
            sides["x"]["f32"] = np.array(out_x, dtype=f32)
    if out_y is not None:
        ref = np.array(out_y, dtype=f32).astype(np.float64)
        sides["y"] = dict(ref=ref, weight=np.zeros_like(ref), plain=np.zeros_like(ref), exact=np.ones(ref.shape, dtype=bool))
    n = (x_all if x_all is not None else y_all).shape[0]
    rows = []
    for b in range(count):
        p = first + b
        r = int(index[p]) if 0 <= p < len(index) else -1
        if not 0 <= r < n:
            for side in sides.values():
                side["ref"][b] = 0
                if "f32" in side:
                    side["f32"][b] = 0
            rows.append(None)
            continue
        if matrices is not None:
            d = dict(rotate=True, mirror=None, zflip=None, t=None, R=np.asarray(matrices[b], dtype=f32).astype(np.float64).reshape(3, 3))
        else:
            d = rotation(seed, epoch, p, p_rot, rot_mirror, rot_zflip)
        rows.append(d)
        if "x" in sides:
            x = np.asarray(x_all[r], dtype=f32)
            if d["rotate"]:
                got = [g.copy() for g in rotate_x(x, d["R"], groups, stats)]
            else:
                got = [x.astype(np.float64), np.zeros(x.shape, dtype=np.complex128), np.zeros(x.shape), np.ones(x.shape, dtype=bool)]
            F, T = x.shape[1:]
            hit = np.zeros(x.shape, dtype=bool)
            for lo, width in _masks(words(seed, epoch, p, 1), n_fmask, f_max, F):
                hit[:, lo:lo + width, :] = True
            for lo, width in _masks(words(seed, epoch, p, 2), n_tmask, t_max, T):
                hit[:, :, lo:lo + width] = True
            got[0][hit], got[1][hit], got[2][hit], got[3][hit] = np.float64(f32(fill)), 0.0, 0.0, True
            for key, g in zip(("ref", "z", "weight", "exact"), got):
                sides["x"][key][b] = g
            if restate:
                o = rotate_x_f32(x, d["R"], groups, stats) if d["rotate"] else x.copy()
                o[hit] = f32(fill)
                sides["x"]["f32"][b] = o
        if "y" in sides:
            y = np.asarray(y_all[r], dtype=f32)
            if d["rotate"]:
                got = rotate_y(y, d["R"])
            else:
                got = (y.astype(np.float64), np.zeros(y.shape), np.zeros(y.shape), np.ones(y.shape, dtype=bool))
            for key, g in zip(("ref", "weight", "plain", "exact"), got):
                sides["y"][key][b] = g
    return dict(rows=rows, **sides)


def error_ratio(got, side, groups, stats):
    """max over the rotated positions of |z(got) - z'| / (2^-24 * Wt + TINY / K): at most K when the bound holds.  0 when
    nothing was rotated."""
    inexact = ~side["exact"]
    if not inexact.any():
        return 0.0
    z, _, _ = complex_of(got, groups, stats)
    return float((np.abs(z - side["z"])[inexact] / (U24 * side["weight"][inexact] + TINY / K)).max())


# ---- the inputs of the GPU tests (here, so that the host test can measure the CPU restatement over them) ----------------
# (n, C, F, T), microphones, floats by which the resident predictors are shifted off 16-byte alignment
CASES = {
    "vector_8x5x12": ((7, 8, 5, 12), 1, 0),             # 16-byte path
    "scalar_16x9x7": ((6, 16, 9, 7), 2, 0),             # T % 4 != 0, two groups
    "tiles_8x33x68": ((5, 8, 33, 68), 1, 0),            # 561 pieces per group: more than one tile of 256, no multiple of it
    "misaligned_8x5x12": ((7, 8, 5, 12), 1, 1),         # T % 4 == 0 but the scalar path
}
STATS = [None, (2.5, 3.1, 0.01, 1.8), (40.0, 7.0, -0.3, 1.81)]
TARGET = (3, 24)                                        # (T_out, 4 * n_sed)


def polar_groups(mics, order="WYZX"):
    """hip_ops.foa_polar, restated (no package import here)."""
    pos = [order.index(ch) for ch in "XYZ"]
    return [tuple(4 * g + pos[a] for a in range(3)) + tuple(4 * (mics + g) + pos[a] for a in range(3)) for g in range(mics)]


@functools.lru_cache(maxsize=None)
def inputs(name, stats_i):
    """(x stored fp32 (n, C, F, T), y fp32 (n, 3, 24), groups) of a case: magnitudes |N(0, 1)| * 3, phases uniform in
    (-pi, pi], standardised with STATS[stats_i] in fp32; engineered positions in every row and group at f = 0:
    t = 0: z_y = -z_x (the mix cancels); t = 1: all three magnitudes 0; t = 2: the x phase exactly fp32 pi."""
    return make_inputs(*CASES[name][:2], stats_i)


@functools.lru_cache(maxsize=None)
def make_inputs(shape, mics, stats_i):
    """`inputs` for any (n, C, F, T) in the magnitude-phase layout of `mics` microphones (C = 8 * mics)."""
    n, C, F, T = shape
    stats = STATS[stats_i]
    groups = polar_groups(mics)
    rng = np.random.default_rng(n * C + F * T + stats_i)
    x = np.empty((n, C, F, T), dtype=f32)
    x[:, :C // 2] = np.abs(rng.standard_normal((n, C // 2, F, T))) * 3
    x[:, C // 2:] = -rng.uniform(-np.pi, np.pi, (n, C // 2, F, T))            # (-pi, pi]
    for mx, my, mz, px, py, pz in groups:
        x[:, my, 0, 0] = x[:, mx, 0, 0]
        x[:, py, 0, 0] = np.where(x[:, px, 0, 0] > 0, x[:, px, 0, 0] - f32(np.pi), x[:, px, 0, 0] + f32(np.pi))
        x[:, [mx, my, mz], 0, 1] = 0
        x[:, px, 0, 2] = f32(np.pi)
    if stats is not None:
        mean_m, sd_m, mean_p, sd_p = (f32(v) for v in stats)
        x[:, :C // 2] = (x[:, :C // 2] - mean_m) / sd_m
        x[:, C // 2:] = (x[:, C // 2:] - mean_p) / sd_p
    y = rng.standard_normal((n,) + TARGET).astype(f32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, groups


def general_rotations(count, seed):
    """`count` fp32 matrices (count, 9): proper rotations about random axes (not about z), every other one mirrored."""
    rng = np.random.default_rng(seed)
    mats = []
    for b in range(count):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q *= np.sign(np.linalg.det(q)) * (-1 if b % 2 else 1)
        mats.append(q.reshape(9))
    return np.stack(mats).astype(f32)


def measured_cpu_ratio():
    """The largest `error_ratio` of the fp32 restatement over every case and statistics set of the GPU tests, with the
    explicit matrices and with drawn rotations: numpy on the CPU."""
    worst = 0.0
    for name, ((n, C, F, T), _, _) in CASES.items():
        for si, stats in enumerate(STATS):
            x, y, groups = inputs(name, si)
            index = np.arange(n)
            for kw in (dict(matrices=general_rotations(n, 5)), dict(p_rot=1.0)):
                ref = gather_polar(x, None, index, 0, n, np.zeros_like(x), None, seed=3, epoch=0, groups=groups, stats=stats,
                                   restate=True, **kw)
                worst = max(worst, error_ratio(ref["x"]["f32"], ref["x"], groups, stats))
    return worst
