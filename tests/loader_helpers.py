"""What the GPU tests of the loader gathers share (tests/test_gpu_loader_*.py): the device scalars and buffers of a call,
the placement of a resident array off 16-byte alignment, the comparison as bits, and the two ways a rotated batch is held
to its host reference (tests/loader_rot_ref.py, tests/loader_polar_ref.py)."""
import numpy as np
import torch

from tests import loader_polar_ref as P
from tests import loader_rot_ref as R

DEV = "cuda:0"
SENTINEL = -7.5
PI32 = float(np.float32(np.pi))
_seen = {"ratio": 0.0}


def epoch(value):
    return torch.tensor([value], device=DEV, dtype=torch.int32)


def bits(t):
    return t.contiguous().view(torch.int32)


def buffers(x_shape, y_shape, rows):
    """Batch buffers of `rows` rows full of the sentinel; a shape is that of one row."""
    return torch.full((rows,) + tuple(x_shape), SENTINEL, device=DEV), torch.full((rows,) + tuple(y_shape), SENTINEL, device=DEV)


def shifted(x, shift):
    """The host array x on the device, its first element `shift` floats behind a 16-byte boundary."""
    flat = torch.zeros(x.size + shift, device=DEV)
    flat[shift:] = torch.tensor(x).reshape(-1).to(DEV)
    xd = flat[shift:].view(x.shape)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4 * shift
    return xd


def hold_rot(got, side, factor, key, what):
    """Exact positions as bits, the others within factor * 2^-24 * side[key] + TINY of the float64 reference."""
    got = got.cpu().numpy()
    exact = side["exact"]
    assert R.bits_equal(got, side["ref"])[exact].all(), what
    err = np.abs(got.astype(np.float64) - side["ref"])[~exact]
    bound = (factor * R.U24 * side[key] + R.TINY)[~exact]
    assert (err <= bound).all(), (what, float((err / bound).max()))


def hold_polar(got, side, groups, stats, what):
    """Exact positions as bits; the complex value of the others within K * 2^-24 * Wt + TINY; the ranges."""
    got = got.cpu().numpy()
    exact = side["exact"]
    assert P.bits_equal(got, side["ref"])[exact].all(), what
    if exact.all():
        return
    z, M, Ph = P.complex_of(got, groups, stats)
    err = np.abs(z - side["z"])[~exact]
    bound = (P.K * P.U24 * side["weight"] + P.TINY)[~exact]
    ratio = P.error_ratio(got, side, groups, stats)
    _seen["ratio"] = max(_seen["ratio"], ratio)
    print(what, "largest |got - ref| / (2^-24 Wt):", ratio, "largest so far:", _seen["ratio"])
    assert (err <= bound).all(), (what, ratio)
    mean_m, _, mean_p, _ = P.NO_STATS if stats is None else stats
    slack_m = 0.0 if stats is None else 2.0 ** -23 * (np.abs(M[~exact]) + abs(mean_m))
    slack_p = 0.0 if stats is None else 2.0 ** -23 * (np.pi + abs(mean_p))
    assert (M[~exact] >= -slack_m).all() and (np.abs(Ph[~exact]) <= PI32 + slack_p).all(), what
