"""Host side of the rotating gather for magnitude-phase predictors: hip_ops.foa_polar, Augment(rot_polar=...), the flags of
train.augment_from_args, the tolerance constant of the GPU tests, and the fact the whole feature rests on, in float64:
magnitude and phase of the STFT of a sound field whose directional channels were mixed by R are the polar form of R
applied to the complex spectra.  No GPU."""
import math

import numpy as np
import pytest

from tests import loader_polar_ref as P
from tests.helpers import pkg


def test_foa_polar_values_and_refusals():
    H, L = pkg().hip_ops, pkg()._lib
    assert H.foa_polar() == [(3, 1, 2, 7, 5, 6)] == H.foa_polar("wyzx", 1)
    assert H.foa_polar(mics=2) == [(3, 1, 2, 11, 9, 10), (7, 5, 6, 15, 13, 14)]
    assert H.foa_polar("XWZY") == [(0, 3, 2, 4, 7, 6)]                      # W anywhere in the block
    assert H.foa_polar("XWZY", 2) == [(0, 3, 2, 8, 11, 10), (4, 7, 6, 12, 15, 14)]
    for order, mics in (("WXYZ", 1), ("XWZY", 2)):
        assert H.foa_polar(order, mics) == P.polar_groups(mics, order)
    # the magnitude half of a group is what the signed permutations of foa_transforms(phase=True) move
    table = H.foa_transforms("XWZY", mics=2, phase=True)
    swap = table[8]                                                         # x <-> y
    for mx, my, mz, px, py, pz in H.foa_polar("XWZY", 2):
        assert (swap[mx], swap[my], swap[mz], swap[px], swap[py], swap[pz]) == (my, mx, mz, py, px, pz)
    for kw in (dict(order="WXY"), dict(order="WXYY"), dict(order="ABCD"), dict(mics=0), dict(mics=3)):
        with pytest.raises(L.SeldHipError):
            H.foa_polar(**kw)


def test_augment_polar_fields_packing_and_refusals():
    H, L = pkg().hip_ops, pkg()._lib
    off = H.Augment()
    assert off.rot_polar is None and off.polar_channels is None and (off.p_rot, off.rot_triples) == (0.0, None)
    aug = H.Augment(p_rot=0.25, rot_polar=[[3, 1, 2, 7, 5, 6]], rot_mirror=False)
    assert aug.rot_polar == ((3, 1, 2, 7, 5, 6),) and aug.polar_channels == 8 and aug.polar_packed == 0x657213
    assert aug.rot_triples is None and aug.table is None and (aug.rot_mirror, aug.rot_zflip) == (False, True)
    two = H.Augment(p_rot=1.0, rot_polar=np.array(H.foa_polar(mics=2)))
    assert two.polar_channels == 16 and two.polar_packed == 0xEDF657_A9B213
    assert H.Augment(rot_polar=H.foa_polar()).p_rot == 0.0                  # groups alone: for explicit matrices
    # the old arguments give the Augment they gave
    old = H.Augment(p_rot=0.25, rot_triples=[(5, 6, 7), (1, 2, 3)], rot_zflip=False)
    assert (old.rot_triples, old.rot_packed, old.rot_channels, old.rot_polar) == (((5, 6, 7), (1, 2, 3)), 0x321765, 8, None)
    g = [(3, 1, 2, 7, 5, 6)]
    bad = [dict(p_rot=0.5), dict(p_rot=0.5, rot_polar=g, rot_triples=[(0, 4, 8)]), dict(p_rot=0.5, rot_polar=[]),
           dict(rot_polar=[(1, 2, 3)]), dict(rot_polar=[(1, 2, 3, 4, 5, 5)]), dict(rot_polar=[(1, 2, 3, 4, 5, 16)]),
           dict(rot_polar=[(-1, 2, 3, 4, 5, 6)]), dict(rot_polar=[(0.0, 1.0, 2.0, 3.0, 4.0, 5.0)]), dict(rot_polar=(1, 2, 3, 4, 5, 6)),
           dict(rot_polar=[(0, 1, 2, 3, 4, 5), (5, 6, 7, 8, 9, 10)]),
           dict(rot_polar=[(0, 1, 2, 3, 4, 5), (6, 7, 8, 9, 10, 11), (12, 13, 14, 15, 0, 1)]),
           dict(p_rot=1.5, rot_polar=g), dict(p_rot=0.5, rot_polar=g, p_swap=0.5, table=H.foa_transforms(phase=True))]
    for kw in bad:
        with pytest.raises(L.SeldHipError):
            H.Augment(**kw)
    with pytest.raises(Exception):
        aug.rot_polar = None                                                # frozen


def test_train_flags_build_the_polar_augment():
    T, H = pkg().train, pkg().hip_ops
    res = ["--TextArgs=none", "--resident_loader=True"]
    for mics in (1, 2):
        for norm in ([], ["--dataset_normalization=True"]):
            args = T.parse_args(res + ["--augment_rotate=0.5", "--phase=True", f"--n_mics={mics}", "--augment_freq_masks=1",
                                       "--augment_freq_width=4"] + norm)
            aug = T.augment_from_args(args, "cpu")
            assert aug.p_rot == 0.5 and aug.rot_polar == tuple(H.foa_polar(mics=mics)) and aug.rot_triples is None
            assert aug.table is None and aug.p_swap == 0.0 and (aug.freq_masks, aug.freq_width) == (1, 4)
            assert (aug.rot_mirror, aug.rot_zflip) == (True, True)
    # magnitudes alone are not covariant: still refused, and the message says what would work
    with pytest.raises(ValueError, match="feature_layout") as info:
        T.augment_from_args(T.parse_args(res + ["--augment_rotate=0.5"]), "cpu")
    assert "magnitudes alone" in str(info.value) and "--phase=True" in str(info.value)
    for extra, match in ((["--augment_rotate=0.5", "--phase=True", "--augment_swap=0.5"], "augment_swap"),
                         (["--augment_rotate=0.5", "--phase=True", "--n_mics=4"], "n_mics"),
                         (["--augment_rotate=1.5", "--phase=True"], "probability"),
                         (["--augment_rotate=0.5", "--phase=True", "--feature_layout=iv"], "phase"),
                         (["--augment_swap=0.5", "--phase=True", "--dataset_normalization=True"], "raw phase")):
        with pytest.raises(ValueError, match=match):
            T.augment_from_args(T.parse_args(res + extra), "cpu")
    with pytest.raises(ValueError, match="resident_loader"):
        T.augment_from_args(T.parse_args(["--TextArgs=none", "--augment_rotate=0.5", "--phase=True"]), "cpu")


def test_polar_stats_from_the_entries_of_normalize_dataset():
    T = pkg().train
    import torch
    assert T.polar_stats_from(None, "cpu") is None
    got = T.polar_stats_from((torch.tensor([2.5, 3.0]), torch.tensor([0.5, 1.5])), "cpu")
    assert got.dtype == torch.float32 and got.is_contiguous() and got.tolist() == [2.5, 3.0, 0.5, 1.5]
    with pytest.raises(ValueError):
        T.polar_stats_from((torch.tensor([2.5, 3.0]),), "cpu")


def test_the_tolerance_constant_is_four_times_the_measured_cpu_maximum_rounded_up():
    worst = P.measured_cpu_ratio()
    print("largest ratio of the fp32 restatement over the GPU tests' inputs:", worst)
    assert worst > 0.5                                                      # the restatement is fp32, not the reference again
    assert P.K == 2 ** math.ceil(math.log2(4 * worst))


def test_reference_marks_what_moves_as_bits_and_restates_itself():
    """Unrotated samples, pass channels, masked cells, zero rows and rows >= count are exact; the complex value read back
    from the fp32 restatement is within K * 2^-24 * Wt of z'; magnitudes >= 0, phases in [-pi, pi]."""
    name, si = "scalar_16x9x7", 2
    x, y, groups = P.inputs(name, si)
    stats = P.STATS[si]
    index = np.array([3, -1, 0, 5, 2, 6, 1])
    ox, oy = np.full((5,) + x.shape[1:], -7.5, np.float32), np.full((5,) + y.shape[1:], -7.5, np.float32)
    ref = P.gather_polar(x, y, index, 0, 4, ox, oy, seed=2, epoch=1, groups=groups, stats=stats, p_rot=0.5, n_fmask=1, f_max=3,
                         n_tmask=1, t_max=2, fill=-1.5, restate=True)
    flags = P.rotated_flags(2, 1, np.arange(4), 0.5)
    assert flags.any() and not flags.all()
    side = ref["x"]
    grouped = sorted(c for g in groups for c in g)
    passing = [c for c in range(x.shape[1]) if c not in grouped]
    for b, d in enumerate(ref["rows"]):
        if d is None:
            assert b == 1 and not side["ref"][b].any() and side["exact"][b].all() and not ref["y"]["ref"][b].any()
            continue
        assert d["rotate"] == bool(flags[b])
        assert side["exact"][b][passing].all()
        assert side["exact"][b][grouped].all() == (not d["rotate"])
        if d["rotate"]:
            masked = side["exact"][b][grouped[0]]
            assert (side["ref"][b][:, masked] == -1.5).all() and masked.any() and not masked.all()
    assert side["exact"][4].all() and (side["ref"][4] == -7.5).all() and (ref["y"]["ref"][4] == -7.5).all()
    assert P.bits_equal(side["f32"], side["ref"])[side["exact"]].all()
    assert 0 < P.error_ratio(side["f32"], side, groups, stats) <= P.K / 4
    _, M, Ph = P.complex_of(side["f32"], groups, stats)
    slack = 2.0 ** -23 * (np.abs(M) + abs(stats[0])), 2.0 ** -23 * (np.pi + abs(stats[2]))
    inexact = ~side["exact"]
    assert (M[inexact] >= -slack[0][inexact]).all() and (np.abs(Ph[inexact]) <= np.float64(np.float32(np.pi)) + slack[1]).all()


def _stft(sig, frame, hop):
    """Frame-wise rfft with a Hann window: (channels, frame // 2 + 1, frames) complex128."""
    starts = range(0, sig.shape[1] - frame + 1, hop)
    win = np.hanning(frame)
    return np.stack([np.fft.rfft(sig[:, s:s + frame] * win, axis=1) for s in starts], axis=-1)


def _orthogonal(rng, mirrored):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q)) * (-1 if mirrored else 1)


@pytest.mark.parametrize("order", ["WYZX", "XWZY"])
@pytest.mark.parametrize("mirrored", [False, True])
def test_magnitude_and_phase_are_covariant_as_one_complex_number(order, mirrored):
    """A random 4-channel signal, its X, Y, Z rotated by a general R in the TIME domain; magnitude and angle of the framed
    rfft of the rotated signal equal the reference's polar rotation of the unrotated signal's features, to 1e-9 on the
    complex value; W's features do not move."""
    H = pkg().hip_ops
    rng = np.random.default_rng(7 + mirrored)
    R = _orthogonal(rng, mirrored)
    assert np.linalg.det(R) * (-1 if mirrored else 1) > 0.99 and abs(R[2, 2]) < 0.999      # general: not about z
    sig = rng.standard_normal((4, 400))
    pos = [order.index(ch) for ch in "XYZ"]
    turned = sig.copy()
    turned[pos] = R @ sig[pos]
    spec, spec_r = _stft(sig, 64, 32), _stft(turned, 64, 32)
    feats = np.concatenate([np.abs(spec), np.angle(spec)])                  # [magnitude block | phase block], float64
    feats_r = np.concatenate([np.abs(spec_r), np.angle(spec_r)])
    groups = H.foa_polar(order)
    _, z, weight, exact = P.rotate_x(feats, R, groups)
    w = order.index("W")
    assert exact[[w, 4 + w]].all() and not exact[[c for g in groups for c in g]].any()
    assert np.array_equal(feats_r[[w, 4 + w]], feats[[w, 4 + w]])
    want, _, _ = P.complex_of(feats_r, groups, None)
    assert np.abs(z - want)[~exact].max() <= 1e-9
    assert np.abs(want[~exact]).max() > 1 and (weight[~exact] > 0).all()
