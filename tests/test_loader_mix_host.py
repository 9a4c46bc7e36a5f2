"""Host side of the gather that mixes two clips: Augment(p_mix=...), the flags of train.augment_from_args, the tolerance
constant of the GPU tests, the merge rule of the targets, the occupancy table, and the fact the whole feature rests on, in
float64: magnitude and phase of the STFT of a + g b are the polar form of the sum of the two complex spectra.  No GPU."""
import math

import numpy as np
import pytest

from tests import loader_mix_ref as M
from tests.helpers import pkg
from tests.labels_helpers import encode_numpy

f32 = np.float32


def test_the_tolerance_constant_is_four_times_the_measured_cpu_maximum_rounded_up():
    worst = M.measured_cpu_ratio()
    print("largest ratio of the fp32 restatement over the GPU tests' inputs:", worst)
    assert worst > 0.5                                                      # the restatement is fp32, not the reference again
    assert M.K == 2 ** math.ceil(math.log2(4 * worst))


def _stft(sig, frame, hop):
    """Frame-wise rfft with a Hann window: (channels, frame // 2 + 1, frames) complex128."""
    starts = range(0, sig.shape[1] - frame + 1, hop)
    win = np.hanning(frame)
    return np.stack([np.fft.rfft(sig[:, s:s + frame] * win, axis=1) for s in starts], axis=-1)


@pytest.mark.parametrize("g", [0.5, 0.8125, 1.0])
def test_the_stft_of_a_mixture_is_the_reference_mix_of_the_magnitude_phase_arrays(g):
    """Two random 4-channel signals a and b: magnitude and angle of the framed rfft of a + g b equal the reference's mix of
    the features of a and of b, to 1e-9 on the complex value, W included."""
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((4, 400)), rng.standard_normal((4, 400))
    feats = [np.concatenate([np.abs(s), np.angle(s)]) for s in (_stft(a, 64, 32), _stft(b, 64, 32), _stft(a + g * b, 64, 32))]
    _, z, weight, exact = M.mix_x(feats[0], feats[1], g)
    want, _, _ = M.complex_of(feats[2], None)
    assert not exact.any() and z.shape == feats[0].shape
    assert np.abs(z - want).max() <= 1e-9 and np.abs(want).max() > 1 and (weight > 0).all()


def _row(activity, overlaps, seed=0):
    """One frame (1, 4 * n_sed) with the given activities and locations that are nowhere 0."""
    n_sed = len(activity)
    loc = np.random.default_rng(seed).uniform(0.1, 1.0, 3 * n_sed)
    return np.concatenate([np.asarray(activity, dtype=f32), loc.astype(f32)])[None]


def _slot(y, s):
    n_sed = y.shape[-1] // 4
    return (float(y[0, s]),) + tuple(float(v) for v in y[0, n_sed + 3 * s:n_sed + 3 * s + 3])


def test_merge_rule_cases():
    O = 3
    empty, full = _row([0, 0, 0, 0, 0, 0], O, 1), _row([1, 0.75, 1, 0, 1, 0], O, 2)
    for ya, yb in ((empty, full), (full, empty)):                           # empty + full: full's events, packed, in slot order
        out = M.merge_targets(ya, yb, O)
        assert [_slot(out, s) for s in (0, 1, 2, 3)] == [_slot(full, s) for s in (0, 1, 2, 4)]
        assert _slot(out, 4) == _slot(out, 5) == (0.0, 0.0, 0.0, 0.0) and not np.signbit(out).any()
    one, two = _row([0, 0, 1, 0, 0, 0], O, 3), _row([1, 0, 0.75, 0, 0, 0], O, 4)      # 1 + 2 at O = 3: A's, then B's, non-prefix slots
    out = M.merge_targets(one, two, O)
    assert [_slot(out, s) for s in range(3)] == [_slot(one, 2), _slot(two, 0), _slot(two, 2)]
    assert not out[0, 3:6].any() and not out[0, 6 + 9:].any()               # the other class stays empty, locations included
    out = M.merge_targets(two, two, O)                                      # 2 + 2: the fourth entry is dropped
    assert [_slot(out, s) for s in range(3)] == [_slot(two, 0), _slot(two, 2), _slot(two, 0)]
    nan = _row([np.nan, 1, 0, 0.5, 0.501, np.nan], O, 5)                    # a NaN and exactly 0.5 are inactive
    out = M.merge_targets(nan, nan, O)
    assert [_slot(out, s) for s in range(6)] == [_slot(nan, 1), _slot(nan, 1), (0.0,) * 4, _slot(nan, 4), _slot(nan, 4), (0.0,) * 4]
    assert not np.isnan(out).any()
    assert M.occupancy(np.stack([nan, full, empty]), O).tolist() == [[1, 1], [3, 1], [0, 0]]
    assert M.occupancy(np.stack([nan, full, empty]), 2).tolist() == [[1, 0, 1], [2, 1, 1], [0, 0, 0]]


@pytest.mark.parametrize("overlaps", [2, 3])
def test_merging_two_encoded_event_lists_is_encoding_the_concatenated_list(overlaps):
    """Targets as csv_to_matrix_task2 makes them (tests/labels_helpers.encode_numpy) of two event lists, merged, against the
    encoding of list A followed by list B: equal wherever nothing overflows (and there the first events are kept)."""
    rng = np.random.default_rng(11 + overlaps)
    frames, classes = 40, 4

    def events(n):
        first = rng.integers(0, frames - 1, n)
        return first, np.minimum(first + rng.integers(0, 12, n), frames - 1), rng.integers(0, classes, n), rng.uniform(-2, 2, (n, 3))
    a, b = events(9), events(8)
    ya, over_a = encode_numpy(*a, frames, classes, overlaps)
    yb, _ = encode_numpy(*b, frames, classes, overlaps)
    both, overflowing = encode_numpy(*(np.concatenate([u, v]) for u, v in zip(a, b)), frames, classes, overlaps)
    assert overflowing > over_a >= 0                                        # the case has cells that overflow only when mixed
    got = M.merge_targets(ya.astype(f32), yb.astype(f32), overlaps)
    assert np.array_equal(got, both.astype(f32))
    occ = M.occupancy(np.stack([ya, yb]).astype(f32), overlaps)
    assert not M.fits(occ, 0, 1, overlaps)                                  # and the occupancy test would not have mixed these two
    few = events(2)
    yf, _ = encode_numpy(*few, frames, classes, overlaps)
    occ = M.occupancy(np.stack([yf, yf]).astype(f32), overlaps)
    if M.fits(occ, 0, 1, overlaps):
        merged = M.merge_targets(yf.astype(f32), yf.astype(f32), overlaps)
        assert M.active(merged, overlaps).sum() == 2 * M.active(yf.astype(f32), overlaps).sum()      # nothing was dropped


def test_occupancy_reference_against_a_plain_loop():
    for overlaps in (2, 3):
        y = M.targets(7, overlaps)
        occ = M.occupancy(y, overlaps)
        assert occ.dtype == np.uint8 and occ.shape == (7, 6 // overlaps)
        for r in range(7):
            for c in range(6 // overlaps):
                counts = [sum(1 for o in range(overlaps) if y[r, fr, c * overlaps + o] > 0.5) for fr in range(y.shape[1])]
                assert occ[r, c] == max(counts) == M._EVENTS[overlaps][r][c]
        assert np.isnan(y).any() and occ.max() == overlaps and occ.min() == 0


def test_the_drawn_test_mixes_and_refuses():
    """Over the drawn test of the GPU suite (every number of rows of its cases, both overlaps, both epochs) the reference
    alone: partners are never the sample itself, gains lie in the range, at least a quarter of the drawn samples are mixed
    and at least one is refused for occupancy; the epochs draw differently."""
    for n in sorted({shape[0] for shape, _, _ in M.CASES.values()}):
        for overlaps in (2, 3):
            per_epoch = [M.drawn_rows(n, overlaps, e) for e in M.DRAWN["epochs"]]
            rows = [d for rows in per_epoch for d in rows]
            drawn = [d for d in rows if d["p2"] >= 0]
            assert all(d["p2"] != p for rows_ in per_epoch for p, d in enumerate(rows_))
            assert all(M.DRAWN["mix_gain"][0] <= d["g"] <= M.DRAWN["mix_gain"][1] for d in drawn)
            mixed, refused = sum(d["mixed"] for d in rows), sum(d["refused"] for d in rows)
            assert 0 < len(drawn) < len(rows) and mixed + refused == len(drawn)
            assert 4 * mixed >= len(drawn) and refused >= 1, (n, overlaps, len(drawn), mixed, refused)
            assert [d["p2"] for d in per_epoch[0]] != [d["p2"] for d in per_epoch[1]]


def test_reference_marks_what_moves_as_bits_and_restates_itself():
    name, si = "scalar_16x9x7", 2
    x, stats = M.inputs(name, si), M.STATS[si]
    y = M.targets(x.shape[0], 3)
    index = np.array([3, -1, 0, 5, 2, 4, 1])
    ox, oy = np.full((5,) + x.shape[1:], -7.5, f32), np.full((5,) + y.shape[1:], -7.5, f32)
    ref = M.gather_mix(x, y, index, 0, 4, ox, oy, seed=2, epoch=1, overlaps=3, stats=stats, partners=[2, 0, -1, 1], gains=[0.5, 1, 1, 0.75],
                       n_fmask=1, f_max=3, n_tmask=1, t_max=2, fill=-1.5, restate=True)
    side = ref["x"]
    assert [None if d is None else d["mixed"] for d in ref["rows"]] == [True, None, False, False]      # partner position 1 is invalid
    assert not side["ref"][1].any() and side["exact"][1].all() and not ref["y"][1].any()
    assert side["exact"][2].all() and side["exact"][3].all() and np.array_equal(ref["y"][2].view(np.uint32), y[0].view(np.uint32))
    masked = side["exact"][0]
    assert masked.any() and not masked.all() and (side["ref"][0][masked] == -1.5).all()
    assert side["exact"][4].all() and (side["ref"][4] == -7.5).all() and (ref["y"][4] == -7.5).all()
    assert np.array_equal(ref["y"][0].view(np.uint32), M.merge_targets(y[3], y[0], 3).view(np.uint32))
    assert M.bits_equal(side["f32"], side["ref"])[side["exact"]].all()
    assert 0 < M.error_ratio(side["f32"], side, stats) <= M.K / 4


def test_augment_mix_fields_and_refusals():
    H, L = pkg().hip_ops, pkg()._lib
    off = H.Augment()
    assert (off.p_mix, off.mix_gain, off.kind) == (0.0, (0.5, 1.0), "swap")
    aug = H.Augment(p_mix=0.25, mix_gain=[0.25, 2], freq_masks=2, freq_width=4, time_masks=1, time_width=3, fill=-1.0)
    assert aug.kind == "mix" and aug.mix_gain == (0.25, 2.0) and aug.table is None and (aug.freq_masks, aug.time_masks) == (2, 1)
    assert H.Augment(p_mix=1.0, mix_gain=(1, 1)).kind == "mix"
    # the other kinds are what they were
    assert H.Augment(p_rot=0.5, rot_polar=H.foa_polar()).kind == "polar" and H.Augment(p_rot=0.5, rot_triples=[(1, 2, 3)]).kind == "rot"
    assert H.Augment(rot_polar=H.foa_polar(), p_mix=0.5).kind == "mix"      # groups alone transform nothing
    bad = [dict(p_mix=1.5), dict(p_mix=-0.1), dict(p_mix=float("nan")), dict(p_mix=0.5, mix_gain=(0, 1)), dict(p_mix=0.5, mix_gain=(1, 0.5)),
           dict(mix_gain=(0.5, float("inf"))), dict(mix_gain=(float("nan"), 1)), dict(mix_gain=0.5), dict(mix_gain=(0.5, 1, 2)),
           dict(p_mix=0.5, p_rot=0.5, rot_polar=H.foa_polar()), dict(p_mix=0.5, p_rot=0.5, rot_triples=[(1, 2, 3)]),
           dict(p_mix=0.5, p_swap=0.5, table=H.foa_transforms(phase=True))]
    for kw in bad:
        with pytest.raises(L.SeldHipError):
            H.Augment(**kw)


def test_train_flags_build_the_mix_augment():
    T = pkg().train
    res = ["--TextArgs=none", "--resident_loader=True"]
    args = T.parse_args(res)
    assert (args.augment_mix, args.augment_mix_gain_lo, args.augment_mix_gain_hi) == (0.0, 0.5, 1.0)
    assert not T.augment_requested(args) and T.augment_from_args(args, "cpu") is None
    for norm in ([], ["--dataset_normalization=True"]):
        args = T.parse_args(res + ["--augment_mix=0.5", "--phase=True", "--augment_mix_gain_lo=0.25", "--augment_freq_masks=1",
                                   "--augment_freq_width=4"] + norm)
        aug = T.augment_from_args(args, "cpu")
        assert aug.kind == "mix" and aug.p_mix == 0.5 and aug.mix_gain == (0.25, 1.0) and (aug.freq_masks, aug.freq_width) == (1, 4)
        assert aug.table is None and aug.p_swap == 0.0 and aug.p_rot == 0.0
    with pytest.raises(ValueError, match="not linear") as info:
        T.augment_from_args(T.parse_args(res + ["--augment_mix=0.5"]), "cpu")
    assert "--phase=True" in str(info.value) and "magnitudes alone" in str(info.value)
    for extra, match in ((["--augment_mix=0.5", "--phase=True", "--augment_rotate=0.5"], "augment_rotate"),
                         (["--augment_mix=0.5", "--phase=True", "--augment_swap=0.5"], "augment_swap"),
                         (["--augment_mix=0.5", "--feature_layout=iv"], "not linear"),
                         (["--augment_mix=0.5", "--feature_layout=quaternion"], "intensity vectors"),
                         (["--augment_mix=1.5", "--phase=True"], "probability"),
                         (["--augment_mix=-0.5", "--phase=True"], "probability"),
                         (["--augment_mix=0.5", "--phase=True", "--augment_mix_gain_lo=0"], "gain"),
                         (["--augment_mix=0.5", "--phase=True", "--augment_mix_gain_lo=2"], "gain"),
                         (["--augment_mix=0.5", "--phase=True", "--class_overlaps=9"], "class_overlaps")):
        with pytest.raises(ValueError, match=match):
            T.augment_from_args(T.parse_args(res + extra), "cpu")
    with pytest.raises(ValueError, match="resident_loader"):
        T.augment_from_args(T.parse_args(["--TextArgs=none", "--augment_mix=0.5", "--phase=True"]), "cpu")
