"""Host side of the augmented gather: the numpy reference (tests/loader_aug_ref.py), the transform preset
hip_ops.foa_transforms, the table validation and the --augment_* flags.  No GPU."""
import numpy as np
import pytest

from tests import loader_aug_ref as R
from tests.helpers import pkg


def _table_parts(table):
    C = (table.shape[1] - 6) // 2
    return C, table[:, :C], table[:, C:2 * C], table[:, 2 * C:2 * C + 3], table[:, 2 * C + 3:]


def test_reference_draws_depend_on_seed_epoch_and_position_only():
    """Twice the same draws for the same (seed, epoch, p); another seed, epoch or position gives other words; the three
    groups differ; the counter layout is the documented one (epoch above bit 34, p above bit 2)."""
    kw = dict(K=16, p_swap=0.5, n_fmask=2, f_max=5, F=11, n_tmask=2, t_max=7, T=40)
    assert R.draws(3, 1, 9, **kw) == R.draws(3, 1, 9, **kw)
    base = R.words(3, 1, 9, 0)
    assert base == R.words(3, 1, 9, 0)
    for other in (R.words(4, 1, 9, 0), R.words(3, 2, 9, 0), R.words(3, 1, 10, 0), R.words(3, 1, 9, 1), R.words(3, 1, 9, 2)):
        assert other != base
    counter = (1 << 34) | (9 << 2) | 2
    assert R.words(3, 1, 9, 2) == [int(w) for w in R.P.philox4x32_10(np.uint64(counter), np.uint64(3))[0]]
    # the loader's epoch before its first begin_epoch is -1: the counter wraps mod 2^64
    assert R.words(3, -1, 9, 0) == [int(w) for w in R.P.philox4x32_10(np.uint64((2 ** 64 - 2 ** 34) | (9 << 2)), np.uint64(3))[0]]


def test_reference_integers_and_masks_stay_in_range():
    for p in range(200):
        d = R.draws(11, 0, p, K=16, p_swap=0.5, n_fmask=2, f_max=5, F=5, n_tmask=1, t_max=0, T=9)
        assert d["k"] is None or 0 <= d["k"] < 16
        assert len(d["fmasks"]) == 2 and len(d["tmasks"]) == 1
        for first, width in d["fmasks"]:
            assert 0 <= width <= 5 and 0 <= first and first + width <= 5
        assert d["tmasks"][0][1] == 0                       # t_max = 0: always an empty mask
    assert R.int_below(0xFFFFFFFF, 16) == 15 and R.int_below(0, 16) == 0 and R.int_below(0x10000000, 16) == 1


@pytest.mark.parametrize("elevation, K", [(True, 16), (False, 8)])
@pytest.mark.parametrize("mics, phase", [(1, False), (2, False), (1, True), (2, True)])
def test_foa_transforms_gives_distinct_valid_rows(elevation, K, mics, phase):
    H = pkg().hip_ops
    table = H.foa_transforms(mics=mics, phase=phase, elevation=elevation)
    assert table.dtype == np.int32 and table.shape == (K, 2 * 4 * mics * (2 if phase else 1) + 6)
    C, src, flip, axis, sign = _table_parts(table)
    assert len({tuple(r) for r in table.tolist()}) == K
    assert len({tuple(r) for r in np.concatenate([axis, sign], 1).tolist()}) == K
    assert table[0].tolist() == list(range(C)) + [0] * C + [0, 1, 2, 1, 1, 1]         # the identity comes first
    assert (np.sort(src, axis=1) == np.arange(C)).all()                                # a permutation of the channels
    assert (np.sort(axis, axis=1) == np.arange(3)).all() and (np.abs(sign) == 1).all()
    assert (axis[:, 2] == 2).all()                                                     # z stays vertical
    assert elevation or (sign[:, 2] == 1).all()
    assert set(np.unique(flip)) <= ({0, 2} if phase else {0})
    assert (src // 4 == np.arange(C) // 4).all()                                       # every block maps into itself
    assert H.loader._check_table(table, C).shape == table.shape


@pytest.mark.parametrize("order", ["WYZX", "WXYZ"])
def test_preset_rows_transform_an_encoded_direction_like_its_label(order):
    """A plane wave from the unit direction d = (d_x, d_y, d_z) encodes as W = 1 and the directional channels d_axis (in
    the block's channel order).  For every preset row, moving the channels by src and negating where the sign is -1
    (flip 1) gives the encoding of the direction the row makes of the label: sign[a] * d[axis[a]]."""
    H = pkg().hip_ops
    table = H.foa_transforms(order=order)
    pos = [order.index(ch) for ch in "XYZ"]
    rng = np.random.default_rng(5)
    d = rng.standard_normal((6, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)

    def encode(direction):
        x = np.ones((4, 1, direction.shape[0]), dtype=np.float32)
        for a in range(3):
            x[pos[a], 0] = direction[:, a]
        return x
    for row in table:
        C, _, _, axis, sign = _table_parts(row[None])
        flips = [0] * 4
        for a in range(3):
            flips[pos[a]] = 1 if sign[0, a] < 0 else 0
        signed = np.concatenate([row[:4], np.asarray(flips, dtype=np.int32), row[8:]])
        label = np.concatenate([np.ones((6, 1), dtype=np.float32), d], axis=1)          # n_sed = 1: [activity | x y z]
        moved = R.transform_y(label, signed, 4)
        assert np.array_equal(moved[:, 0], label[:, 0])
        assert np.array_equal(moved[:, 1:], np.stack([np.float32(sign[0, a]) * d[:, axis[0, a]] for a in range(3)], 1))
        assert np.array_equal(R.transform_x(encode(d), signed), encode(moved[:, 1:]))


def test_phase_preset_turns_a_raw_phase_into_the_phase_of_the_negated_signal():
    """The phase half of the preset gets flip 2 exactly where the sign is -1, and flip 2 of angle(z) is angle(-z).

    flipop(2, v) is ONE fp32 addition of PI_F to the fp32 phase, while angle(-z) is the correctly rounded theta -+ pi:
    the two are fl(theta + d1 -+ PI_F) and fl(theta -+ pi) with |d1| <= ulp(theta) / 2 from rounding the phase and
    PI_F - pi = 8.74e-8.  They are the same float unless an fp32 rounding boundary lies between the two exact values,
    so: (a) for EVERY input they differ by at most |d1| + |PI_F - pi| + one rounding of the result, below
    2 ulp at pi = 4.8e-7; (b) bit for bit on the inputs whose exact theta -+ pi (in float64) is farther from every
    rounding boundary of its binade than |d1| + |PI_F - pi|, a criterion on the input alone.  Inputs with a phase within
    1e-3 of 0 or +-pi (the ties of the rule) are left out."""
    H = pkg().hip_ops
    table = H.foa_transforms(phase=True)
    C, src, flip, axis, sign = _table_parts(table)
    pos = ["WYZX".index(ch) for ch in "XYZ"]
    for row, fl in zip(table, flip):
        assert fl[:4].tolist() == [0] * 4 and fl[4] == 0
        for a in range(3):
            assert fl[4 + pos[a]] == (2 if row[2 * C + 3 + a] < 0 else 0)
    rng = np.random.default_rng(7)
    z = rng.standard_normal(4000) + 1j * rng.standard_normal(4000)
    theta = np.angle(z)                                       # float64
    keep = (np.abs(theta) > 1e-3) & (np.abs(np.abs(theta) - np.pi) > 1e-3)
    z, theta = z[keep], theta[keep]
    v = theta.astype(np.float32)
    want = np.angle(-z).astype(np.float32)
    got = R.flipop(2, v)
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 4.8e-7)
    exact = np.where(theta <= 0, theta + np.pi, theta - np.pi)
    shift = np.abs(v.astype(np.float64) - theta) + abs(float(R.PI_F) - np.pi)
    nearest = np.abs(exact).astype(np.float32)
    ulp = np.spacing(np.nextafter(nearest, np.float32(0))).astype(np.float64)     # the finer side at a power of two
    below = np.abs(exact) - np.abs(exact).astype(np.float32).astype(np.float64)        # distance to the nearest float
    to_boundary = ulp / 2 - np.abs(below)
    safe = to_boundary > shift + 1e-12
    assert safe.sum() > 200
    assert np.array_equal(got[safe], want[safe])
    # through a preset row: the x channel of the phase block under x -> -x
    row = table[1]
    assert row[2 * C + 3:].tolist() == [-1, 1, 1]
    x = np.zeros((8, 1, int(safe.sum())), dtype=np.float32)
    x[4 + pos[0], 0] = v[safe]
    assert np.array_equal(R.transform_x(x, row)[4 + pos[0], 0], want[safe])


def test_reference_gather_applies_transform_then_masks_and_zero_fills_invalid_rows():
    rng = np.random.default_rng(1)
    x_all = rng.standard_normal((4, 4, 5, 8)).astype(np.float32)
    y_all = rng.standard_normal((4, 3, 8)).astype(np.float32)
    table = pkg().hip_ops.foa_transforms()
    index = np.array([2, -1, 3, 0])
    ox, oy = np.full((5, 4, 5, 8), -7.5, np.float32), np.full((5, 3, 8), -7.5, np.float32)
    kw = dict(seed=5, epoch=0, table=table, p_swap=1.0, n_fmask=1, f_max=5, n_tmask=2, t_max=3, fill=0.25)
    gx, gy = R.gather_aug(x_all, y_all, index, 0, 4, ox, oy, **kw)
    assert not gx[1].any() and not gy[1].any()                              # invalid index: zeros, no fill value
    assert (gx[4] == -7.5).all() and (gy[4] == -7.5).all()                  # beyond count
    d = R.draws(5, 0, 2, 16, 1.0, 1, 5, 5, 2, 3, 8)
    want = R.transform_x(x_all[3], table[d["k"]])
    for first, width in d["fmasks"]:
        want[:, first:first + width] = 0.25
    for first, width in d["tmasks"]:
        want[:, :, first:first + width] = 0.25
    assert np.array_equal(gx[2], want) and np.array_equal(gy[2], R.transform_y(y_all[3], table[d["k"]], 4))
    again = R.gather_aug(x_all, y_all, index, 0, 4, ox, oy, **kw)
    assert np.array_equal(again[0], gx) and np.array_equal(again[1], gy)
    plain = R.gather_aug(x_all, y_all, index, 0, 4, ox, oy, seed=5, epoch=0)
    assert np.array_equal(plain[0][0], x_all[2]) and np.array_equal(plain[1][3], y_all[0])


def test_bad_tables_are_refused_before_any_upload():
    H, L = pkg().hip_ops, pkg()._lib
    good = H.foa_transforms()
    check = H.loader._check_table

    def changed(r, c, v):
        t = good.copy()
        t[r, c] = v
        return t
    for bad in (changed(0, 0, 4), changed(0, 1, -1), changed(3, 4, 3), changed(3, 5, -1), changed(2, 8, 1), changed(2, 9, 3),
                changed(5, 11, 0), changed(5, 12, 2), good[:, :-1], good[:0], np.concatenate([good] * 5), good.astype(np.float32),
                good[0], np.zeros((2, 2 * 17 + 6), dtype=np.int32)):
        with pytest.raises(L.SeldHipError):
            check(bad, None)
    with pytest.raises(L.SeldHipError):
        check(good, 8)
    for kwargs in (dict(p_swap=1.5), dict(p_swap=-0.1), dict(p_swap=float("nan")), dict(freq_masks=3), dict(time_masks=-1),
                   dict(freq_width=-1), dict(time_width=-2)):
        with pytest.raises(L.SeldHipError):
            H.Augment(**kwargs)
    off = H.Augment()
    assert off.table is None and off.transforms == 0 and off.channels is None
    with pytest.raises(Exception):
        off.p_swap = 0.5                                                    # frozen


def test_augment_flags_default_to_off_and_need_the_resident_loader():
    T = pkg().train
    off = T.parse_args(["--TextArgs=none"])
    assert (off.augment_swap, off.augment_freq_masks, off.augment_freq_width, off.augment_time_masks, off.augment_time_width,
            off.augment_seed) == (0.0, 0, 0, 0, 0, 0)
    assert not T.augment_requested(off) and T.augment_from_args(off, "cpu") is None
    for flag in ("--augment_swap=0.5", "--augment_freq_masks=1", "--augment_time_masks=2"):
        args = T.parse_args(["--TextArgs=none", flag])
        assert T.augment_requested(args)
        with pytest.raises(ValueError, match="resident_loader"):
            T.main(args)
        with pytest.raises(ValueError, match="resident_loader"):
            T.augment_from_args(args, "cpu")
    # standardised phase with sign flips stays out; raw phase and magnitudes alone pass the check
    args = T.parse_args(["--TextArgs=none", "--resident_loader=True", "--augment_swap=0.5", "--phase=True", "--input_channels=8"])
    with pytest.raises(ValueError, match="raw phase"):
        T.augment_from_args(args, "cpu")
    args = T.parse_args(["--TextArgs=none", "--resident_loader=True", "--augment_swap=0.5", "--phase=True",
                         "--dataset_normalization=False", "--augment_time_masks=1", "--augment_time_width=9", "--augment_seed=3"])
    aug = T.augment_from_args(args, "cpu")
    assert aug.transforms == 16 and aug.channels == 8 and aug.p_swap == 0.5 and (aug.time_masks, aug.time_width) == (1, 9)
    args = T.parse_args(["--TextArgs=none", "--resident_loader=True", "--augment_swap=0.25", "--n_mics=2"])
    assert T.augment_from_args(args, "cpu").channels == 8
