"""Host side of the rotated gather and of the intensity layouts: the tables hip_ops.foa_transforms(layout=...) against a
direct construction, hip_ops.foa_triples, every refusal of Augment / foa_transforms / train.augment_from_args, the numpy
reference tests/loader_rot_ref.py, and the covariance the whole feature rests on, in float64: the intensity features of
a sound field whose directional channels were mixed by R are R applied to the features.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import loader_rot_ref as R
from tests.helpers import pkg

AXES = "XYZ"
ORDERS = ["WYZX", "WXZY"]


def _roles(layout, order, mics, phase=False):
    """What every channel of a layout is: (kind, microphone, letter), kind in mag / phase / lp / iv."""
    if layout == "magphase":
        return [(kind, g, ch) for kind in (("mag", "phase") if phase else ("mag",)) for g in range(mics) for ch in order]
    if layout == "quaternion":
        return [("lp" if ch == "W" else "iv", g, ch) for g in range(mics) for ch in order]
    iv = [("iv", g, ch) for g in range(mics) for ch in order[1:]]
    return iv if layout == "iv" else [("lp", g, ch) for g in range(mics) for ch in order] + iv


def _signed_permutations(elevation):
    """(axis, sign) of the preset rows in their order: location'[a] = sign[a] * location[axis[a]]."""
    for swap, sz, sy, sx in itertools.product((False, True), (1, -1) if elevation else (1,), (1, -1), (1, -1)):
        yield ([1, 0, 2] if swap else [0, 1, 2]), [sx, sy, sz]


def _direct_table(layout, order, mics, phase, elevation):
    roles = _roles(layout, order, mics, phase)
    rows = []
    for axis, sign in _signed_permutations(elevation):
        src, flip = [], []
        for kind, g, ch in roles:
            if ch == "W":
                src.append(roles.index((kind, g, ch)))
                flip.append(0)
                continue
            a = AXES.index(ch)
            src.append(roles.index((kind, g, AXES[axis[a]])))
            flip.append(0 if sign[a] > 0 or kind in ("mag", "lp") else 1 if kind == "iv" else 2)
        rows.append(src + flip + axis + sign)
    return np.asarray(rows, dtype=np.int32)


@pytest.mark.parametrize("elevation", [True, False])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mics", [1, 2])
@pytest.mark.parametrize("layout", ["quaternion", "iv", "logpower_iv"])
def test_tables_of_the_intensity_layouts_equal_a_direct_construction(layout, mics, order, elevation):
    H = pkg().hip_ops
    table = H.foa_transforms(order=order, mics=mics, elevation=elevation, layout=layout)
    C = {"quaternion": 4, "iv": 3, "logpower_iv": 7}[layout] * mics
    assert table.dtype == np.int32 and table.shape == (16 if elevation else 8, 2 * C + 6)
    assert np.array_equal(table, _direct_table(layout, order, mics, False, elevation))
    assert table[0].tolist() == list(range(C)) + [0] * C + [0, 1, 2, 1, 1, 1]         # the identity comes first
    assert set(np.unique(table[:, C:2 * C])) <= {0, 1}
    assert H.loader._check_table(table, C).shape == table.shape
    # the (axis, sign) columns are those of the magnitude table, row for row
    assert np.array_equal(table[:, 2 * C:], H.foa_transforms(mics=mics, elevation=elevation)[:, 8 * mics:])


@pytest.mark.parametrize("mics, phase", [(1, False), (2, False), (1, True), (2, True)])
def test_magphase_layout_is_the_table_as_it_was(mics, phase):
    H = pkg().hip_ops
    for order in ("WYZX", "XWZY"):                                  # W anywhere: the magnitude layout never asked for it first
        for elevation in (True, False):
            table = H.foa_transforms(order, mics, phase, elevation)
            assert np.array_equal(table, H.foa_transforms(order=order, mics=mics, phase=phase, elevation=elevation, layout="magphase"))
            assert np.array_equal(table, _direct_table("magphase", order, mics, phase, elevation))


def test_foa_triples_values_and_refusals():
    H, L = pkg().hip_ops, pkg()._lib
    assert H.foa_triples() == [(3, 1, 2)]                           # W Y Z X: x is channel 3
    assert H.foa_triples("WXYZ", 2, "quaternion") == [(1, 2, 3), (5, 6, 7)]
    assert H.foa_triples("WYZX", 2, "iv") == [(2, 0, 1), (5, 3, 4)]
    assert H.foa_triples(order="wxzy", mics=1, layout="iv") == [(0, 2, 1)]
    for kw in (dict(layout="magphase"), dict(layout="logpower_iv"), dict(layout="mel"), dict(order="XWYZ"), dict(order="WXYY"),
               dict(mics=3), dict(mics=0)):
        with pytest.raises(L.SeldHipError):
            H.foa_triples(**kw)
    for kw in (dict(layout="mel"), dict(layout="quaternion", phase=True), dict(layout="iv", phase=True),
               dict(layout="logpower_iv", phase=True), dict(layout="quaternion", order="XWYZ"), dict(layout="iv", mics=3)):
        with pytest.raises(L.SeldHipError):
            H.foa_transforms(**kw)


def test_augment_rotation_fields_and_refusals():
    H, L = pkg().hip_ops, pkg()._lib
    off = H.Augment()
    assert (off.p_rot, off.rot_triples, off.rot_mirror, off.rot_zflip) == (0.0, None, True, True) and off.rot_channels is None
    aug = H.Augment(p_rot=0.25, rot_triples=[[5, 6, 7], (1, 2, 3)], rot_zflip=False)
    assert aug.rot_triples == ((5, 6, 7), (1, 2, 3)) and aug.rot_channels == 8 and aug.table is None
    assert aug.rot_packed == 0x321765
    assert H.Augment(rot_triples=np.array([[0, 1, 2]])).p_rot == 0.0           # triples alone: for explicit matrices
    five = [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(5)]
    assert H.Augment(p_rot=1.0, rot_triples=five).rot_channels == 15
    table = H.foa_transforms(layout="quaternion")
    bad = [dict(p_rot=1.5, rot_triples=five), dict(p_rot=-0.1, rot_triples=five), dict(p_rot=float("nan"), rot_triples=five),
           dict(p_rot=0.5), dict(p_rot=0.5, rot_triples=[]), dict(p_rot=0.5, rot_triples=[(1, 2)]), dict(rot_triples=[(1, 2, 2)]),
           dict(rot_triples=[(1, 2, 3), (3, 4, 5)]), dict(rot_triples=[(1, 2, 16)]), dict(rot_triples=[(-1, 2, 3)]),
           dict(rot_triples=[(0.0, 1.0, 2.0)]), dict(rot_triples=five + [(15, 16, 17)]), dict(rot_triples=(1, 2, 3)),
           dict(p_rot=0.5, rot_triples=[(1, 2, 3)], p_swap=0.5, table=table)]
    for kw in bad:
        with pytest.raises(L.SeldHipError):
            H.Augment(**kw)                                                    # device="cuda" by default: nothing was uploaded
    with pytest.raises(Exception):
        aug.p_rot = 0.5                                                        # frozen


def test_train_flags_for_layouts_and_rotation():
    T = pkg().train
    base = ["--TextArgs=none"]
    off = T.parse_args(base)
    assert (off.feature_layout, off.augment_rotate) == ("magphase", 0.0) and not T.augment_requested(off)
    rot = T.parse_args(base + ["--augment_rotate=0.5"])
    assert T.augment_requested(rot)
    for call in (lambda: T.main(rot), lambda: T.augment_from_args(rot, "cpu")):
        with pytest.raises(ValueError, match="resident_loader"):
            call()
    res = base + ["--resident_loader=True"]
    for extra, match in ((["--augment_rotate=0.5"], "feature_layout"),
                         (["--augment_rotate=0.5", "--feature_layout=logpower_iv"], "feature_layout"),
                         (["--augment_rotate=0.5", "--feature_layout=mel"], "feature_layout"),
                         (["--augment_rotate=1.5", "--feature_layout=iv"], "probability"),
                         (["--augment_rotate=0.5", "--feature_layout=iv", "--augment_swap=0.5"], "augment_swap"),
                         (["--augment_rotate=0.5", "--feature_layout=iv", "--phase=True"], "phase"),
                         (["--augment_rotate=0.5", "--feature_layout=iv", "--n_mics=4"], "n_mics"),
                         (["--augment_swap=0.5", "--feature_layout=mel"], "feature_layout"),
                         (["--augment_swap=0.5", "--feature_layout=quaternion", "--phase=True"], "phase")):
        with pytest.raises(ValueError, match=match):
            T.augment_from_args(T.parse_args(res + extra), "cpu")
    aug = T.augment_from_args(T.parse_args(res + ["--augment_rotate=0.5", "--feature_layout=quaternion", "--n_mics=2",
                                                  "--augment_time_masks=1", "--augment_time_width=9"]), "cpu")
    assert aug.p_rot == 0.5 and aug.rot_triples == ((3, 1, 2), (7, 5, 6)) and aug.table is None and aug.p_swap == 0.0
    assert (aug.time_masks, aug.time_width, aug.rot_mirror, aug.rot_zflip) == (1, 9, True, True)
    aug = T.augment_from_args(T.parse_args(res + ["--augment_rotate=1", "--feature_layout=iv"]), "cpu")
    assert aug.rot_triples == ((2, 0, 1),)
    H = pkg().hip_ops
    for layout, C in (("quaternion", 8), ("iv", 6), ("logpower_iv", 14), ("magphase", 8)):
        aug = T.augment_from_args(T.parse_args(res + ["--augment_swap=0.5", f"--feature_layout={layout}", "--n_mics=2"]), "cpu")
        assert aug.channels == C and aug.p_rot == 0.0 and aug.rot_triples is None
        assert np.array_equal(aug.table.numpy(), H.foa_transforms(mics=2, layout=layout))
        ens = T.ensemble_from_args(T.parse_args(base + ["--test_tta=8", f"--feature_layout={layout}", "--n_mics=2"]))
        assert np.array_equal(ens["table"], H.foa_transforms(mics=2, layout=layout, elevation=False))
    for extra, match in ((["--test_tta=16", "--feature_layout=mel"], "feature_layout"),
                         (["--test_tta=16", "--feature_layout=iv", "--phase=True"], "phase")):
        with pytest.raises(ValueError, match=match):
            T.ensemble_from_args(T.parse_args(base + extra))
    # the layout alone asks for nothing
    assert T.augment_from_args(T.parse_args(res + ["--feature_layout=iv"]), "cpu") is None
    assert T.ensemble_from_args(T.parse_args(base + ["--feature_layout=iv"])) is None


def test_reference_rotations_are_yaws_with_mirrors_drawn_from_group_three():
    seen = set()
    for p in range(64):
        d = R.rotation(7, 1, p, 0.5)
        w = R.words(7, 1, p, 3)
        assert d["rotate"] == bool(np.float32(w[1] >> 8) * np.float32(2.0 ** -24) < np.float32(0.5))
        assert d["t"] == np.float32(2) * (np.float32(w[0] >> 8) * np.float32(2.0 ** -24)) and 0 <= d["t"] < 2
        assert (d["mirror"], d["zflip"]) == (bool(w[2] >> 31), bool(w[3] >> 31))
        M = d["R"]
        assert np.allclose(M @ M.T, np.eye(3), atol=1e-15)
        assert np.isclose(np.linalg.det(M), (-1.0 if d["mirror"] else 1.0) * (-1.0 if d["zflip"] else 1.0))
        assert M[2].tolist() == [0.0, 0.0, -1.0 if d["zflip"] else 1.0] and M[0, 1] == -np.sin(np.pi * np.float64(d["t"]))
        seen.add((d["rotate"], d["mirror"], d["zflip"]))
        off = R.rotation(7, 1, p, 0.5, rot_mirror=False, rot_zflip=False)
        assert not off["mirror"] and not off["zflip"] and np.isclose(np.linalg.det(off["R"]), 1.0)
    assert len(seen) == 8
    assert np.array_equal(R.rotated_flags(7, 1, np.arange(64), 0.5), [R.rotation(7, 1, p, 0.5)["rotate"] for p in range(64)])
    assert np.array_equal(R.rotated_flags(7, -1, np.arange(8), 0.5), [R.rotation(7, -1, p, 0.5)["rotate"] for p in range(8)])
    assert not R.rotated_flags(7, 1, np.arange(64), 0.0).any() and R.rotated_flags(7, 1, np.arange(64), 1.0).all()


def test_reference_gather_marks_what_moves_as_bits():
    rng = np.random.default_rng(2)
    x_all = rng.standard_normal((3, 4, 3, 5)).astype(np.float32)
    y_all = rng.standard_normal((3, 2, 8)).astype(np.float32)
    M = rng.standard_normal((4, 9)).astype(np.float32)
    ox, oy = np.full((5, 4, 3, 5), -7.5, np.float32), np.full((5, 2, 8), -7.5, np.float32)
    g = R.gather_rot(x_all, y_all, np.array([2, -1, 0, 1]), 0, 4, ox, oy, seed=1, epoch=0, triples=[(3, 1, 2)], matrices=M,
                     n_fmask=1, f_max=2, n_tmask=1, t_max=2, fill=0.5)
    assert g["rows"][1] is None and not g["x"]["ref"][1].any() and not g["y"]["ref"][1].any()
    assert (g["x"]["ref"][4] == -7.5).all() and g["x"]["exact"][4].all() and g["x"]["exact"][1].all()
    assert g["x"]["exact"][0, 0].all() and np.array_equal(g["x"]["ref"][0, 0][~(g["x"]["ref"][0, 0] == 0.5)],
                                                          x_all[2, 0][~(g["x"]["ref"][0, 0] == 0.5)].astype(np.float64))
    assert g["y"]["exact"][0, :, :2].all() and not g["y"]["exact"][0, :, 2:].any()
    M0 = M[0].astype(np.float64).reshape(3, 3)
    free = ~g["x"]["exact"][0, 3]                                               # not masked
    assert free.any() and np.allclose(g["x"]["ref"][0, 3][free], (M0[0, 0] * x_all[2, 3] + M0[0, 1] * x_all[2, 1] + M0[0, 2] * x_all[2, 2])[free])
    assert np.allclose(g["y"]["ref"][0, 1, 2 + 3 + 1], M0[1] @ y_all[2, 1, 5:8].astype(np.float64))
    assert (g["x"]["weight"][g["x"]["exact"]] == 0).all() and (g["x"]["weight"][~g["x"]["exact"]] >= 0).all()


# ---- covariance ---------------------------------------------------------------------------------------------------------
def _spectra(signal, nperseg=32, hop=16):
    """Framed rfft spectra (channels, bins, frames) of a (channels, L) signal, Hann window."""
    frames = 1 + (signal.shape[1] - nperseg) // hop
    idx = np.arange(nperseg)[None, :] + hop * np.arange(frames)[:, None]
    return np.fft.rfft(signal[:, idx] * np.hanning(nperseg), axis=-1).transpose(0, 2, 1)


def _features(Z, fb, eps=1e-10):
    """(lp (4, bands, frames), iv (3, bands, frames)) of one group [W, D1, D2, D3] by the formulas of include/seld_hip.h."""
    p = np.abs(Z) ** 2
    E = eps + p[0] + (p[1] + p[2] + p[3]) / 3
    i = np.real(np.conj(Z[:1]) * Z[1:]) / E
    if fb is not None:
        p, i = np.einsum('mk,ckt->cmt', fb, p), np.einsum('mk,ckt->cmt', fb, i)
    return np.log(p + eps), i


def _layout(lp, iv, layout):
    return {"quaternion": np.concatenate([lp[:1], iv]), "iv": iv, "logpower_iv": np.concatenate([lp, iv])}[layout]


def _mixed(signal, order, M):
    """The recording of the sound field turned by M (xyz): the directional channels, taken in x, y, z order, mixed by M."""
    pos = [order.index(ch) for ch in AXES]
    out = signal.copy()
    out[pos] = M @ signal[pos]
    return out


def _small_filterbank(bins, bands=5):
    centres = np.linspace(1, bins - 2, bands)
    return np.maximum(0.0, 1.0 - np.abs(np.arange(bins)[None, :] - centres[:, None]) / 3.0)


@pytest.mark.parametrize("with_fb", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_intensity_features_are_covariant_under_rotations_of_the_sound_field(order, with_fb):
    """float64, numpy only.  A general yaw with mirror and z-flip, drawn by the reference: features(mixed signal) equal the
    reference's rotate_x of features(signal) over hip_ops.foa_triples(order), to 1e-9, on the quaternion and the iv layout;
    the log-power of W does not move.  This pins which channel is which axis and the sign conventions of R."""
    H = pkg().hip_ops
    rng = np.random.default_rng(11)
    signal = rng.standard_normal((4, 400))
    signal[1:] += 0.8 * signal[:1] * np.array([[0.3], [-0.5], [0.7]])        # a definite direction
    fb = _small_filterbank(17) if with_fb else None
    p = next(p for p in range(64) if all(R.rotation(3, 0, p, 1.0)[k] for k in ("mirror", "zflip")))
    M = R.rotation(3, 0, p, 1.0)["R"]
    assert abs(M[0, 1]) > 0.05 and abs(M[0, 0]) > 0.05 and np.isclose(np.linalg.det(M[:2, :2]), -1) and M[2, 2] == -1
    lp, iv = _features(_spectra(signal), fb)
    lp_m, iv_m = _features(_spectra(_mixed(signal, order, M)), fb)
    assert np.abs(iv).max() > 0.05
    for layout in ("quaternion", "iv"):
        triples = H.foa_triples(order, 1, layout)
        want, _, _, exact = R.rotate_x(_layout(lp, iv, layout), M, triples)
        got = _layout(lp_m, iv_m, layout)
        assert np.abs(got - want).max() <= 1e-9
        assert exact.sum() == (want[0].size if layout == "quaternion" else 0)
        assert np.abs(got - _layout(lp, iv, layout)).max() > 1e-3           # and it did move
    # per axis: component a of the turned field is sum_b M[a][b] component b, component a living at order.index(axis) - 1
    comp = [order.index(ch) - 1 for ch in AXES]
    for a in range(3):
        assert np.abs(iv_m[comp[a]] - sum(M[a, b] * iv[comp[b]] for b in range(3))).max() <= 1e-9


@pytest.mark.parametrize("order", ORDERS)
def test_table_rows_of_every_intensity_layout_are_the_features_of_the_permuted_field(order):
    """Every row of the 16-row preset, on all three layouts: moving the channels by src and negating where flip is 1 gives
    the features of the signal whose directional channels were mixed by the row's signed permutation matrix."""
    H = pkg().hip_ops
    rng = np.random.default_rng(12)
    signal = rng.standard_normal((4, 200))
    lp, iv = _features(_spectra(signal), _small_filterbank(17))
    for layout in ("quaternion", "iv", "logpower_iv"):
        table = H.foa_transforms(order=order, layout=layout)
        C = (table.shape[1] - 6) // 2
        x = _layout(lp, iv, layout)
        for row in table:
            M = np.zeros((3, 3))
            for a in range(3):
                M[a, row[2 * C + a]] = row[2 * C + 3 + a]
            got = np.stack([(-1.0 if row[C + c] == 1 else 1.0) * x[row[c]] for c in range(C)])
            want = _layout(*_features(_spectra(_mixed(signal, order, M)), _small_filterbank(17)), layout)
            assert np.abs(got - want).max() <= 1e-9
