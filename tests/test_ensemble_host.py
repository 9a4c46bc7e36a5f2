"""Host side of whole-recording inference: names and signatures, the two entry points in the header and the library, every
documented refusal (nothing is launched, so dummy pointers do), window_count, and the numpy reference
(tests/ensemble_ref.py) against hand-worked cases and on the inputs of tests/test_gpu_ensemble.py.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import ensemble_ref as E
from tests.helpers import pkg

EINVAL, EUNSUPPORTED = -1, -4
NULL = ctypes.c_void_p(0)
SOME = ctypes.c_void_p(64)              # never dereferenced: every call here is refused before any launch


def test_public_names_and_signatures():
    H, T = pkg().hip_ops, pkg().train
    assert H.window_batch is H.ensemble.window_batch and H.ensemble_combine is H.ensemble.ensemble_combine
    assert H.window_count is H.ensemble.window_count

    def params(fn):
        return [(n, p.kind, p.default) for n, p in inspect.signature(fn).parameters.items()]
    PK, KW, none = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    assert params(H.window_batch) == [("x", PK, none), ("out", PK, none), ("seg_len", KW, none), ("hop", KW, none),
                                      ("segments", KW, none), ("table", KW, None), ("first", KW, 0), ("count", KW, None)]
    assert params(H.ensemble_combine) == [("sed", PK, none), ("doa", PK, none), ("recordings", KW, none), ("segments", KW, none),
                                          ("hop_out", KW, none), ("frames", KW, none), ("classes", KW, 14), ("overlaps", KW, 3),
                                          ("table", KW, None), ("window", KW, "triangular"), ("align", KW, True),
                                          ("return_perm", KW, False)]
    assert params(H.window_count) == [("length", PK, none), ("seg_len", PK, none), ("hop", PK, none)]
    assert params(T.predict_recordings) == [("model", PK, none), ("x", PK, none), ("seg_len", KW, none), ("hop", KW, none),
                                            ("table", KW, None), ("window", KW, "triangular"), ("align", KW, True),
                                            ("batch", KW, 32), ("frames", KW, None)]
    got = params(T.evaluate_recordings)
    assert got[:5] == [("model", PK, none), ("device", PK, none), ("x_all", PK, none), ("y_all", PK, none), ("args", PK, none)]
    assert got[5:8] == [("hop", KW, none), ("table", KW, none), ("epoch", KW, 0)] and all(k == KW for _, k, _ in got[8:])


def test_header_declares_and_library_exports_both_entry_points():
    L = pkg()._lib
    with open(L.HEADER_PATH) as f:
        declared = L.prototypes(f.read())
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert declared["seld_window_batch"] == (ctypes.c_int, [ptr, i64, i32, i32, i32, i32, i32, i32, ptr, i32, i64, i32, i32, ptr, ptr])
    assert declared["seld_ensemble_combine"] == (ctypes.c_int, [ptr, ptr, i64, i32, i32, i32, i32, i32, i32, i32, ptr, ptr, i32,
                                                               i32, ptr, ptr, ptr, ptr])
    lib = L.lib()
    for name in ("seld_window_batch", "seld_ensemble_combine"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == declared[name][1]


def _window(lib, x=SOME, out=SOME, R=2, C=8, F=4, L=64, T=16, hop=8, S=7, table=SOME, K=16, m0=0, B=4, count=4):
    return lib.seld_window_batch(x, R, C, F, L, T, hop, S, table, K, m0, B, count, out, NULL)


def _combine(lib, sed=SOME, doa=SOME, R=2, S=4, K=16, T_out=8, hop_out=4, frames=19, classes=14, overlaps=3, win=SOME,
             table=SOME, C=8, align=1, out_sed=SOME, out_doa=SOME, perm=NULL):
    return lib.seld_ensemble_combine(sed, doa, R, S, K, T_out, hop_out, frames, classes, overlaps, win, table, C, align,
                                     out_sed, out_doa, perm, NULL)


def test_window_batch_refuses_without_launching():
    lib = pkg()._lib.lib()
    for kw in (dict(x=NULL), dict(out=NULL), dict(R=0), dict(R=-1), dict(C=0), dict(C=17), dict(F=0), dict(L=0), dict(T=0),
               dict(hop=0), dict(hop=-8), dict(S=0), dict(B=0), dict(count=0), dict(count=5), dict(B=70000, count=65536),
               dict(K=65), dict(K=-1), dict(table=NULL), dict(K=0), dict(m0=-1), dict(m0=2 * 7 * 16 - 3),
               dict(K=0, table=NULL, m0=2 * 7 - 3)):
        assert _window(lib, **kw) == EINVAL, kw
    assert _window(lib, C=16, F=1 << 14, T=1 << 13) == EUNSUPPORTED              # a row of 2^31 floats
    assert _window(lib, C=16, F=1 << 14, L=1 << 13) == EUNSUPPORTED


def test_ensemble_combine_refuses_without_launching():
    lib = pkg()._lib.lib()
    for kw in (dict(sed=NULL), dict(doa=NULL), dict(win=NULL), dict(out_sed=NULL), dict(out_doa=NULL), dict(R=0), dict(S=0),
               dict(T_out=0), dict(hop_out=0), dict(frames=0), dict(classes=0), dict(overlaps=0), dict(overlaps=-1),
               dict(K=65), dict(K=-1), dict(table=NULL), dict(K=0), dict(C=0), dict(C=17), dict(align=2), dict(align=-1)):
        assert _combine(lib, **kw) == EINVAL, kw
    assert _combine(lib, classes=13, overlaps=5, align=0) == EUNSUPPORTED       # n = 65 > 64
    assert _combine(lib, classes=22, overlaps=3) == EUNSUPPORTED
    assert _combine(lib, classes=14, overlaps=4) == EUNSUPPORTED                # align searches at most 3 slots
    assert _combine(lib, classes=14, overlaps=4, align=1, perm=SOME) == EUNSUPPORTED
    assert _combine(lib, R=1 << 40, frames=1 << 20) == EUNSUPPORTED             # 2^31 workgroups or more


def test_host_checks_of_the_wrappers():
    """What the binding refuses before it touches a device: window weights and, through _check_table, the table."""
    H, L = pkg().hip_ops, pkg()._lib
    for bad in ([1.0, 0.0, 1.0], [1.0, -1.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0], [1.0, 1.0]):
        with pytest.raises(L.SeldHipError):
            H.ensemble_window(np.asarray(bad, dtype=np.float32), 3, "cpu")
    with pytest.raises(L.SeldHipError):
        H.ensemble_window("hann", 8, "cpu")
    assert H.ensemble_window("uniform", 5, "cpu").tolist() == [1.0] * 5
    assert H.ensemble_window("triangular", 5, "cpu").tolist() == [1.0, 2.0, 3.0, 2.0, 1.0]
    assert H.ensemble_window("triangular", 4, "cpu").tolist() == [1.0, 2.0, 2.0, 1.0]
    assert H.ensemble_window([0.5, 2.0], 2, "cpu").tolist() == [0.5, 2.0]
    bad = H.foa_transforms()
    bad[3, 9] = 0                                                             # axis no permutation
    with pytest.raises(L.SeldHipError):
        H.ensemble_table(bad, "cpu")
    with pytest.raises(L.SeldHipError):
        H.ensemble_table(H.foa_transforms(), "cpu", channels=8)
    good = H.ensemble_table(H.foa_transforms(), "cpu", channels=4)
    assert H.ensemble_table(good, "cpu") is good and good.dtype.is_floating_point is False


def test_window_count():
    H, L = pkg().hip_ops, pkg()._lib
    W = H.window_count
    assert W(4800, 512, 256) == 18 and len(range(0, 4800, 256)) == 19        # segment's count has a mostly-padding tail window
    assert W(4800, 4800, 4800) == 1 and W(100, 512, 256) == 1 and W(512, 512, 256) == 1 and W(513, 512, 256) == 2
    assert W(37, 16, 8) == 4 and W(64, 16, 8) == 7 and W(160, 64, 32) == 4 and W(128, 64, 64) == 2 and W(20, 8, 3) == 5
    for length, seg, hop in ((37, 16, 8), (4800, 512, 256), (20, 8, 3), (5, 8, 3)):
        S = W(length, seg, hop)
        assert (S - 1) * hop + seg >= length and (S == 1 or (S - 2) * hop + seg < length)      # covers, and no fewer would
    for bad in ((0, 8, 4), (8, 0, 4), (8, 8, 0)):
        with pytest.raises(L.SeldHipError):
            W(*bad)


def test_reference_single_member_returns_its_input():
    rng = np.random.default_rng(0)
    sed = rng.uniform(0, 1, (1, 8, 42)).astype(np.float32)
    doa = rng.uniform(-1, 1, (1, 8, 126)).astype(np.float32)
    for kind in ("uniform", "triangular"):
        ref = E.combine(sed, doa, recordings=1, segments=1, hop_out=8, frames=8, classes=14, overlaps=3,
                        win=E.window_weights(kind, 8))
        assert np.array_equal(ref["sed"][0], sed[0].astype(np.float64)) and np.array_equal(ref["doa"][0], doa[0].astype(np.float64))
        assert (ref["perm"] == 0).all() and (ref["members"] == 1).all()
    # frames beyond the window are zeros, positions beyond `frames` get -1
    ref = E.combine(sed, doa, recordings=1, segments=1, hop_out=8, frames=10, classes=14, overlaps=3, win=E.window_weights("uniform", 8))
    assert not ref["sed"][0, 8:].any() and not ref["doa"][0, 8:].any() and ref["members"].tolist() == [1] * 8 + [0] * 2
    ref = E.combine(sed, doa, recordings=1, segments=1, hop_out=8, frames=5, classes=14, overlaps=3, win=E.window_weights("uniform", 8))
    assert (ref["perm"][0, :5] == 0).all() and (ref["perm"][0, 5:] == -1).all()


def test_reference_transform_rows_round_trip():
    """Labels transformed by the training formula (tests/loader_aug_ref.transform_y: location'[a] = sign[a] *
    location[axis[a]]) and mapped back by the combine's rule are the labels, for every preset row and the 3-cycle rows;
    a one-row table through `combine` gives the un-transformed input."""
    from tests.loader_aug_ref import transform_y
    H = pkg().hip_ops
    rng = np.random.default_rng(1)
    loc = rng.uniform(-1, 1, (5, 6, 3)).astype(np.float32)                   # (frames, slots, axes)
    for table in (H.foa_transforms(), H.foa_transforms(mics=2, phase=True), E.hand_table(4)):
        K, axis, sign = E.rows_of(table)
        C = (table.shape[1] - 6) // 2
        for k in range(K):
            moved = E.transform_doa(loc, axis[k], sign[k].astype(np.float32))
            y = np.concatenate([np.zeros((5, 6), np.float32), loc.reshape(5, 18)], axis=1)
            assert np.array_equal(transform_y(y, table[k], C)[:, 6:].reshape(5, 6, 3), moved)
            assert np.array_equal(E.untransform_doa(moved, axis[k], sign[k].astype(np.float32)), loc)
            sed = rng.uniform(0, 1, (1, 5, 6)).astype(np.float32)
            ref = E.combine(sed, moved.reshape(1, 5, 18), recordings=1, segments=1, hop_out=5, frames=5, classes=2, overlaps=3,
                            win=np.ones(5, np.float32), table=table[k:k + 1])
            assert np.array_equal(ref["doa"][0], loc.reshape(5, 18).astype(np.float64)) and (ref["perm"] == 0).all()


def test_reference_anchor_weights_and_alignment_by_hand():
    """Two windows of 4 frames, hop 2, one class of 2 slots, triangular weights 1 2 2 1.  Frame 2 is covered by window 0 at
    j = 2 (weight 2) and window 1 at j = 0 (weight 1): the anchor is window 0; window 1 holds the slots swapped."""
    sed = np.zeros((2, 4, 2), np.float32)
    doa = np.zeros((2, 4, 6), np.float32)
    sed[0, 2], doa[0, 2] = [0.9, 0.1], [1, 0, 0, 0, 1, 0]
    sed[1, 0], doa[1, 0] = [0.3, 0.6], [0, 1, 0, 1, 0, 0]
    win = E.window_weights("triangular", 4)
    assert win.tolist() == [1, 2, 2, 1]
    ref = E.combine(sed, doa, recordings=1, segments=2, hop_out=2, frames=6, classes=1, overlaps=2, win=win)
    assert ref["perm"][1, 0, 0] == 1 and ref["perm"][0, 2, 0] == 0
    assert np.allclose(ref["sed"][0, 2], [(2 * 0.9 + 0.6) / 3, (2 * 0.1 + 0.3) / 3], atol=1e-7)
    assert np.allclose(ref["doa"][0, 2], [1, 0, 0, 0, 1, 0], atol=1e-7)
    plain = E.combine(sed, doa, recordings=1, segments=2, hop_out=2, frames=6, classes=1, overlaps=2, win=win, align=False)
    assert np.allclose(plain["doa"][0, 2], [2 / 3, 1 / 3, 0, 1 / 3, 2 / 3, 0], atol=1e-7) and (plain["perm"] == 0).all()
    # equal weights: the lowest s is the anchor (frame 3: window 0 at j = 3 and window 1 at j = 1 under uniform weights)
    s_star, cover = E.anchors(2, 4, 2, 6, np.ones(4))
    assert s_star.tolist() == [0, 0, 0, 0, 1, 1] and cover.tolist() == [1, 1, 2, 2, 1, 1]
    s_star, _ = E.anchors(2, 4, 2, 6, win)
    assert s_star.tolist() == [0, 0, 0, 1, 1, 1]


def test_reference_window_batch_by_hand():
    H = pkg().hip_ops
    x = np.arange(2 * 8 * 1 * 5, dtype=np.float32).reshape(2, 8, 1, 5) / 100 - 0.2
    table = H.foa_transforms(mics=1, phase=True)
    out = E.window_batch(x, np.full((3, 8, 1, 4), -7.5, np.float32), seg_len=4, hop=3, segments=2, table=table, first=16 + 1, count=2)
    # member 17: r = 0, s = 1, k = 1 (x -> -x: the phase channel of X, 4 + 3, turned by pi; padding included)
    assert table[1, 8:16].tolist() == [0, 0, 0, 0, 0, 0, 0, 2]
    assert np.array_equal(out[0, 0], np.array([[x[0, 0, 0, 3], x[0, 0, 0, 4], 0, 0]], np.float32))
    assert np.array_equal(out[0, 7, 0, 2:], np.array([np.pi, np.pi], np.float32))
    assert np.array_equal(out[0, 7, 0, :2], E.flipop(2, x[0, 7, 0, 3:5]))
    assert (out[2] == -7.5).all()


@pytest.mark.parametrize("shape", E.PLANTED_SHAPES)
def test_reference_finds_no_ambiguous_cell_in_the_planted_cases(shape):
    """... and recovers the field in the anchor's order to the members' noise, under both windows."""
    R, S, K, T_out, hop_out, frames, classes, O = shape
    table = E.table_for(K, pkg().hip_ops.foa_transforms)
    case = E.planted(shape, table)
    for kind in ("uniform", "triangular"):
        win = E.window_weights(kind, T_out)
        ref = E.combine(case["sed"], case["doa"], recordings=R, segments=S, hop_out=hop_out, frames=frames, classes=classes,
                        overlaps=O, win=win, table=table)
        assert not ref["ambiguous"].any() and not ref["ambiguous_members"].any()
        ts, td = E.truth_for(case, shape, win)
        assert np.abs(ref["sed"] - ts).max() <= 0.01 + 1e-6 and np.abs(ref["doa"] - td).max() <= 0.01 + 1e-6


@pytest.mark.parametrize("shape", E.RANDOM_SHAPES)
def test_reference_ambiguity_of_the_random_cases(shape):
    """The seeds of the random cases: no ambiguous member at the small shape, at most 0.1 % of the members' cells (the
    entries of perm, which is where a near-tie can flip the kernel's choice) at the 600-frame one.  Measured with seed 0
    there: 17 of 258048 entries (0.007 %), which touch 17 of the 8400 output cells (0.20 %); over seeds 0..11 the output
    cells touched are 17..33, so no seed brings THAT count under 0.1 %: each of the 32 members of a cell is a chance."""
    R, S, K, T_out, hop_out, frames, classes, O = shape
    table = E.table_for(K, pkg().hip_ops.foa_transforms)
    sed, doa = E.uniform_members(shape, E.RANDOM_SEEDS[shape])
    ref = E.combine(sed, doa, recordings=R, segments=S, hop_out=hop_out, frames=frames, classes=classes, overlaps=O,
                    win=E.window_weights("triangular", T_out), table=table)
    live = ref["perm"] >= 0
    assert live.any() and not ref["ambiguous_members"][~live].any()
    if frames < 600:
        assert not ref["ambiguous_members"].any() and not ref["ambiguous"].any()
    else:
        assert ref["ambiguous_members"].sum() <= 1e-3 * live.sum()
        assert 0 < ref["ambiguous"].sum() <= ref["ambiguous_members"].sum()


def test_flags_default_to_off_and_refusals_come_before_the_device():
    T = pkg().train
    off = T.parse_args(["--TextArgs=none"])
    assert (off.test_hop, off.test_tta) == (0, 0) and not T.ensemble_requested(off) and T.ensemble_from_args(off) is None
    got = T.ensemble_from_args(T.parse_args(["--TextArgs=none", "--test_hop=256", "--time_dim=512"]))
    assert got["hop"] == 256 and got["table"] is None
    got = T.ensemble_from_args(T.parse_args(["--TextArgs=none", "--test_tta=8", "--n_mics=2", "--input_channels=8"]))
    assert got["hop"] == 4800 and got["table"].shape == (8, 22) and (got["table"][:, -1] == 1).all()      # z fixed
    got = T.ensemble_from_args(T.parse_args(["--TextArgs=none", "--test_tta=16", "--phase=True", "--dataset_normalization=False"]))
    assert got["table"].shape == (16, 22) and set(np.unique(got["table"][:, 8:16])) == {0, 2}
    for argv, match in ((["--test_tta=16", "--phase=True"], "raw phase"), (["--test_tta=4"], "test_tta"),
                        (["--test_hop=-1"], "test_hop"), (["--test_tta=8", "--n_mics=3"], "n_mics")):
        args = T.parse_args(["--TextArgs=none"] + argv)
        with pytest.raises(ValueError, match=match):
            T.ensemble_from_args(args)
        with pytest.raises(ValueError, match=match):
            T.main(args)
