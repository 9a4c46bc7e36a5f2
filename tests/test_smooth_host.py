"""Track post-processing without a device: the reference of tests/smooth_ref.py against scipy and its own planted cases,
the proof that every rule fires in the random cases, what the library refuses before it launches, and the --post_* flags
of train.py (those tests are the ones that need this feature; the rest validates the yardstick)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
from scipy.ndimage import median_filter

from tests import smooth_ref as S
from tests.helpers import pkg

EINVAL, EUNSUPPORTED = -1, -4
NULL, SOME = None, ctypes.c_void_p(4096)            # never dereferenced: every call here is refused before the launch
PLANTED = S.planted_cases()


# ---- the yardstick --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("median", S.MEDIANS + (5, 13))
def test_reference_median_is_scipys_nearest_mode(median):
    for shape, seed in (((2, 40, 3), 1), ((1, 7, 2), 2), ((1, 1, 1), 3), ((3, 65, 5), 4)):
        sed, doa = S.random_track(*shape, seed)
        got = S.smooth(sed, doa, median=median)["prob"]
        assert np.array_equal(got, median_filter(sed, size=(1, median, 1), mode="nearest")), (shape, median)


@pytest.mark.parametrize("case", PLANTED, ids=[c["name"] for c in PLANTED])
def test_reference_gives_the_planted_outputs(case):
    mode = case["want_doa"][0] if case["want_doa"] else "frame"
    ref = S.smooth(case["sed"], case["doa"], doa_mode=mode, **case["params"])
    assert np.array_equal(ref["sed"], case["want_sed"])
    if case["want_prob"] is not None:
        assert np.array_equal(ref["prob"], case["want_prob"])
    if case["want_doa"] is not None:
        assert np.array_equal(ref["doa"], case["want_doa"][1])
        assert not np.array_equal(ref["doa"], case["doa"])
    else:
        assert np.array_equal(ref["doa"], case["doa"])


def test_planted_cases_cover_every_rule():
    names = {c["name"] for c in PLANTED}
    assert {"gap_fill", "gap_at_the_ends", "min_frames", "runs_touching_the_ends", "hysteresis", "fill_then_duration",
            "duration_without_fill", "at_the_thresholds", "median_3", "median_wider_than_T", "mean_doa",
            "weighted_doa"} <= names
    by = {c["name"]: S.smooth(c["sed"], c["doa"], **c["params"]) for c in PLANTED}
    assert by["gap_fill"]["filled"] == 1 and by["gap_at_the_ends"]["filled"] == 1
    assert by["min_frames"]["short"] == 2 and by["runs_touching_the_ends"]["short"] == 0
    assert (by["hysteresis"]["kept"], by["hysteresis"]["dropped"]) == (1, 2)
    assert (by["fill_then_duration"]["filled"], by["fill_then_duration"]["short"]) == (1, 0)
    assert (by["duration_without_fill"]["filled"], by["duration_without_fill"]["short"]) == (0, 2)
    assert (by["at_the_thresholds"]["kept"], by["at_the_thresholds"]["dropped"]) == (2, 1)
    assert any(c["params"]["median"] > c["sed"].shape[1] for c in PLANTED)


def test_reference_identity_settings():
    sed, doa = S.random_track(3, 65, 42, 11)
    ref = S.smooth(sed, doa, **S.IDENTITY)
    assert np.array_equal(ref["sed"], (sed > 0.5).astype(np.float32)) and np.array_equal(ref["prob"], sed)
    assert np.array_equal(ref["doa"], doa)
    assert (sed == 0.5).any() and ref["filled"] == ref["short"] == ref["dropped"] == 0
    rows, offsets, _ = S.events(ref["sed"], doa)
    assert [(int(r[0]), int(r[1]) * 3 + int(r[2]), int(r[3]), int(r[4])) for r in rows] == [q[:4] for q in ref["runs"]]
    assert offsets[0] == 0 and offsets[-1] == len(rows) and (np.diff(offsets) >= 0).all()


@pytest.mark.parametrize("T", [t for t in S.RANDOM_T if t >= 63] + [S.MAX_FRAMES])
def test_every_rule_fires_in_the_random_cases(T):
    """Over the random cases at T frames a gap is filled, a run is dropped for its length, and the `on` rule keeps one
    run and drops another, each in at least one case; ties and at-threshold values occur; both DOA modes, every median
    and every setting occur over the whole list."""
    specs = S.random_specs(T) if T != S.MAX_FRAMES else [S.longest_spec()]
    cases = [S.random_case(spec) for spec in specs]
    for counter in ("filled", "short", "kept", "dropped"):
        assert max(c["ref"][counter] for c in cases) >= 1, (T, counter)
    assert any((c["ref"]["prob"] == np.float32(c["params"]["on"])).any() for c in cases)
    assert any((c["ref"]["prob"] == np.float32(c["params"]["off"])).any() for c in cases)
    if T != S.MAX_FRAMES:
        assert sorted({c["shape"] for c in cases}) == sorted((R, T, n) for R in S.RANDOM_R for n in S.RANDOM_N)
        assert any(c["params"]["max_gap"] >= T for c in cases) or any(c["params"]["min_frames"] > T for c in cases)


def test_random_cases_take_every_setting_with_every_kind_of_shape():
    specs = [s for T in S.RANDOM_T for s in S.random_specs(T)]
    assert {s["params"]["median"] for s in specs} == set(S.MEDIANS)
    assert {s["doa_mode"] for s in specs} == {"mean", "weighted"}
    for n in S.RANDOM_N:
        mine = [s for s in specs if s["shape"][2] == n and s["shape"][1] >= 63]
        assert {s["params"]["median"] for s in mine} == set(S.MEDIANS), n
        assert any(s["params"]["off"] == s["params"]["on"] for s in mine) and any(s["params"]["off"] == 0 for s in mine)
        assert any(s["params"]["max_gap"] >= s["shape"][1] for s in mine), n
        assert any(s["params"]["min_frames"] > s["shape"][1] for s in mine), n
    assert S.longest_spec()["shape"] == (1, pkg().hip_ops.SMOOTH_MAX_FRAMES, 3)


# ---- the library, before any launch -----------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    L = pkg()._lib
    with open(L.HEADER_PATH) as f:
        text = f.read()
    declared = L.prototypes(text)
    i32, i64, ptr, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert declared["seld_smooth_tracks"] == (ctypes.c_int, [ptr, ptr, i64, i32, i32, i32, f32, f32, i32, i32, i32, ptr, ptr,
                                                             ptr, ptr])
    assert declared["seld_track_events_workspace"] == (ctypes.c_size_t, [i64, i32, i32])
    assert declared["seld_track_events_count"] == (ctypes.c_int, [ptr, i64, i32, i32, ptr, ctypes.c_size_t, ptr])
    assert declared["seld_track_events_write"] == (ctypes.c_int, [ptr, ptr, i64, i32, i32, i32, ctypes.c_double, ptr,
                                                                  ctypes.c_size_t, ptr, i64, ptr, ptr])
    H = pkg().hip_ops
    assert f"#define SELD_SMOOTH_MAX_MEDIAN {H.SMOOTH_MAX_MEDIAN}\n" in text
    assert f"#define SELD_SMOOTH_MAX_FRAMES {H.SMOOTH_MAX_FRAMES} " in text and H.SMOOTH_MAX_FRAMES >= 16384
    for name, code in H.SMOOTH_DOA_MODES.items():
        assert f"#define SELD_SMOOTH_DOA_{name.upper()} {code}\n" in text
    assert (S.MAX_MEDIAN, S.MAX_FRAMES, S.DOA_MODES) == (H.SMOOTH_MAX_MEDIAN, H.SMOOTH_MAX_FRAMES, tuple(H.SMOOTH_DOA_MODES))
    lib = L.lib()
    for name in ("seld_smooth_tracks", "seld_track_events_workspace", "seld_track_events_count", "seld_track_events_write"):
        assert list(getattr(lib, name).argtypes) == declared[name][1]


def _smooth(lib, sed=SOME, doa=SOME, R=2, T=64, n=42, median=7, on=0.75, off=0.25, min_frames=3, max_gap=2, mode=2,
            out_sed=SOME, out_doa=SOME, out_prob=NULL):
    return lib.seld_smooth_tracks(sed, doa, R, T, n, median, on, off, min_frames, max_gap, mode, out_sed, out_doa, out_prob, NULL)


def test_smooth_tracks_refuses_without_launching():
    lib = pkg()._lib.lib()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(sed=NULL), dict(doa=NULL), dict(out_sed=NULL), dict(out_doa=NULL), dict(R=0), dict(R=-1), dict(T=0),
               dict(n=0), dict(n=-3), dict(median=0), dict(median=2), dict(median=30), dict(median=33), dict(median=-1),
               dict(on=nan), dict(off=nan), dict(on=inf), dict(off=-inf), dict(on=0.25, off=0.75), dict(on=1.5),
               dict(off=-0.25), dict(min_frames=0), dict(min_frames=-2), dict(max_gap=-1), dict(mode=3), dict(mode=-1)):
        assert _smooth(lib, **kw) == EINVAL, kw
    assert _smooth(lib, T=S.MAX_FRAMES + 1) == EUNSUPPORTED
    assert _smooth(lib, R=1 << 26, n=32) == EUNSUPPORTED                         # 2^31 columns
    assert _smooth(lib, R=1 << 40, n=1) == EUNSUPPORTED


def test_track_events_refuses_without_launching():
    lib = pkg()._lib.lib()
    assert lib.seld_track_events_workspace(2, 600, 42) == 16 + 8 * 840 + 4 * 840
    assert lib.seld_track_events_workspace(1, 1, 1) == 16 + 8 + 8
    assert lib.seld_track_events_workspace(0, 600, 42) == 0 and lib.seld_track_events_workspace(2, 0, 42) == 0
    assert lib.seld_track_events_workspace(1 << 24, 64 * 128 + 1, 1) == 0        # 2^31 segments
    ws = lib.seld_track_events_workspace(2, 600, 42)
    assert lib.seld_track_events_count(NULL, 2, 600, 42, SOME, ws, NULL) == EINVAL
    assert lib.seld_track_events_count(SOME, 0, 600, 42, SOME, ws, NULL) == EINVAL
    assert lib.seld_track_events_count(SOME, 2, 600, 42, NULL, ws, NULL) == -2
    assert lib.seld_track_events_count(SOME, 2, 600, 42, SOME, ws - 1, NULL) == -2
    assert lib.seld_track_events_count(SOME, 1 << 24, 64 * 128 + 1, 1, SOME, ws, NULL) == EUNSUPPORTED

    def write(sed=SOME, doa=SOME, R=2, T=600, classes=14, overlaps=3, work=SOME, nbytes=ws, rows=SOME, capacity=5, offs=SOME):
        return lib.seld_track_events_write(sed, doa, R, T, classes, overlaps, 2.0, work, nbytes, rows, capacity, offs, NULL)
    for kw in (dict(sed=NULL), dict(doa=NULL), dict(offs=NULL), dict(rows=NULL), dict(capacity=-1), dict(classes=0),
               dict(overlaps=0), dict(R=0), dict(T=-1)):
        assert write(**kw) == EINVAL, kw
    assert write(work=NULL) == -2 and write(nbytes=ws - 8) == -2


def test_wrappers_validate_on_the_host(monkeypatch):
    H, L = pkg().hip_ops, pkg()._lib
    monkeypatch.setattr(torch.cuda, "_lazy_init", lambda *a, **k: pytest.fail("the device was touched"))
    assert list(inspect.signature(H.smooth_tracks).parameters)[2:] == ["median", "on", "off", "min_frames", "max_gap", "doa",
                                                                      "return_prob"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(inspect.signature(H.smooth_tracks).parameters.values())[2:])
    assert list(inspect.signature(H.track_events).parameters) == ["sed", "doa", "max_loc_value", "num_classes", "max_overlaps"]
    sed, doa = torch.zeros(8, 3), torch.zeros(8, 9)
    for kw in (dict(median=2), dict(median=33), dict(on=0.2, off=0.4), dict(on=1.2), dict(off=-0.1), dict(on=float("nan")),
               dict(min_frames=0), dict(max_gap=-1), dict(doa="median"), dict(median=3.0), dict()):
        with pytest.raises(L.SeldHipError):                 # the settings first, then "no CPU path"
            H.smooth_tracks(sed, doa, **kw)
    with pytest.raises(L.SeldHipError):
        H.track_events(sed, doa, 2., 1, 3)
    post = H.PostProcess()
    assert post.is_identity and post.kwargs() == dict(S.IDENTITY, doa="frame")
    for kw in (dict(median=3), dict(on=0.6), dict(off=0.4), dict(min_frames=2), dict(max_gap=1), dict(doa="mean")):
        assert not H.PostProcess(**kw).is_identity
    with pytest.raises(Exception):
        post.median = 3                                     # frozen


# ---- train.py ---------------------------------------------------------------------------------------------------------
def test_post_flags_default_to_off_and_refusals_come_before_the_device(monkeypatch):
    T, H = pkg().train, pkg().hip_ops
    monkeypatch.setattr(torch.cuda, "_lazy_init", lambda *a, **k: pytest.fail("the device was touched"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    off = T.parse_args(["--TextArgs=none"])
    assert (off.post_median, off.post_on, off.post_off, off.post_min_frames, off.post_max_gap, off.post_doa) == \
        (1, 0.5, 0.5, 1, 0, "frame")
    assert not T.postprocess_requested(off) and T.postprocess_from_args(off) is None
    got = T.postprocess_from_args(T.parse_args(["--TextArgs=none", "--post_median=7", "--post_on=0.6", "--post_off=0.4",
                                                "--post_min_frames=3", "--post_max_gap=2", "--post_doa=weighted"]))
    assert got == H.PostProcess(median=7, on=0.6, off=0.4, min_frames=3, max_gap=2, doa="weighted") and not got.is_identity
    for flag in ("--post_median=3", "--post_on=0.7", "--post_off=0.3", "--post_min_frames=2", "--post_max_gap=1",
                 "--post_doa=mean"):
        args = T.parse_args(["--TextArgs=none", flag])
        assert T.postprocess_requested(args) and isinstance(T.postprocess_from_args(args), H.PostProcess), flag
    for argv, match in ((["--post_median=4"], "median"), (["--post_median=33"], "median"), (["--post_median=-1"], "median"),
                        (["--post_on=0.3", "--post_off=0.4"], "off"), (["--post_off=0.6"], "off"),
                        (["--post_on=1.5"], "on"), (["--post_off=-0.1"], "off"), (["--post_on=nan"], "on"),
                        (["--post_min_frames=0"], "min_frames"), (["--post_max_gap=-1"], "max_gap"),
                        (["--post_doa=median"], "doa")):
        args = T.parse_args(["--TextArgs=none"] + argv)
        assert T.postprocess_requested(args)
        with pytest.raises(ValueError, match=match):
            T.postprocess_from_args(args)
        with pytest.raises(ValueError, match=match):
            T.main(args)


def test_test_leg_entry_points_take_the_settings():
    T = pkg().train
    assert "post" not in inspect.signature(T.predict_test).parameters       # tests/test_decode_host.py pins its signature
    assert [(k, v.default) for k, v in inspect.signature(T.predict_test_post).parameters.items()] == \
        [(k, v.default) for k, v in inspect.signature(T.predict_test).parameters.items()] + [("post", None)]
    assert inspect.signature(T.evaluate_recordings).parameters["post"].default is None
    assert inspect.signature(T.evaluate_recordings).parameters["post"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "post" not in inspect.signature(T.evaluate_test).parameters      # it reads them from its `args`
    assert T._active_post(None) is None and T._active_post(pkg().hip_ops.PostProcess()) is None
    assert T._active_post(dict(median=3)).median == 3
