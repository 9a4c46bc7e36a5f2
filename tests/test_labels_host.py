"""Target encoding and segmentation without a GPU: the public names and their signatures, the C ABI (symbols, refusals
before the device is touched), event_frames against the frames the reference fills, the plain-numpy statements of
both operations against the reference's fixture (tests/golden/labels.npz), and the fixture against its case table."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests.golden.labels_cases import (CLASS_NAMES, ENCODE_CASES, ENCODE_IDS, SEGMENT_CASES, SEGMENT_IDS, class_dict,
                                       encode_csv, segment_inputs)
from tests.helpers import pkg
from tests.labels_helpers import (class_names, csv_times, encode_events_host, encode_numpy, fixture_chunks,
                                  segment_numpy)

EINVAL, EUNSUPPORTED = -1, -4                       # include/seld_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty
TASK2 = [c for c in SEGMENT_CASES if c["fn"] == "segment_task2" and not c["raises"] and not c["ragged"]]


def _params(fn):
    return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]


def test_public_names_and_signatures():
    p = pkg()
    UF, H = p.utility_functions, p.hip_ops
    assert _params(UF.csv_to_matrix_task2) == [("path", EMPTY), ("class_dict", EMPTY), ("dur", 60), ("step", 0.1),
                                               ("max_loc_value", 2.), ("no_overlaps", False)]
    assert _params(UF.segment_task2) == [("predictors", EMPTY), ("target", EMPTY), ("predictors_len_segment", 400),
                                         ("target_len_segment", 50), ("overlap", 0.5)]
    assert _params(UF.segment_waveforms) == [("predictors", EMPTY), ("target", EMPTY), ("length", EMPTY)]
    assert _params(H.event_frames) == [("start", EMPTY), ("end", EMPTY), ("dur", 60), ("step", 0.1)]
    assert _params(H.encode_events)[:11] == [
        ("first", EMPTY), ("last", EMPTY), ("cls", EMPTY), ("xyz", EMPTY), ("rec_offsets", EMPTY), ("frames", EMPTY),
        ("classes", 14), ("overlaps", 3), ("max_loc_value", 2.), ("no_overlaps", False), ("dtype", torch.float64)]
    assert _params(H.segment) == [("x", EMPTY), ("seg_len", EMPTY), ("hop", EMPTY), ("time_first", False), ("segments", None)]


def test_header_declares_and_library_exports_entry_points():
    with open(os.path.join(ROOT, "include", "seld_hip.h")) as f:
        header = f.read()
    for name in ("seld_encode_events", "seld_segment"):
        assert f"{name}(" in header, name
    for cite in ("utility_functions.py:219-267", "utility_functions.py:302-342", ":272-299", "SELD_ENCODE_MAX_EVENTS 4096"):
        assert cite in header, cite
    lib = pkg()._lib.lib()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert lib.seld_encode_events.argtypes == [vp, vp, vp, vp, vp, i64, i32, i64, i32, i32, i32, ctypes.c_double, i32, i32,
                                               vp, vp, vp]
    assert lib.seld_segment.argtypes == [vp, i32, i32, i64, i64, i64, i64, i64, vp, vp]
    assert pkg().hip_ops.ENCODE_MAX_EVENTS == 4096


def _encode(lib, p, events=10, max_rec=10, R=2, frames=600, classes=14, overlaps=3, dtype=1, first=True, last=True,
            cls=True, xyz=True, offs=True, target=True, overflow=True):
    a = [p if k else None for k in (first, last, cls, xyz, offs)]
    return lib.seld_encode_events(a[0], a[1], a[2], a[3], a[4], events, max_rec, R, frames, classes, overlaps, 2.0, 0, dtype,
                                  p if target else None, p if overflow else None, None)


def test_encode_refusals_without_gpu():
    """Host-side argument checking: a refused call returns before it touches the device (on a machine without one a
    launch could only answer SELD_ELAUNCH)."""
    lib = pkg()._lib.lib()
    p = ctypes.c_void_p(64)
    for kw in (dict(R=0), dict(R=-1), dict(frames=0), dict(frames=-3), dict(classes=0), dict(overlaps=0), dict(events=-1),
               dict(max_rec=-1), dict(max_rec=11), dict(dtype=2), dict(dtype=-1), dict(first=False), dict(last=False),
               dict(cls=False), dict(xyz=False), dict(offs=False), dict(target=False), dict(overflow=False)):
        assert _encode(lib, p, **kw) == EINVAL, kw
    # the stated limits: 64 slots, SELD_ENCODE_MAX_EVENTS events in one recording, 2^31 workgroups
    for kw in (dict(classes=13, overlaps=5), dict(classes=65, overlaps=1), dict(classes=1, overlaps=65),
               dict(classes=22, overlaps=3), dict(events=5000, max_rec=4097), dict(R=1 << 31, frames=600)):
        assert _encode(lib, p, **kw) == EUNSUPPORTED, kw
    # the refusal comes before the limits are even looked at when the descriptor is malformed
    assert _encode(lib, p, classes=22, overlaps=3, target=False) == EINVAL


def test_segment_refusals_without_gpu():
    lib = pkg()._lib.lib()
    p = ctypes.c_void_p(64)

    def seg(src=p, dtype=0, layout=0, rows=8, length=100, seg_len=10, hop=5, segments=20, dst=p):
        return lib.seld_segment(src, dtype, layout, rows, length, seg_len, hop, segments, dst, None)
    for kw in (dict(src=None), dict(dst=None), dict(dtype=2), dict(dtype=-1), dict(layout=2), dict(layout=-1), dict(rows=0),
               dict(length=0), dict(seg_len=0), dict(hop=0), dict(hop=-1), dict(segments=0), dict(rows=-4)):
        assert seg(**kw) == EINVAL, kw
    for kw in (dict(rows=1 << 30, length=1 << 16), dict(rows=1 << 30, seg_len=1 << 16), dict(segments=1 << 30, hop=1 << 16),
               dict(layout=1, rows=1 << 20, length=1 << 26)):
        assert seg(**kw) == EUNSUPPORTED, kw


def test_wrappers_validate_on_the_host():
    p = pkg()
    L, H, UF = p._lib, p.hip_ops, p.utility_functions
    ok = dict(first=[0, 5], last=[3, 9], cls=[1, 13], xyz=[[0.1, 0.2, 0.3], [1, 1, 1]], rec_offsets=[0, 2], frames=10)
    bad = [dict(cls=[1, 14]), dict(cls=[-1, 3]), dict(last=[3, 10]), dict(first=[-1, 5]), dict(rec_offsets=[0, 3]),
           dict(rec_offsets=[1, 2]), dict(rec_offsets=[0, 2, 1, 2]), dict(xyz=[[0.1, 0.2, 0.3]]), dict(frames=0),
           dict(classes=22), dict(overlaps=0), dict(dtype=torch.float16),
           dict(first=[0] * 4097, last=[0] * 4097, cls=[0] * 4097, xyz=[[0., 0., 0.]] * 4097, rec_offsets=[0, 4097])]
    for kw in bad:
        with pytest.raises(L.SeldHipError):
            H.encode_events(**dict(ok, **kw))
    with pytest.raises(L.SeldHipError, match="no CPU path"):
        H.segment(torch.zeros(4, 100), 10, 5)
    with pytest.raises(L.SeldHipError, match="both be numpy arrays or both device tensors"):
        UF.segment_task2(np.zeros((2, 3, 800), np.float32), torch.zeros(100, 8))
    with pytest.raises(L.SeldHipError, match="unsupported dtype"):
        UF.segment_waveforms(np.zeros((2, 800), np.int16), np.zeros((2, 800), np.int16), 100)
    if not torch.cuda.is_available():
        with pytest.raises(L.SeldHipError, match="no HIP device"):
            H.encode_events(**ok)
        with pytest.raises(L.SeldHipError, match="no HIP device"):
            UF.segment_task2(np.zeros((2, 3, 800), np.float32), np.zeros((100, 8), np.float32))


def test_fixture_agrees_with_the_case_table(golden):
    g = golden("labels")
    meta = json.loads(str(g["meta"]))
    assert meta["stand_ins"] in ([], ["librosa"])
    assert meta["encode_cases"] == ENCODE_IDS and meta["segment_cases"] == SEGMENT_IDS
    assert class_names(g) == CLASS_NAMES and len(class_dict()) == 14
    for c in ENCODE_CASES:
        name = c["name"]
        assert bytes(g[name + ".csv"]).decode() == encode_csv(c), name
        assert str(g[name + ".raised"]) == c["raises"], name
        assert ((name + ".matrix") in g) == (not c["raises"]), name
        events = len(encode_csv(c).splitlines()) - 1
        assert g[name + ".first"].shape == g[name + ".last"].shape == g[name + ".cls"].shape == (events,)
        assert g[name + ".xyz"].shape == (events, 3)
    for c in SEGMENT_CASES:
        assert str(g[c["name"] + ".raised"]) == c["raises"], c["name"]
    # what the cases are for
    by = {c["name"]: c for c in ENCODE_CASES}
    frames = int(by["random_60"]["dur"] / by["random_60"]["step"])
    m = g["random_60.matrix"]
    assert m.shape == (600, 168) and frames == 600 and m.dtype == np.float64
    assert 50 <= g["random_60.first"].shape[0] <= 70 and 1500 < m[:, :42].sum() < 2500
    assert g["random_60_single.matrix"].shape == (600, 56)
    assert (g["three_same.matrix"][:, :42].reshape(600, 14, 3).sum(2) == 3).any()          # every slot of a class filled
    assert g["ends_at_dur.last"].max() == 599 and g["ends_at_dur.matrix"][599, :42].sum() == 3
    assert str(g["four_same.raised"]) == str(g["four_same_single.raised"]) == "IndexError"
    assert g["empty.first"].shape == (0,) and not g["empty.matrix"].any()
    assert g["maxloc_1p7.matrix"].shape == (300, 168) and g["step_0p2.matrix"].shape == (100, 168)
    counts = {c["name"]: int(g[c["name"] + ".count"]) for c in SEGMENT_CASES if not c["raises"]}
    assert counts["task2_4800"] == 24 and counts["task2_1237"] == 7 and counts["task2_overlap_1"] == 3
    assert str(g["task2_counts_differ.raised"]) == "ValueError"
    assert {c["p_dtype"] for c in SEGMENT_CASES} == {"float32", "float64"}
    # where this package raises, the reference returns target chunks of different lengths
    _, Y = fixture_chunks(g, "task2_ragged_target")
    assert [y.shape for y in Y] == [(50, 4), (50, 4), (40, 4), (50, 4)]
    # the padded last chunk is float64 in the reference whatever the input (the documented dtype difference)
    X, Y = fixture_chunks(g, "task2_4800")
    assert X[0].dtype == np.float32 and X[-1].dtype == np.float64 and Y[0].dtype == np.float32 and Y[-1].dtype == np.float64


@pytest.mark.parametrize("case", ENCODE_CASES, ids=ENCODE_IDS)
def test_event_frames_equal_the_frames_the_reference_fills(golden, case):
    g = golden("labels")
    H = pkg().hip_ops
    start, end = csv_times(bytes(g[case["name"] + ".csv"]).decode())
    first, last = H.event_frames(start, end, case["dur"], case["step"])
    assert first.dtype == np.int64 and last.dtype == np.int64
    assert np.array_equal(first, g[case["name"] + ".first"]) and np.array_equal(last, g[case["name"] + ".last"])


def test_event_frames_equal_the_reference_lambdas_spelled_out():
    """The vectorised form against the per-element expressions of utility_functions.py:226-228, ties included."""
    H = pkg().hip_ops
    x = np.concatenate([np.arange(0, 1201) * 0.05, [59.96, 60.0, 61.0, 1e-9, 33.349, 33.351]])
    for dur, step in ((60, 0.1), (20, 0.2), (30, 0.1)):
        n = int(dur / step)
        want = [int(np.interp(round(float(v) / step) * step, (0, dur), (0, n - 1))) for v in x]
        first, last = H.event_frames(x, x[::-1], dur, step)
        assert first.tolist() == want and last.tolist() == want[::-1]


@pytest.mark.parametrize("case", [c for c in ENCODE_CASES if not c["raises"]],
                         ids=[c["name"] for c in ENCODE_CASES if not c["raises"]])
def test_numpy_statement_of_the_encoding_equals_the_reference(golden, case):
    g = golden("labels")
    first, last, cls, xyz = encode_events_host(g, case["name"])
    frames = int(case["dur"] / case["step"])
    got, over = encode_numpy(first, last, cls, xyz, frames, 14, 3, case["max_loc"], case["no_overlaps"])
    ref = g[case["name"] + ".matrix"]
    assert over == 0 and got.shape == ref.shape and got.tobytes() == ref.tobytes()


def test_numpy_statement_counts_the_overflow_the_reference_raises_on(golden):
    g = golden("labels")
    for name in ("four_same", "four_same_single"):
        first, last, cls, xyz = encode_events_host(g, name)
        _, over = encode_numpy(first, last, cls, xyz, 600, no_overlaps=name.endswith("single"))
        assert over == 3                                     # the three frames of the fourth event of class 5


@pytest.mark.parametrize("case", TASK2, ids=[c["name"] for c in TASK2])
def test_reshape_quirk_is_the_time_last_cut_of_the_reinterpreted_target(golden, case):
    """Y_s.flat[m] = target.flat[(m // Lt) * T + s * hop + m % Lt], 0 where s * hop + m % Lt >= T: the reference's
    reshape(1, n, T) reinterprets the (T, n) buffer, so its target chunks are the time-last cut of that buffer seen as
    (n, T), each (n, Lt) result viewed as (Lt, n)."""
    g = golden("labels")
    p, t = segment_inputs(case)
    kw = dict(dict(predictors_len_segment=400, target_len_segment=50, overlap=0.5), **case["kw"])
    Lp, Lt = kw["predictors_len_segment"], kw["target_len_segment"]
    hop_p, hop_t = int(Lp * kw["overlap"]), int(Lt * kw["overlap"])
    X, Y = fixture_chunks(g, case["name"])
    T, n = t.shape
    flat = t.reshape(-1)
    m = np.arange(Lt * n)
    for s, y in enumerate(Y):
        pos = s * hop_t + m % Lt
        want = np.where(pos < T, flat[np.minimum((m // Lt) * T + pos, flat.size - 1)], 0)
        assert y.shape == (Lt, n) and np.array_equal(y.reshape(-1), want), s
    cut = segment_numpy(t.reshape(n, T), Lt, hop_t, len(Y)).reshape(len(Y), Lt, n)
    assert all(np.array_equal(cut[s], y) for s, y in enumerate(Y))
    assert not np.array_equal(cut, segment_numpy(t, Lt, hop_t, len(Y), time_first=True))      # not the cut by rows
    cut_x = segment_numpy(p, Lp, hop_p, len(X))
    assert all(x.shape == cut_x[s].shape and np.array_equal(cut_x[s], x) for s, x in enumerate(X))
