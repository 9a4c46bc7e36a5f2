"""Event decoding without a GPU: the public names and their signatures, the C ABI (symbols, workspace, refusals before
the device is touched), and the fixture (tests/golden/decode.npz, made by the reference's gen_submission_list_task2 and
gen_submission_list_task2_OLD) against oracle.decode_events turned into rows, bit for bit."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests.decode_helpers import fixture_dict, oracle_rows
from tests.golden.decode_cases import CASE_IDS, DECODE_CASES, decode_inputs, uniform
from tests.helpers import pkg

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4            # include/seld_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["seld_decode_workspace", "seld_decode_count", "seld_decode_write"]
SIGNATURE = [("sed", inspect.Parameter.empty), ("doa", inspect.Parameter.empty), ("max_loc_value", 2.), ("num_frames", 600),
             ("num_classes", 14), ("max_overlaps", 3)]


def test_public_names_and_signatures():
    from importlib import import_module
    uf = import_module(pkg().__name__ + ".utility_functions")
    for name in ("gen_submission_list_task2", "gen_submission_list_task2_OLD"):
        sig = inspect.signature(getattr(uf, name))
        assert [(k, v.default) for k, v in sig.parameters.items()] == SIGNATURE, (name, sig)
    p = pkg()
    sig = inspect.signature(p.hip_ops.decode_events)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("sed", inspect.Parameter.empty), ("doa", inspect.Parameter.empty), ("max_loc_value", 2.), ("num_classes", 14),
        ("max_overlaps", 3)]
    sig = inspect.signature(p.train.predict_test)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("model", inspect.Parameter.empty), ("device", inspect.Parameter.empty), ("dataloader", inspect.Parameter.empty),
        ("max_loc_value", 2.), ("num_frames", 600)]


def test_header_declares_and_library_exports_entry_points():
    with open(os.path.join(ROOT, "include", "seld_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert f"{name}(" in header, name
    for cite in ("utility_functions.py:158-181", "utility_functions.py:184-210", "train.py:110-116"):
        assert cite in header, cite
    lib = pkg()._lib.lib()
    for name in NAMES:
        assert hasattr(lib, name), name


def _count(lib, sed, dtype, R, T, classes, overlaps, ws, ws_bytes):
    return lib.seld_decode_count(sed, dtype, R, T, classes, overlaps, ws, ws_bytes, None)


def _write(lib, doa, dtype, R, T, classes, overlaps, ws, ws_bytes, rows, event, cap, offs):
    return lib.seld_decode_write(doa, dtype, R, T, classes, overlaps, 2.0, ws, ws_bytes, rows, event, cap, offs, None)


def test_refusals_without_gpu():
    """Host-side argument checking: every entry point refuses before it touches the device."""
    lib = pkg()._lib.lib()
    p = ctypes.c_void_p(64)
    need = lib.seld_decode_workspace(2, 600, 14, 3)
    assert need >= 8 + 8 * 1200                                   # the total and one 64-bit mask per frame
    big = 1 << 30
    # non-positive sizes, an unknown dtype
    for R, T, c, o in [(0, 600, 14, 3), (2, 0, 14, 3), (2, 600, 0, 3), (2, 600, 14, 0), (-1, 600, 14, 3), (2, -5, 14, 3)]:
        assert lib.seld_decode_workspace(R, T, c, o) == 0, (R, T, c, o)
        assert _count(lib, p, 0, R, T, c, o, p, big) == EINVAL, (R, T, c, o)
        assert _write(lib, p, 0, R, T, c, o, p, big, p, p, 10, p) == EINVAL, (R, T, c, o)
    assert _count(lib, p, 2, 2, 600, 14, 3, p, big) == EINVAL
    assert _write(lib, p, -1, 2, 600, 14, 3, p, big, p, p, 10, p) == EINVAL
    # more than one wave's ballot; more frames than a 31-bit index
    for c, o in [(13, 5), (65, 1), (1, 65), (22, 3)]:
        assert lib.seld_decode_workspace(2, 600, c, o) == 0, (c, o)
        assert _count(lib, p, 0, 2, 600, c, o, p, big) == EUNSUPPORTED, (c, o)
        assert _write(lib, p, 1, 2, 600, c, o, p, big, p, p, 10, p) == EUNSUPPORTED, (c, o)
    assert lib.seld_decode_workspace(16, 600, 16, 4) > 0 and lib.seld_decode_workspace(3, 7, 1, 64) > 0
    assert lib.seld_decode_workspace(1 << 22, 600, 14, 3) == 0
    assert _count(lib, p, 0, 1 << 22, 600, 14, 3, p, big) == EUNSUPPORTED
    # null pointers
    assert _count(lib, None, 0, 2, 600, 14, 3, p, need) == EINVAL
    assert _write(lib, None, 0, 2, 600, 14, 3, p, need, p, p, 10, p) == EINVAL
    assert _write(lib, p, 0, 2, 600, 14, 3, p, need, None, p, 10, p) == EINVAL
    assert _write(lib, p, 0, 2, 600, 14, 3, p, need, p, None, 10, p) == EINVAL
    assert _write(lib, p, 0, 2, 600, 14, 3, p, need, p, p, 10, None) == EINVAL
    assert _write(lib, p, 0, 2, 600, 14, 3, p, need, p, p, -1, p) == EINVAL
    # a missing or short workspace
    assert _count(lib, p, 0, 2, 600, 14, 3, None, need) == EWORKSPACE
    assert _count(lib, p, 0, 2, 600, 14, 3, p, need - 1) == EWORKSPACE
    assert _write(lib, p, 0, 2, 600, 14, 3, None, need, p, p, 10, p) == EWORKSPACE
    assert _write(lib, p, 0, 2, 600, 14, 3, p, need - 1, p, p, 10, p) == EWORKSPACE
    assert _write(lib, p, 0, 2, 600, 14, 3, p, 0, None, None, 0, p) == EWORKSPACE


def test_workspace_grows_with_the_frames():
    lib = pkg()._lib.lib()
    sizes = [lib.seld_decode_workspace(R, T, 14, 3) for R, T in [(1, 1), (1, 600), (2, 600), (500, 600)]]
    assert sizes == sorted(set(sizes)) and all(s % 8 == 0 for s in sizes)
    assert sizes[-1] <= 9 * 500 * 600                               # masks + a little: far below the inputs' 200 MB
    assert lib.seld_decode_workspace(500, 600, 14, 3) == lib.seld_decode_workspace(500, 600, 16, 4)


def test_host_inputs_and_mismatches_raise_before_the_device():
    p = pkg()
    L, H = p._lib, p.hip_ops
    with pytest.raises(L.SeldHipError, match="no CPU path"):
        H.decode_events(torch.zeros(4, 42), torch.zeros(4, 126))
    if not torch.cuda.is_available():
        with pytest.raises(L.SeldHipError, match="no HIP device"):
            p.utility_functions.gen_submission_list_task2(np.zeros((4, 42), np.float32), np.zeros((4, 126), np.float32))
    with pytest.raises(L.SeldHipError, match="unsupported dtype"):
        p.utility_functions.gen_submission_list_task2_OLD(np.zeros((4, 42), np.float16), np.zeros((4, 126), np.float16))


def test_cases_cover_what_the_fixture_is_for(golden):
    g = golden("decode")
    assert json.loads(str(g["meta"]))["stand_ins"] in ([], ["librosa"])
    by = {c["name"]: c for c in DECODE_CASES}
    assert g["no_events.rows"].shape == (0,) and g["no_events.rows"].dtype == np.float64
    assert g["no_events.keys"].shape == (0,)
    assert by["sigmoid_600"]["T"] == 600 and (by["sigmoid_600"]["classes"], by["sigmoid_600"]["overlaps"]) == (14, 3)
    n_slots = 600 * 42
    assert 0.005 < g["sparse_600.rows"].shape[0] / n_slots < 0.015
    for name in ("dense_21", "c16_o4_dense", "one_frame"):
        c = by[name]
        assert g[name + ".rows"].shape[0] == c["T"] * c["classes"] * c["overlaps"], name
    assert {(c["classes"], c["overlaps"]) for c in DECODE_CASES} >= {(14, 3), (5, 1), (16, 4)}
    assert {c["dtype"] for c in DECODE_CASES} == {"float32", "float64"}
    assert any(c["max_loc"] == 1.7 and c["dtype"] == "float32" for c in DECODE_CASES)
    assert any(c["T"] == 1 for c in DECODE_CASES) and any(c["T"] % 8 and c["T"] > 64 for c in DECODE_CASES)
    sed, _ = decode_inputs(by["ties"])
    assert {0.5, 1.5, 2.5, -0.5} <= set(np.unique(sed).tolist())
    # the negatives case: frames 0, 3, 5 and 11 hold active slots and cancel; they are absent from the rows
    sed, _ = decode_inputs(by["negatives"])
    r = np.round(sed)
    cancelled = [f for f in range(sed.shape[0]) if (r[f] != 0).any() and r[f].sum() == 0]
    assert cancelled == [0, 3, 5, 11]
    assert not set(g["negatives.rows"][:, 0].astype(int).tolist()) & set(cancelled)
    assert -0.6 in sed[2].astype(np.float32) and 2.0 in g["negatives.rows"][:, 0]
    # all-zero frames at the start, across the middle and at the end
    sed, _ = decode_inputs(by["zero_frames"])
    zero = np.nonzero(~sed.any(axis=1))[0].tolist()
    assert zero[:3] == [0, 1, 2] and set(range(60, 70)) <= set(zero) and zero[-1] == sed.shape[0] - 1
    # 1.7 is where the float32 multiply shows: the double product differs from the stored coordinates
    sed, doa = decode_inputs(by["maxloc_1p7"])
    rows = g["maxloc_1p7.rows"]
    j = int(rows[0, 1]) * 3 + int(g["maxloc_1p7.entries"][0, 4])
    src = doa[int(rows[0, 0]), 3 * j:3 * j + 3]
    assert np.array_equal(rows[0, 2:], (src * np.float32(1.7)).astype(np.float64))
    assert not np.array_equal(g["maxloc_1p7.rows"][:, 2:], g["float64_1p7.rows"][:, 2:])


def test_uniform_is_a_fixed_function():
    """The seeded draws do not depend on numpy's generators: the first values of two seeds are pinned."""
    u = uniform(11, (2, 3))
    assert (u.ravel() * (1 << 24)).tolist() == [7810373, 11350319, 2057796, 8972906, 11009731, 13807822]
    assert (uniform(0, (2,)) * (1 << 24)).tolist() == [14819496, 7239838]
    assert u.dtype == np.float64 and ((0 <= u) & (u < 1)).all()
    assert np.array_equal(u, uniform(11, (6,)).reshape(2, 3))
    assert not np.array_equal(u, uniform(12, (2, 3)))
    assert np.array_equal(u * (1 << 24), np.floor(u * (1 << 24)))


@pytest.mark.parametrize("case", DECODE_CASES, ids=CASE_IDS)
def test_fixture_agrees_with_oracle_bit_for_bit(golden, case):
    g = golden("decode")
    name = case["name"]
    sed, doa = decode_inputs(case)
    assert sed.dtype == np.dtype(case["dtype"]) and doa.dtype == sed.dtype
    rows, event = oracle_rows(sed, doa, case["max_loc"], case["classes"], case["overlaps"])
    ref = g[name + ".rows"]
    assert ref.dtype == np.float64 and int(g[name + ".old_same"]) == 1 and int(g[name + ".types"]) == 1
    if rows.shape[0] == 0:
        assert ref.shape == (0,)
    else:
        assert ref.shape == rows.shape
        assert ref.tobytes() == rows.tobytes()
    # the dict: the same rows grouped by frame, [class, x, y, z, event]
    entries = g[name + ".entries"]
    assert entries.shape == (rows.shape[0], 5)
    assert np.array_equal(entries[:, 0], rows[:, 1]) and entries[:, 1:4].tobytes() == rows[:, 2:].copy().tobytes()
    assert np.array_equal(entries[:, 4], event)
    frames, first = np.unique(rows[:, 0], return_index=True)
    assert np.array_equal(g[name + ".keys"], frames.astype(np.int64))         # first appearance = ascending frames
    assert np.array_equal(g[name + ".counts"], np.diff(np.append(first, rows.shape[0])))
    d = fixture_dict(g, name)
    assert list(d) == g[name + ".keys"].tolist()
