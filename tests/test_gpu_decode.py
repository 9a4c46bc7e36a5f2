"""Event decoding on the device (csrc/decode.hip): gen_submission_list_task2, gen_submission_list_task2_OLD,
hip_ops.decode_events and train.predict_test against the reference's fixture (tests/golden/decode.npz) and the oracle.
Everything is compared exactly: the integers, the order, and the coordinates, which are one correctly rounded multiply."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import seld_oracle as O
from tests.decode_helpers import fixture_dict, oracle_rows
from tests.golden.decode_cases import CASE_IDS, DECODE_CASES, decode_inputs, uniform
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _kw(case):
    return dict(max_loc_value=case["max_loc"], num_classes=case["classes"], max_overlaps=case["overlaps"])


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _decode(sed, doa, **kw):
    rows, event, offsets = pkg().hip_ops.decode_events(sed, doa, **kw)
    assert rows.dtype == torch.float64 and event.dtype == torch.int32 and offsets.dtype == torch.int64
    assert rows.is_cuda and event.is_cuda and offsets.is_cuda
    assert rows.dim() == 2 and rows.shape[1] == 5 and event.shape == (rows.shape[0],)
    return rows.cpu().numpy(), event.cpu().numpy(), offsets.cpu().numpy()


def _random_batch(seed, R, T, classes, overlaps, active, dtype=np.float32, negatives=False):
    n = classes * overlaps
    u = uniform(seed, (R, T, n))
    sed = np.where(u < active, 0.5 + 0.5 * u / max(active, 1e-9) + 0.001, 0.499 * (u - active) / max(1 - active, 1e-9))
    if negatives:                                         # a tenth of the slots negated: cancelling frames do occur
        sed = np.where(uniform(seed + 7, (R, T, n)) < 0.1, -sed, sed)
    doa = 2.0 * uniform(seed + 1000, (R, T, 3 * n)) - 1.0
    return np.ascontiguousarray(sed.astype(dtype)), np.ascontiguousarray(doa.astype(dtype))


@pytest.mark.parametrize("case", DECODE_CASES, ids=CASE_IDS)
def test_fixture_cases_exact(golden, case):
    UF = pkg().utility_functions
    g = golden("decode")
    name = case["name"]
    ref = g[name + ".rows"]
    ref_dict = fixture_dict(g, name)
    sed, doa = decode_inputs(case)
    kw = dict(_kw(case), num_frames=case["T"])
    for form in ("numpy", "device"):
        a, b = (sed, doa) if form == "numpy" else (torch.from_numpy(sed).to(DEV), torch.from_numpy(doa).to(DEV))
        rows, d = UF.gen_submission_list_task2(a, b, **kw)
        old = UF.gen_submission_list_task2_OLD(a, b, **kw)
        assert isinstance(rows, np.ndarray) and isinstance(old, np.ndarray)
        assert _same_bytes(rows, ref), (form, rows.shape, ref.shape)
        assert _same_bytes(old, ref), form
        assert d == ref_dict and list(d) == list(ref_dict), form
        assert all(type(k) is int for k in d), form
        assert all([type(x) for x in e] == [int, float, float, float, int] for v in d.values() for e in v), form
    rows, event, offsets = _decode(torch.from_numpy(sed).to(DEV), torch.from_numpy(doa).to(DEV), **_kw(case))
    assert rows.shape == (g[name + ".entries"].shape[0], 5)
    if rows.shape[0]:
        assert _same_bytes(rows, ref)
    assert np.array_equal(event, g[name + ".entries"][:, 4].astype(np.int32))
    assert offsets.tolist() == [0, rows.shape[0]]


def test_batch_equals_single_calls_and_offsets_split_it(golden):
    """(R, T, n): the 14 x 3 float32 fixture cases cut to a common length, with event-free recordings in the middle."""
    T = 21
    cases = [c for c in DECODE_CASES if (c["classes"], c["overlaps"], c["dtype"]) == (14, 3, "float32") and c["T"] >= T
             and c["max_loc"] == 2.0]
    assert len(cases) >= 4
    seds, doas = zip(*(tuple(a[:T] for a in decode_inputs(c)) for c in cases))
    zero = np.zeros_like(seds[0])
    seds = list(seds[:2]) + [zero, zero] + list(seds[2:]) + [zero]
    doas = list(doas[:2]) + [doas[0], doas[1]] + list(doas[2:]) + [doas[0]]
    sed, doa = torch.from_numpy(np.stack(seds)).to(DEV), torch.from_numpy(np.stack(doas)).to(DEV)
    rows, event, offsets = _decode(sed, doa)
    assert offsets[0] == 0 and offsets[-1] == rows.shape[0] and (np.diff(offsets) >= 0).all()
    singles = [_decode(sed[r], doa[r]) for r in range(sed.shape[0])]
    assert _same_bytes(rows, np.concatenate([s[0] for s in singles]))
    assert np.array_equal(event, np.concatenate([s[1] for s in singles]))
    assert np.diff(offsets).tolist() == [s[0].shape[0] for s in singles]
    assert np.diff(offsets)[[2, 3, -1]].tolist() == [0, 0, 0]
    for r in range(sed.shape[0]):
        want, want_event = oracle_rows(seds[r], doas[r], 2.0, 14, 3)
        assert _same_bytes(rows[offsets[r]:offsets[r + 1]], want), r
        assert np.array_equal(event[offsets[r]:offsets[r + 1]], want_event), r


SWEEP = [  # seed, R, T, classes, overlaps, active, dtype, negatives, max_loc
    (1, 1, 1, 14, 3, 0.5, np.float32, False, 2.0), (2, 3, 7, 14, 3, 0.2, np.float32, True, 2.0),
    (3, 2, 64, 14, 3, 0.05, np.float32, False, 1.7), (4, 5, 65, 14, 3, 0.9, np.float32, True, 2.0),
    (5, 4, 63, 1, 1, 0.3, np.float32, False, 2.0), (6, 2, 200, 16, 4, 1.0, np.float32, False, 0.9),
    (7, 7, 129, 2, 5, 0.4, np.float64, True, 1.7), (8, 1, 1000, 7, 9, 0.01, np.float64, False, 2.0),
    (9, 9, 31, 64, 1, 0.6, np.float32, True, 3.3), (10, 130, 1, 14, 3, 0.3, np.float32, True, 2.0),
    (11, 6, 100, 14, 3, 0.0, np.float32, False, 2.0), (12, 3, 128, 1, 64, 0.97, np.float64, True, 2.0),
]


@pytest.mark.parametrize("p", SWEEP, ids=[f"s{p[0]}_{p[1]}x{p[2]}x{p[3]}x{p[4]}" for p in SWEEP])
def test_sweep_against_oracle(p):
    seed, R, T, classes, overlaps, active, dtype, negatives, max_loc = p
    sed, doa = _random_batch(seed, R, T, classes, overlaps, active, dtype, negatives)
    kw = dict(max_loc_value=max_loc, num_classes=classes, max_overlaps=overlaps)
    rows, event, offsets = _decode(torch.from_numpy(sed).to(DEV), torch.from_numpy(doa).to(DEV), **kw)
    want = [oracle_rows(sed[r], doa[r], max_loc, classes, overlaps) for r in range(R)]
    # the row count per recording is the oracle's number of active slots
    counts = [int(O.decode_events(sed[r], doa[r], max_loc, classes, overlaps)[0].sum()) for r in range(R)]
    print(f"sweep {p[:6]}: rows {rows.shape[0]}, per recording {counts[:8]}")
    assert np.diff(offsets).tolist() == counts
    assert _same_bytes(rows, np.concatenate([w[0] for w in want]))
    assert np.array_equal(event, np.concatenate([w[1] for w in want]))
    if negatives and R * T >= 200 and active >= 0.2 and classes * overlaps <= 10:
        r = np.round(sed)
        assert ((r != 0).any(-1) & (r.sum(-1) == 0)).any()         # the cancelling-frame rule was exercised


def test_large_case_counts_and_sampled_recordings():
    """500 x 600 x 42 as tools/measure_rows.py: the total against a host popcount of the rule, sampled recordings
    against the oracle, and two runs bit-identical."""
    g = torch.Generator().manual_seed(3)
    sed = torch.rand(500, 600, 42, generator=g)
    doa = torch.rand(500, 600, 126, generator=g) * 2 - 1
    sed_n, doa_n = sed.numpy(), doa.numpy()
    r = np.round(sed_n)
    active = (r != 0) & (r.sum(-1, keepdims=True) != 0)
    per_rec = active.reshape(500, -1).sum(1)
    sd, dd = sed.to(DEV), doa.to(DEV)
    rows, event, offsets = _decode(sd, dd)
    print(f"large case: {rows.shape[0]} rows of {sed.numel()} slots")
    assert rows.shape[0] == int(active.sum())
    assert np.array_equal(np.diff(offsets), per_rec)
    for k in (0, 1, 137, 250, 498, 499):
        want, want_event = oracle_rows(sed_n[k], doa_n[k], 2.0, 14, 3)
        assert int(O.decode_events(sed_n[k], doa_n[k])[0].sum()) == offsets[k + 1] - offsets[k]
        assert _same_bytes(rows[offsets[k]:offsets[k + 1]], want), k
        assert np.array_equal(event[offsets[k]:offsets[k + 1]], want_event), k
    rows2, event2, offsets2 = _decode(sd, dd)
    assert _same_bytes(rows, rows2) and _same_bytes(event, event2) and _same_bytes(offsets, offsets2)


def test_two_runs_identical_and_numpy_equals_device():
    UF = pkg().utility_functions
    sed, doa = _random_batch(21, 1, 600, 14, 3, 0.1, np.float32, True)
    sed, doa = sed[0], doa[0]
    a = UF.gen_submission_list_task2(sed, doa)
    b = UF.gen_submission_list_task2(torch.from_numpy(sed).to(DEV), torch.from_numpy(doa).to(DEV))
    c = UF.gen_submission_list_task2(sed, doa)
    assert _same_bytes(a[0], b[0]) and _same_bytes(a[0], c[0]) and a[1] == b[1] == c[1]
    assert list(a[1]) == list(b[1])
    # a non-contiguous device view decodes as its contiguous copy
    wide = torch.from_numpy(np.concatenate([sed, sed], 1)).to(DEV)
    d = UF.gen_submission_list_task2_OLD(wide[:, :42], torch.from_numpy(doa).to(DEV))
    assert _same_bytes(d, a[0])


def test_refusals_raise_and_write_nothing():
    p = pkg()
    L, H = p._lib, p.hip_ops
    sed = torch.full((2, 10, 42), 0.9, device=DEV)
    doa = torch.full((2, 10, 126), 0.25, device=DEV)
    bad = [(sed, doa[:, :, :125].contiguous(), {}), (sed, doa[:, :9], {}), (sed[0], doa, {}), (sed, doa.double(), {}),
           (sed.half(), doa.half(), {}), (sed, doa, dict(num_classes=13)), (sed, doa, dict(max_overlaps=2)),
           (sed.cpu(), doa, {}), (sed[None], doa[None], {}),
           (torch.zeros(2, 10, 66, device=DEV), torch.zeros(2, 10, 198, device=DEV), dict(num_classes=22))]
    for a, b, kw in bad:
        with pytest.raises(L.SeldHipError):
            H.decode_events(a, b, **kw)
    # the C entries: sentinel-filled outputs and workspace stay as they are
    lib = L.lib()
    need = lib.seld_decode_workspace(2, 10, 14, 3)
    ws = torch.full((need // 8,), -7, device=DEV, dtype=torch.int64)
    rows = torch.full((840, 5), -3.0, device=DEV, dtype=torch.float64)
    event = torch.full((840,), -5, device=DEV, dtype=torch.int32)
    offs = torch.full((3,), -9, device=DEV, dtype=torch.int64)
    s = L.current_stream()

    def count(sed_p, classes, overlaps, ws_bytes, frames=10):
        return lib.seld_decode_count(sed_p, 0, 2, frames, classes, overlaps, L.ptr(ws), ws_bytes, s)

    def write(doa_p, classes, overlaps, ws_bytes, cap=840, rows_p=None):
        return lib.seld_decode_write(doa_p, 0, 2, 10, classes, overlaps, 2.0, L.ptr(ws), ws_bytes,
                                     L.ptr(rows) if rows_p is None else rows_p, L.ptr(event), cap, L.ptr(offs), s)
    assert count(L.ptr(sed), 22, 3, need) == -4 and write(L.ptr(doa), 22, 3, need) == -4
    assert count(L.ptr(sed), 14, 3, need - 8) == -2 and write(L.ptr(doa), 14, 3, need - 8) == -2
    assert count(None, 14, 3, need) == -1 and write(None, 14, 3, need) == -1
    assert count(L.ptr(sed), 14, 3, need, frames=0) == -1 and write(L.ptr(doa), 14, 3, need, cap=-1) == -1
    assert write(L.ptr(doa), 14, 3, need, rows_p=ctypes.c_void_p(0)) == -1
    torch.cuda.synchronize()
    assert (ws == -7).all() and (rows == -3.0).all() and (event == -5).all() and (offs == -9).all()
    # and the accepted call on the same buffers fills exactly E rows
    assert count(L.ptr(sed), 14, 3, need) == 0 and write(L.ptr(doa), 14, 3, need) == 0
    torch.cuda.synchronize()
    assert int(ws[0]) == 840 and offs.tolist() == [0, 420, 840]
    assert (rows[:, 2:] == 0.5).all() and (event.view(-1, 3) == torch.arange(3, device=DEV, dtype=torch.int32)).all()
    # a capacity below E: the rows beyond it are not written
    rows.fill_(-3.0)
    event.fill_(-5)
    assert write(L.ptr(doa), 14, 3, need, cap=100) == 0
    torch.cuda.synchronize()
    assert (rows[:100, 2:] == 0.5).all() and (rows[100:] == -3.0).all() and (event[100:] == -5).all()


def test_predict_test_matches_oracle_decoding():
    """A tiny DualQ model, a two-batch loader: predict_test equals the oracle's decoding of the model's own outputs."""
    p = pkg()
    kw = dict(time_dim=64, freq_dim=128, input_channels=8, output_classes=14, domain='DQ', domain_classifier='DQ',
              cnn_filters=[16, 16, 16], pool_size=[[8, 2], [8, 2], [2, 2]], pool_time='TCN', D=[10],
              dilation_mode='fibonacci', G=32, U=16, V=[16, 16], V_kernel_size=3, fc_layers=[16],
              fc_activations='linear', fc_dropout='Last', dropout_perc=0.0, spatial_dropout_rate=0.0,
              class_overlaps=3, use_bias_conv=0, use_bias_linear=1, batch_norm='BN')
    torch.manual_seed(1)
    inner = p.model.SELD_Model(**kw)
    O.closed_form_fill_(list(inner.state_dict().items()))
    inner = inner.to(DEV)

    class Spread:
        """The model with its activities spread over (0, 1.8), so that slots land on both sides of one half."""
        def eval(self):
            inner.eval()
            return self

        def __call__(self, x):
            sed, doa = inner(x)
            gain = 0.2 + 1.6 * torch.from_numpy(uniform(5, tuple(sed.shape[1:]))).to(sed)
            return sed * gain, doa

    xs = [O.closed_form_input((2, 8, 128, 64)), O.closed_form_input((3, 8, 128, 64)).flip(0) * 0.7]
    loader = [(x, torch.zeros(x.shape[0], 1)) for x in xs]
    got = p.train.predict_test(Spread(), torch.device(DEV), loader, max_loc_value=1.7)
    assert len(got) == 5
    model = Spread().eval()
    total = 0
    with torch.no_grad():
        outs = [model(x.to(DEV)) for x in xs]
    k = 0
    for sed, doa in outs:
        assert sed.shape[-1] == 42
        for r in range(sed.shape[0]):
            want, _ = oracle_rows(sed[r].cpu().numpy(), doa[r].cpu().numpy(), 1.7, 14, 3)
            assert got[k].dtype == np.float64 and got[k].shape == want.shape
            assert got[k].tobytes() == want.tobytes(), k
            total += want.shape[0]
            k += 1
    print(f"predict_test: {total} rows over 5 recordings of {outs[0][0].shape[1]} frames")
    assert total > 0


def test_mixed_dtypes_follow_doa():
    """numpy inputs of different dtypes: doa's dtype decides the multiply, as in the reference; sed is rounded exactly."""
    p = pkg()
    UF, L = p.utility_functions, p._lib
    sed, doa = _random_batch(31, 1, 40, 14, 3, 0.2, np.float32, True)
    sed, doa = sed[0], doa[0]
    ints = np.round(sed * 3).astype(np.int64)
    for s_in, d_in in ((sed, doa.astype(np.float64)), (ints, doa), (ints, doa.astype(np.float64)), (ints != 0, doa),
                       (ints.astype(np.int8), doa.astype(np.float64))):
        want, want_event = oracle_rows(s_in, d_in, 1.7, 14, 3)
        rows, d = UF.gen_submission_list_task2(s_in, d_in, max_loc_value=1.7)
        assert _same_bytes(rows, want), (s_in.dtype, d_in.dtype)
        assert [e[4] for v in d.values() for e in v] == want_event.tolist()
        assert _same_bytes(UF.gen_submission_list_task2_OLD(s_in, d_in, max_loc_value=1.7), want)
    dev_rows = UF.gen_submission_list_task2_OLD(torch.from_numpy(sed).to(DEV), torch.from_numpy(doa.astype(np.float64)).to(DEV))
    assert _same_bytes(dev_rows, oracle_rows(sed, doa.astype(np.float64), 2.0, 14, 3)[0])
    with pytest.raises(L.SeldHipError, match="float64 sed with float32 doa"):
        UF.gen_submission_list_task2(sed.astype(np.float64), doa)
    with pytest.raises(L.SeldHipError, match="both be numpy arrays or both device tensors"):
        UF.gen_submission_list_task2(sed, torch.from_numpy(doa).to(DEV))
