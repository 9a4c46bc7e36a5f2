"""Target encoding and segmentation on the device (csrc/labels.hip): hip_ops.encode_events, hip_ops.segment and the
drop-ins csv_to_matrix_task2, segment_task2, segment_waveforms against the reference's fixture (tests/golden/labels.npz).
Both operations move data and divide once in double, so everything is compared exactly: float64 byte for byte, float32
against the fixture rounded once."""
import numpy as np
import pytest
import torch

from tests.golden.decode_cases import uniform
from tests.golden.labels_cases import ENCODE_CASES, SEGMENT_CASES, SEGMENT_IDS, class_dict, segment_inputs
from tests.helpers import pkg
from tests.labels_helpers import (encode_events_host, encode_numpy, expected_rows, fixture_chunks, segment_numpy)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RETURNING = [c for c in ENCODE_CASES if not c["raises"]]
RAISING = [c for c in ENCODE_CASES if c["raises"]]
TORCH_DTYPES = {"float32": torch.float32, "float64": torch.float64}


def _frames(case):
    return int(case["dur"] / case["step"])


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _to_dev(first, last, cls, xyz, offsets):
    return (torch.from_numpy(np.asarray(first, dtype=np.int32)).to(DEV), torch.from_numpy(np.asarray(last, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.asarray(cls, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.asarray(xyz, dtype=np.float64).reshape(-1, 3)).to(DEV),
            torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(DEV))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", RETURNING, ids=[c["name"] for c in RETURNING])
def test_encode_events_against_fixture(golden, case, dtype):
    H = pkg().hip_ops
    g = golden("labels")
    ref = g[case["name"] + ".matrix"].astype(dtype)
    first, last, cls, xyz = encode_events_host(g, case["name"])
    E = first.shape[0]
    kw = dict(classes=14, overlaps=3, max_loc_value=case["max_loc"], no_overlaps=case["no_overlaps"], dtype=TORCH_DTYPES[dtype])
    for form in ("host", "device"):
        args = (first, last, cls, xyz, [0, E]) if form == "host" else _to_dev(first, last, cls, xyz, [0, E])
        out = H.encode_events(*args, _frames(case), **kw)
        assert out.is_cuda and out.dtype == TORCH_DTYPES[dtype] and out.shape == (1,) + ref.shape
        assert _same_bytes(out[0].cpu().numpy(), ref), (form, int((out[0].cpu().numpy() != ref).sum()))


@pytest.mark.parametrize("case", ENCODE_CASES, ids=[c["name"] for c in ENCODE_CASES])
def test_csv_to_matrix_task2_against_fixture(golden, case, tmp_path):
    pytest.importorskip("pandas")
    UF = pkg().utility_functions
    g = golden("labels")
    path = tmp_path / "labels.csv"
    path.write_bytes(bytes(g[case["name"] + ".csv"]))
    kw = dict(dur=case["dur"], step=case["step"], max_loc_value=case["max_loc"], no_overlaps=case["no_overlaps"])
    if case["raises"]:
        assert case["raises"] == "IndexError"
        with pytest.raises(IndexError):
            UF.csv_to_matrix_task2(str(path), class_dict(), **kw)
        return
    m = UF.csv_to_matrix_task2(str(path), class_dict(), **kw)
    assert isinstance(m, np.ndarray) and _same_bytes(m, g[case["name"] + ".matrix"])


def test_overflow_raises_index_error_and_bad_events_raise(golden):
    p = pkg()
    L, H = p._lib, p.hip_ops
    g = golden("labels")
    for case in RAISING:
        first, last, cls, xyz = encode_events_host(g, case["name"])
        E = first.shape[0]
        for args in ((first, last, cls, xyz, [0, E]), _to_dev(first, last, cls, xyz, [0, E])):
            with pytest.raises(IndexError):
                H.encode_events(*args, 600, no_overlaps=case["no_overlaps"])
        counters = torch.full((2,), -1, device=DEV, dtype=torch.int32)
        H.encode_events(*_to_dev(first, last, cls, xyz, [0, E]), 600, no_overlaps=case["no_overlaps"], counters=counters)
        assert counters.tolist() == [encode_numpy(first, last, cls, xyz, 600)[1], 0]
    # device inputs are judged by the kernel: class and frame out of range, offsets that do not ascend, too many events
    first, last, cls, xyz = encode_events_host(g, "three_same")
    E = first.shape[0]
    good = H.encode_events(*_to_dev(first, last, cls, xyz, [0, E]), 600)

    def changed(**kw):
        a = dict(first=first.copy(), last=last.copy(), cls=cls.copy(), xyz=xyz, offsets=[0, E])
        a.update(kw)
        return _to_dev(a["first"], a["last"], a["cls"], a["xyz"], a["offsets"])
    bad_cls, neg_cls, late, early = cls.copy(), cls.copy(), last.copy(), first.copy()
    bad_cls[2], neg_cls[0], late[1], early[3] = 14, -1, 600, -2
    for args in (changed(cls=bad_cls), changed(cls=neg_cls), changed(last=late), changed(first=early),
                 changed(offsets=[0, E + 1]), changed(offsets=[0, 5, 3, E]), changed(offsets=[-1, E])):
        out = torch.full((len(args[4]) - 1, 600, 168), float("nan"), device=DEV, dtype=torch.float64)
        with pytest.raises(L.SeldHipError, match="invalid"):
            H.encode_events(*args, 600, out=out)
        assert not torch.isnan(out).any()                    # still every element written, nothing outside
    n = H.ENCODE_MAX_EVENTS + 1
    many = _to_dev(np.arange(n) % 600, np.arange(n) % 600, np.arange(n) % 14, np.zeros((n, 3)), [0, n])
    with pytest.raises(L.SeldHipError, match="invalid"):
        H.encode_events(*many, 600, classes=14, overlaps=4)
    # an event whose last frame precedes its first covers nothing and is no error
    empty_last = last.copy()
    empty_last[4] = first[4] - 1
    out = H.encode_events(*changed(last=empty_last), 600)
    want, _ = encode_numpy(first, empty_last, cls, xyz, 600)
    assert _same_bytes(out[0].cpu().numpy(), want) and not torch.equal(out, good)


def _batch(golden):
    g = golden("labels")
    names = ["random_60", "empty", "three_same", "ends_at_dur", "empty", "ticks"]
    parts = [encode_events_host(g, n) for n in names]
    offsets = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])])
    first, last, cls, xyz = (np.concatenate([p[k] for p in parts]) for k in range(4))
    return g, names, parts, (first, last, cls, xyz, offsets)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_batch_equals_single_calls_and_two_runs_are_identical(golden, dtype):
    H = pkg().hip_ops
    g, names, parts, batch = _batch(golden)
    dev_args = _to_dev(*batch)
    out = H.encode_events(*dev_args, 600, dtype=dtype)
    assert out.shape == (len(names), 600, 168)
    singles = [H.encode_events(*p, [0, p[0].shape[0]], 600, dtype=dtype) for p in parts]
    assert torch.equal(out, torch.cat(singles)) and _same_bytes(out.cpu().numpy(), torch.cat(singles).cpu().numpy())
    for r, n in enumerate(names):
        assert _same_bytes(out[r].cpu().numpy(), g[n + ".matrix"].astype(out[r].cpu().numpy().dtype)), n
    again = H.encode_events(*dev_args, 600, dtype=dtype)
    host_form = H.encode_events(*batch, 600, dtype=dtype)
    assert _same_bytes(out.cpu().numpy(), again.cpu().numpy()) and _same_bytes(out.cpu().numpy(), host_form.cpu().numpy())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("no_overlaps", [False, True])
def test_every_output_element_is_written(golden, dtype, no_overlaps):
    H = pkg().hip_ops
    _, names, _, batch = _batch(golden)
    out = torch.full((len(names), 600, 56 if no_overlaps else 168), float("nan"), device=DEV, dtype=dtype)
    ret = H.encode_events(*_to_dev(*batch), 600, no_overlaps=no_overlaps, dtype=dtype, out=out)
    assert ret is out and not torch.isnan(out).any()
    assert torch.equal(out, H.encode_events(*batch, 600, no_overlaps=no_overlaps, dtype=dtype))
    # a buffer whose address is not a multiple of 16 takes the scalar stores
    flat = torch.full((out.numel() + 1,), float("nan"), device=DEV, dtype=dtype)
    shifted = flat[1:].view(out.shape)
    assert shifted.data_ptr() % 16 != 0
    H.encode_events(*_to_dev(*batch), 600, no_overlaps=no_overlaps, dtype=dtype, out=shifted)
    assert torch.equal(shifted, out) and torch.isnan(flat[0])


SWEEP = [  # seed, R, frames, classes, overlaps, events per recording, longest event, max_loc, no_overlaps
    (1, 1, 1, 14, 3, 5, 1, 2.0, False), (2, 3, 7, 14, 3, 12, 4, 1.7, False), (3, 5, 65, 16, 4, 90, 20, 0.3, False),
    (4, 2, 600, 1, 64, 700, 300, 2.0, False), (5, 4, 33, 5, 1, 6, 10, 2.0, False), (6, 2, 129, 64, 1, 200, 50, 3.3, True),
    (7, 70, 9, 14, 3, 10, 3, 2.0, True), (8, 1, 1000, 7, 9, 4096, 40, 1.1, False), (9, 3, 50, 14, 3, 150, 30, 2.0, False),
]


@pytest.mark.parametrize("p", SWEEP, ids=[f"s{p[0]}_{p[1]}x{p[2]}x{p[3]}x{p[4]}" for p in SWEEP])
def test_sweep_against_the_numpy_statement(p):
    """Other layouts, frame counts off the tile size, the staging limit, cells that overflow: the target and the overflow
    count against tests/labels_helpers.encode_numpy (which the CPU tests hold to the reference's fixture)."""
    H = pkg().hip_ops
    seed, R, frames, classes, overlaps, per_rec, longest, max_loc, no_overlaps = p
    u = uniform(seed, (R * per_rec, 6))
    first = (u[:, 0] * frames).astype(np.int64)
    last = np.minimum(first + (u[:, 1] * longest).astype(np.int64) - (u[:, 1] < 0.05), frames - 1)      # a few empty events
    cls = (u[:, 2] * classes).astype(np.int64)
    xyz = 4.0 * u[:, 3:] - 2.0
    offsets = np.arange(R + 1) * per_rec
    want, over = zip(*(encode_numpy(first[a:b], last[a:b], cls[a:b], xyz[a:b], frames, classes, overlaps, max_loc, no_overlaps)
                       for a, b in zip(offsets[:-1], offsets[1:])))
    for dtype in (torch.float64, torch.float32):
        counters = torch.full((2,), -1, device=DEV, dtype=torch.int32)
        out = H.encode_events(*_to_dev(first, last, cls, xyz, offsets), frames, classes, overlaps, max_loc, no_overlaps, dtype,
                              counters=counters)
        ref = np.stack(want).astype(np.float32 if dtype == torch.float32 else np.float64)
        print(f"sweep {p}: active {int(ref[..., :ref.shape[-1] // 4].sum())}, overflowing cells {sum(over)}")
        assert counters.tolist() == [sum(over), 0]
        assert _same_bytes(out.cpu().numpy(), ref)


def test_round_trip_through_decode_events(golden):
    """decode_events(encode_events(rows)) gives back [frame, class, x, y, z] of every covered frame, sorted by (frame, class,
    slot), exactly: division and multiplication by 2.0 are exact."""
    H = pkg().hip_ops
    g = golden("labels")
    for name in ("random_60", "three_same", "ends_at_dur", "ticks", "empty"):
        first, last, cls, xyz = encode_events_host(g, name)
        target = H.encode_events(first, last, cls, xyz, [0, first.shape[0]], 600)
        rows, event, offsets = H.decode_events(target[0, :, :42].contiguous(), target[0, :, 42:].contiguous(), 2.0, 14, 3)
        want, want_event = expected_rows(first, last, cls, xyz)
        assert _same_bytes(rows.cpu().numpy(), want), name
        assert np.array_equal(event.cpu().numpy(), want_event) and offsets.tolist() == [0, want.shape[0]]


def _chunks_equal(got, ref, name):
    assert len(got) == len(ref), name
    for i, (a, b) in enumerate(zip(got, ref)):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.shape == b.shape and np.array_equal(a.astype(b.dtype), b), (name, i)


@pytest.mark.parametrize("case", SEGMENT_CASES, ids=SEGMENT_IDS)
def test_segment_functions_against_fixture(golden, case):
    UF = pkg().utility_functions
    g = golden("labels")
    fn = getattr(UF, case["fn"])
    p, t = segment_inputs(case)
    for form in ("numpy", "device"):
        a, b = (p, t) if form == "numpy" else (torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV))
        if case["raises"] or case["ragged"]:
            with pytest.raises(ValueError):
                fn(a, b, **case["kw"])
            continue
        X, Y = fn(a, b, **case["kw"])
        Xr, Yr = fixture_chunks(g, case["name"])
        assert isinstance(X, list) and isinstance(Y, list)
        if form == "numpy":
            assert all(isinstance(x, np.ndarray) and x.dtype == p.dtype for x in X)
            assert all(isinstance(y, np.ndarray) and y.dtype == t.dtype for y in Y)
        else:                                                # views into the two stacked device results, no host copy
            assert all(x.is_cuda and x.dtype == a.dtype for x in X) and all(y.is_cuda and y.dtype == b.dtype for y in Y)
            assert X[1].data_ptr() == X[0].data_ptr() + X[0].numel() * X[0].element_size()
            assert Y[1].data_ptr() == Y[0].data_ptr() + Y[0].numel() * Y[0].element_size()
        _chunks_equal(X, Xr, case["name"])
        _chunks_equal(Y, Yr, case["name"])


SEG_SWEEP = [  # shape, seg_len, hop, segments (None: default), dtype, element offset of the source
    ((600, 168), 50, 25, None, torch.float64, 0), ((600, 168), 50, 25, None, torch.float32, 0),
    ((155, 20), 50, 25, None, torch.float64, 0), ((37, 5), 7, 3, None, torch.float32, 0), ((37, 5), 7, 3, 20, torch.float64, 1),
    ((64, 8), 16, 16, None, torch.float32, 1), ((9, 1), 4, 1, None, torch.float32, 0), ((3, 4, 50), 8, 6, None, torch.float64, 0),
    ((100, 3), 200, 40, 4, torch.float32, 0), ((4800, 6), 400, 200, None, torch.float32, 3),
]


@pytest.mark.parametrize("time_first", [True, False])
@pytest.mark.parametrize("p", SEG_SWEEP, ids=[f"{'x'.join(map(str, p[0]))}_L{p[1]}_h{p[2]}_{str(p[4])[-2:]}_o{p[5]}" for p in SEG_SWEEP])
def test_segment_against_numpy_slicing(p, time_first):
    """The cut by rows (time_first) and by the last axis against plain slicing with zero padding: aligned and unaligned
    sources, odd lengths and hops, more segments than the signal holds."""
    H = pkg().hip_ops
    shape, seg_len, hop, segments, dtype, offset = p
    n = int(np.prod(shape))
    flat = torch.arange(1, n + 1 + offset, dtype=torch.float64).to(dtype).to(DEV)
    x = flat[offset:].view(shape)
    assert x.is_contiguous() and (offset == 0 or x.data_ptr() % 16 != 0)
    out = H.segment(x, seg_len, hop, time_first=time_first, segments=segments)
    length = shape[0] if time_first else shape[-1]
    count = len(range(0, length, hop)) if segments is None else segments
    want = segment_numpy(x.cpu().numpy(), seg_len, hop, count, time_first)
    assert out.dtype == dtype and out.is_contiguous() and _same_bytes(out.cpu().numpy(), want)


def test_segment_task2_at_the_recording_shape():
    """(16, 256, 4800) float32 features and a (600, 168) target, the challenge's recording: both input conventions
    agree, and sampled chunks equal plain slicing of the inputs."""
    UF = pkg().utility_functions
    g = torch.Generator().manual_seed(5)
    p = torch.rand(16, 256, 4800, generator=g)
    t = torch.rand(600, 168, generator=g, dtype=torch.float64)
    X, Y = UF.segment_task2(p.to(DEV), t.to(DEV))
    assert len(X) == len(Y) == 24 and X[0].shape == (16, 256, 400) and Y[0].shape == (50, 168)
    pn, tn = p.numpy(), t.numpy()
    wy = segment_numpy(tn.reshape(168, 600), 50, 25, 24).reshape(24, 50, 168)
    for s in (0, 1, 11, 22, 23):
        wx = np.zeros((16, 256, 400), np.float32)
        piece = pn[:, :, s * 200:s * 200 + 400]
        wx[:, :, :piece.shape[-1]] = piece
        assert np.array_equal(X[s].cpu().numpy(), wx), s
        assert np.array_equal(Y[s].cpu().numpy(), wy[s]), s
    assert not X[23][:, :, 200:].any() and X[23][:, :, :200].any()


def test_both_kernels_replay_from_a_graph(golden):
    """encode_events (with its own counters: no read-back) and segment recorded with torch.cuda.graph and replayed on
    new inputs equal the eager results."""
    H = pkg().hip_ops
    g = golden("labels")
    first, last, cls, xyz = encode_events_host(g, "random_60")
    args = _to_dev(first, last, cls, xyz, [0, first.shape[0]])
    feats = torch.arange(1, 2 * 3 * 1237 + 1, dtype=torch.float32, device=DEV).view(2, 3, 1237)

    def run(counters):
        target = H.encode_events(*args, 600, dtype=torch.float64, counters=counters)
        return target, H.segment(feats, 400, 200), H.segment(target[0], 50, 25, time_first=True)
    counters = torch.zeros(2, device=DEV, dtype=torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(counters)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run(counters)
    args[3].mul_(0.5)                                        # new coordinates, new features
    args[2].copy_((args[2] + 3) % 14)
    feats.add_(7.0)
    counters.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert counters.tolist() == [0, 0]
    eager = run(torch.zeros(2, device=DEV, dtype=torch.int32))
    for k, (a, b) in enumerate(zip(static, eager)):
        assert torch.equal(a, b), k
    want, _ = encode_numpy(first, last, (cls + 3) % 14, xyz * 0.5, 600)
    assert _same_bytes(static[0][0].cpu().numpy(), want)
