"""hip_ops.gather_rows / epoch_step_end (csrc/loader.hip) and train.ResidentLoader against torch indexing and torch's
DataLoader: every comparison is bit for bit, the kernels only move data (and take one fp32 running mean)."""
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.5
B = 5


def _arrays(n_rows, row_x, row_y, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_rows, row_x, generator=g).to(DEV) if row_x else None
    y = torch.randn(n_rows, row_y, generator=g).to(DEV) if row_y else None
    return x, y


def _buffers(row_x, row_y):
    return (torch.full((B, row_x), SENTINEL, device=DEV) if row_x else None,
            torch.full((B, row_y), SENTINEL, device=DEV) if row_y else None)


def _expect(all_, index, start, count, row):
    out = torch.full((B, row), SENTINEL, device=DEV)
    out[:count] = all_[index[start:start + count]]
    return out


@pytest.mark.parametrize("row", [1, 3, 4, 5, 255, 1024, 4099])
@pytest.mark.parametrize("n_rows", [1, 7])
@pytest.mark.parametrize("count", [1, 5])
def test_gather_rows_equals_torch_indexing(row, n_rows, count):
    """Row lengths on both sides of the 16-byte paths (1, 3, 5: every other row unaligned; 255 / 4099: head and tail; 4099:
    more than one 4096-float tile), repeated indices, x alone, y alone, and both with different row lengths; rows >= count
    keep the sentinel.  `start` and the device cursor select the same rows."""
    H = pkg().hip_ops
    row_y = row + 1 if row < 4099 else 7
    x, y = _arrays(n_rows, row, row_y, seed=row + n_rows)
    index = torch.randint(0, n_rows, (3 * B,), generator=torch.Generator().manual_seed(count)).to(DEV)
    for start in (0, 2 * B):
        want_x, want_y = _expect(x, index, start, count, row), _expect(y, index, start, count, row_y)
        for pick_x, pick_y in ((True, False), (False, True), (True, True)):
            ox, oy = _buffers(row if pick_x else 0, row_y if pick_y else 0)
            H.gather_rows(x if pick_x else None, y if pick_y else None, index, ox, oy, start=start, count=count)
            assert ox is None or torch.equal(ox, want_x)
            assert oy is None or torch.equal(oy, want_y)
        ox, oy = _buffers(row, row_y)
        cursor = torch.tensor([start // B], device=DEV, dtype=torch.int32)
        H.gather_rows(x, y, index, ox, oy, cursor=cursor, count=count)
        assert torch.equal(ox, want_x) and torch.equal(oy, want_y)
        assert int(cursor) == start // B                      # read, never written


def test_gather_rows_cursor_stride_and_start_address_a_ranks_share():
    """position = cursor * stride + start + b: the second rank's two rows of the second global batch of four."""
    H = pkg().hip_ops
    x, y = _arrays(9, 6, 2)
    index = torch.randperm(9, generator=torch.Generator().manual_seed(1)).to(DEV)
    ox, oy = torch.zeros(2, 6, device=DEV), torch.zeros(2, 2, device=DEV)
    H.gather_rows(x, y, index, ox, oy, cursor=torch.tensor([1], device=DEV, dtype=torch.int32), start=2, stride=4)
    assert torch.equal(ox, x[index[6:8]]) and torch.equal(oy, y[index[6:8]])


@pytest.mark.parametrize("row", [3, 1024])
def test_gather_rows_zero_fills_rows_of_invalid_indices(row):
    """Indices -1 and n_rows, and positions past the end of `index`, give zero rows; their neighbours are correct."""
    H = pkg().hip_ops
    n_rows = 7
    x, y = _arrays(n_rows, row, 2)
    index = torch.tensor([3, -1, 6, n_rows, 0, 2, 5], device=DEV)
    ox, oy = _buffers(row, 2)
    H.gather_rows(x, y, index, ox, oy, start=0)
    for b, i in enumerate(index[:B].tolist()):
        ok = 0 <= i < n_rows
        assert torch.equal(ox[b], x[i] if ok else torch.zeros(row, device=DEV)), b
        assert torch.equal(oy[b], y[i] if ok else torch.zeros(2, device=DEV)), b
    ox, oy = _buffers(row, 2)
    H.gather_rows(x, y, index, ox, oy, start=5)                 # positions 5, 6 exist; 7, 8, 9 do not
    assert torch.equal(ox[:2], x[index[5:7]]) and not ox[2:].any() and not oy[2:].any()
    H.gather_rows(x, y, index, ox, oy, start=-1, count=2)       # position -1 does not exist either
    assert not ox[0].any() and torch.equal(ox[1], x[3])


def test_gather_rows_refuses_invalid_arguments():
    H, L = pkg().hip_ops, pkg()._lib
    x, y = _arrays(4, 8, 2)
    index = torch.arange(4, device=DEV)
    ox, oy = _buffers(8, 2)
    for kwargs in (dict(count=B + 1), dict(count=0), dict(count=-1), dict(stride=-1, cursor=torch.zeros(1, device=DEV, dtype=torch.int32))):
        with pytest.raises(L.SeldHipError, match="SELD_EINVAL"):
            H.gather_rows(x, y, index, ox, oy, **kwargs)
    lib, s = L.lib(), L.current_stream()
    for call in (lambda: lib.seld_gather_rows(L.ptr(x), 8, L.ptr(ox), None, 0, None, None, 4, 4, None, B, 0, B, B, s),        # no index
                 lambda: lib.seld_gather_rows(None, 0, None, None, 0, None, L.ptr(index), 4, 4, None, B, 0, B, B, s),         # neither pair
                 lambda: lib.seld_gather_rows(L.ptr(x), 8, None, None, 0, None, L.ptr(index), 4, 4, None, B, 0, B, B, s),     # half a pair
                 lambda: lib.seld_gather_rows(L.ptr(x), 0, L.ptr(ox), None, 0, None, L.ptr(index), 4, 4, None, B, 0, B, B, s),
                 lambda: lib.seld_gather_rows(L.ptr(x), 8, L.ptr(ox), None, 0, None, L.ptr(index), 0, 4, None, B, 0, B, B, s),
                 lambda: lib.seld_gather_rows(L.ptr(x), 8, L.ptr(ox), None, 0, None, L.ptr(index), 4, 0, None, B, 0, B, B, s),
                 lambda: lib.seld_gather_rows(L.ptr(x), 8, L.ptr(ox), None, 0, None, L.ptr(index), 4, 4, None, B, 0, 0, 0, s),
                 lambda: lib.seld_gather_rows(L.ptr(x), 8, L.ptr(ox), None, 0, None, L.ptr(index), 4, 4, None, B, 0, 70000, 70000, s),
                 lambda: lib.seld_epoch_step_end(None, L.ptr(ox), L.ptr(index), s)):
        assert call() == -1
    torch.cuda.synchronize()
    assert bool((ox == SENTINEL).all()) and bool((oy == SENTINEL).all())        # nothing was launched
    with pytest.raises(L.SeldHipError):
        H.gather_rows(x, y, index.to(torch.int32), ox, oy)
    with pytest.raises(L.SeldHipError):
        H.gather_rows(x, y, index, ox[:, :4], oy)                               # not contiguous / another row length
    with pytest.raises(L.SeldHipError):
        H.gather_rows(x, None, index, ox, oy)


def test_recorded_gather_and_step_end_walk_through_the_batches():
    """gather_rows(cursor) + epoch_step_end recorded in ONE graph and replayed three times, the loss scalar rewritten
    between replays: batches 0, 1, 2 arrive, the cursor ends at 3, and the mean is the fp32 recurrence of train.main's epoch loop
    computed by torch on the host, bit for bit."""
    H = pkg().hip_ops
    x, y = _arrays(12, 1030, 3, seed=4)
    index = torch.randperm(12, generator=torch.Generator().manual_seed(2)).to(DEV)
    ox, oy = torch.zeros(4, 1030, device=DEV), torch.zeros(4, 3, device=DEV)
    cursor = torch.zeros(1, device=DEV, dtype=torch.int32)
    mean = torch.zeros(1, device=DEV)
    loss = torch.zeros((), device=DEV)
    H.gather_rows(x, y, index, ox, oy, cursor=cursor)         # module load outside the capture
    H.epoch_step_end(loss, mean, cursor)
    torch.cuda.synchronize()
    cursor.zero_()
    mean.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        H.gather_rows(x, y, index, ox, oy, cursor=cursor)
        H.epoch_step_end(loss, mean, cursor)
    losses = [0.7310586, 3.1415927, 0.1234567]
    ref = 0.0
    for i, value in enumerate(losses):
        loss.fill_(value)
        graph.replay()
        assert torch.equal(ox, x[index[4 * i:4 * i + 4]]) and torch.equal(oy, y[index[4 * i:4 * i + 4]]), i
        ref = ref + (torch.tensor(value, dtype=torch.float32) - ref) / (i + 1)       # as train.main writes it
    assert int(cursor) == 3
    assert ref.dtype == torch.float32 and torch.equal(mean.cpu().reshape(()), ref)


def test_resident_loader_yields_the_dataloaders_batches():
    """ResidentLoader against DataLoader(TensorDataset(x, y), 2, shuffle=True) from the same seed, n = 5, two epochs:
    every batch bit-equal, the partial one included, through the cursor path (fetch + step_end) and as an iterator; the
    default generator ends in the same state."""
    T = pkg().train
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(5, 3, 4, 6, generator=g), torch.randn(5, 2, 7, generator=g)
    torch.manual_seed(21)
    ref_loader = DataLoader(TensorDataset(x, y), 2, shuffle=True)
    ref = [[(bx.clone(), by.clone()) for bx, by in ref_loader] for _ in range(2)]
    ref_state = torch.get_rng_state()
    assert [len(e) for e in ref] == [3, 3] and ref[0][2][0].shape[0] == 1
    loss = torch.ones((), device=DEV)

    torch.manual_seed(21)
    loader = T.ResidentLoader(x.to(DEV), y, 2, True)
    assert len(loader) == 3 and loader.target.device == loader.x.device and tuple(loader.x.shape) == (2, 3, 4, 6)
    for epoch in range(2):
        loader.begin_epoch()
        for i, (_, count, graphable) in enumerate(loader.plan):
            bx, by = loader.fetch(count)
            assert graphable == (count == 2)
            assert torch.equal(bx.cpu(), ref[epoch][i][0]) and torch.equal(by.cpu(), ref[epoch][i][1]), (epoch, i)
            loader.step_end(loss)
        assert int(loader.cursor) == 3 and float(loader.mean) == 1.0
    assert torch.equal(torch.get_rng_state(), ref_state)

    torch.manual_seed(21)
    loader = T.ResidentLoader(x.to(DEV), y.to(DEV), 2, True)
    for epoch in range(2):
        got = [(bx.cpu(), by.cpu()) for bx, by in loader]
        assert len(got) == 3
        for (bx, by), (rx, ry) in zip(got, ref[epoch]):
            assert torch.equal(bx, rx) and torch.equal(by, ry)

    # not shuffled: the array's own order, and the same single draw per epoch as the DataLoader's iterator
    torch.manual_seed(21)
    plain = [bx for bx, _ in DataLoader(TensorDataset(x, y), 2, shuffle=False)]
    ref_state = torch.get_rng_state()
    torch.manual_seed(21)
    got = [bx.cpu() for bx, _ in T.ResidentLoader(x.to(DEV), y, 2, False)]
    assert all(torch.equal(a, b) for a, b in zip(got, plain)) and len(got) == len(plain)
    assert torch.equal(torch.get_rng_state(), ref_state)
