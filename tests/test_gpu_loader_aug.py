"""hip_ops.gather_rows_aug (csrc/loader.hip) and train.ResidentLoader(augment=...) against the numpy restatement of
include/seld_hip.h in tests/loader_aug_ref.py.  Every comparison is torch.equal: the kernel moves data, flips signs and
adds one fp32 constant."""
import functools

import numpy as np
import pytest
import torch

from tests import loader_aug_ref as R
from tests.helpers import build_model, pkg
from tests.loader_helpers import DEV, SENTINEL, buffers, epoch as _epoch

pytestmark = pytest.mark.gpu
N_ROWS, B = 7, 5
SHAPES = [(4, 5, 8),            # a row smaller than one tile
          (8, 6, 516),          # 16-byte path, F * T = 3096: tiles straddle channels
          (4, 3, 7),            # scalar path, every other row misaligned
          (16, 4, 1024)]        # several tiles per channel
TARGETS = [(3, 2), (5, 42)]     # (T_out, n_sed)
PRESET = {4: dict(), 8: dict(mics=2), 16: dict(mics=2, phase=True)}


@functools.lru_cache(maxsize=None)
def _data(shape, target):
    rng = np.random.default_rng(sum(shape) + target[1])
    x = rng.standard_normal((N_ROWS,) + shape).astype(np.float32)
    x[:, :, 0, 0] = 0.0                                     # flip 2 at its tie, and signed zeros
    y = rng.standard_normal((N_ROWS, target[0], 4 * target[1])).astype(np.float32)
    return x, y, torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)


def _hand_table(C):
    """Two transforms with flips 1 and 2 and another source on every channel."""
    rows = []
    for shift, flips, axis, sign in ((1, (1, 2), [2, 0, 1], [-1, 1, -1]), (C - 1, (2, 1), [1, 2, 0], [1, -1, -1])):
        rows.append([(c + shift) % C for c in range(C)] + [flips[c % 2] for c in range(C)] + axis + sign)
    return np.asarray(rows, dtype=np.int32)


def _table(kind, C):
    if kind == "preset":
        return pkg().hip_ops.foa_transforms(**PRESET[C])
    return _hand_table(C) if kind == "hand" else None


def _buffers(shape, target):
    return buffers(shape, (target[0], 4 * target[1]), B)


def _check(shape, target, index, first, count, aug_kw, table, *, seed=3, epoch=0, via_cursor=False):
    """One call against the reference; returns the two device buffers."""
    H = pkg().hip_ops
    x, y, xd, yd = _data(shape, target)
    aug = H.Augment(table=table, device=DEV, **aug_kw)
    ox, oy = _buffers(shape, target)
    idx = torch.as_tensor(index, dtype=torch.int64).to(DEV)
    if via_cursor:
        stride = 3
        cursor = torch.tensor([first // stride], device=DEV, dtype=torch.int32)
        H.gather_rows_aug(xd, yd, idx, ox, oy, epoch=_epoch(epoch), seed=seed, augment=aug, cursor=cursor, stride=stride,
                          start=first % stride, count=count)
    else:
        H.gather_rows_aug(xd, yd, idx, ox, oy, epoch=_epoch(epoch), seed=seed, augment=aug, start=first, count=count)
    init_x, init_y = np.full((B,) + shape, SENTINEL, np.float32), np.full((B, target[0], 4 * target[1]), SENTINEL, np.float32)
    want_x, want_y = R.gather_aug(x, y, np.asarray(index), first, count, init_x, init_y, seed=seed, epoch=epoch, table=table,
                                  p_swap=aug_kw.get("p_swap", 0.0), n_fmask=aug_kw.get("freq_masks", 0),
                                  f_max=aug_kw.get("freq_width", 0), n_tmask=aug_kw.get("time_masks", 0),
                                  t_max=aug_kw.get("time_width", 0), fill=aug_kw.get("fill", 0.0))
    assert torch.equal(ox.cpu(), torch.from_numpy(want_x)), (shape, target, first, count)
    assert torch.equal(oy.cpu(), torch.from_numpy(want_y)), (shape, target, first, count)
    return ox, oy


INDEX = [3, 6, 0, 3, 2, 5, 1, 4, 6, 0, 2, 2]


@pytest.mark.parametrize("mode", ["swap_preset", "swap_hand", "masks", "both_hand", "both_preset_half"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_rows_aug_equals_the_reference(shape, mode):
    """The four shapes x {the 16-row preset at p_swap = 1, a hand-made table with flips 1 and 2 and a moved source on every
    channel, masks only (two of each, widths up to the whole axis, fill != 0), both together, both with p_swap = 0.5},
    with count 1 and 5, both target geometries, `start` and the cursor form; rows >= count keep the sentinel."""
    C, F, T = shape
    masks = dict(freq_masks=2, freq_width=F, time_masks=2, time_width=T, fill=0.25)
    aug_kw, kind = {
        "swap_preset": (dict(p_swap=1.0), "preset"), "swap_hand": (dict(p_swap=1.0), "hand"), "masks": (masks, None),
        "both_hand": (dict(masks, p_swap=1.0), "hand"), "both_preset_half": (dict(masks, p_swap=0.5), "preset")}[mode]
    table = _table(kind, C)
    for i, (count, first) in enumerate(((1, 6), (5, 3))):
        _check(shape, TARGETS[i % 2], INDEX, first, count, aug_kw, table, via_cursor=bool(i))
        _check(shape, TARGETS[(i + 1) % 2], INDEX, first, count, aug_kw, table, epoch=1, via_cursor=not i)


@pytest.mark.parametrize("shape", SHAPES)
def test_no_table_and_no_masks_is_the_plain_gather(shape):
    H = pkg().hip_ops
    _, _, xd, yd = _data(shape, TARGETS[1])
    idx = torch.tensor(INDEX, device=DEV)
    for count in (1, 5):
        ox, oy = _buffers(shape, TARGETS[1])
        px, py = _buffers(shape, TARGETS[1])
        H.gather_rows_aug(xd, yd, idx, ox, oy, epoch=_epoch(4), seed=9, augment=H.Augment(device=DEV), start=2, count=count)
        H.gather_rows(xd, yd, idx, px, py, start=2, count=count)
        assert torch.equal(ox, px) and torch.equal(oy, py)
        # masks of width 0 and a table that is never drawn change nothing either
        idle = H.Augment(table=_hand_table(shape[0]), p_swap=0.0, freq_masks=2, freq_width=0, time_masks=1, time_width=0,
                         fill=9.0, device=DEV)
        ox, oy = _buffers(shape, TARGETS[1])
        H.gather_rows_aug(xd, yd, idx, ox, oy, epoch=_epoch(4), seed=9, augment=idle, start=2, count=count)
        assert torch.equal(ox, px) and torch.equal(oy, py)


def test_mask_edges_whole_axis_empty_and_overlapping():
    """Positions chosen from the REFERENCE's draws over 4096 positions of (4, 5, 8) rows: a frequency mask over all of F, a
    time mask over all of T, a mask of width 0 beside one that is not, two overlapping frequency masks, two overlapping time
    masks.  Each is gathered alone with fill = -3.5 and compared; the whole-axis ones leave nothing but the fill."""
    shape, target = SHAPES[0], TARGETS[0]
    C, F, T = shape
    index = [p % N_ROWS for p in range(4096)]
    aug_kw = dict(freq_masks=2, freq_width=F, time_masks=2, time_width=T, fill=-3.5)
    found = {}
    for p in range(4096):
        d = R.draws(3, 0, p, 0, 0.0, 2, F, F, 2, T, T)
        (f0, fw0), (f1, fw1) = d["fmasks"]
        (t0, tw0), (t1, tw1) = d["tmasks"]
        if F in (fw0, fw1):
            found.setdefault("all_f", p)
        if T in (tw0, tw1):
            found.setdefault("all_t", p)
        if (fw0 == 0) != (fw1 == 0) and tw0 and tw1:
            found.setdefault("empty_f", p)
        if fw0 and fw1 and max(f0, f1) < min(f0 + fw0, f1 + fw1) and (f0, fw0) != (f1, fw1):
            found.setdefault("overlap_f", p)
        if tw0 and tw1 and max(t0, t1) < min(t0 + tw0, t1 + tw1) and (t0, tw0) != (t1, tw1):
            found.setdefault("overlap_t", p)
    assert set(found) == {"all_f", "all_t", "empty_f", "overlap_f", "overlap_t"}
    for what, p in found.items():
        ox, _ = _check(shape, target, index, p, 1, aug_kw, None)
        if what in ("all_f", "all_t"):
            assert bool((ox[0] == -3.5).all())
        assert bool((ox[1:] == SENTINEL).all())


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[1]])
def test_rows_of_invalid_indices_stay_zero_and_unaugmented(shape):
    """Indices -1 and n_rows and positions past the end of `index`: zeros as from gather_rows, no fill value, no flip-2
    constant; their neighbours are augmented."""
    C, F, T = shape
    aug_kw = dict(p_swap=1.0, freq_masks=2, freq_width=F, time_masks=2, time_width=T, fill=0.75)
    index = [3, -1, 6, N_ROWS, 0, 2, 5]
    ox, oy = _check(shape, TARGETS[0], index, 0, 5, aug_kw, _hand_table(C))
    assert not ox[1].any() and not ox[3].any() and not oy[1].any() and not oy[3].any() and bool(ox[0].any())
    ox, oy = _check(shape, TARGETS[0], index, 5, 5, aug_kw, _hand_table(C))
    assert not ox[2:].any() and not oy[2:].any()
    _check(shape, TARGETS[0], index, -1, 2, aug_kw, _hand_table(C))


def test_draws_follow_the_position_not_the_form_of_the_call():
    """(epoch, p) fixes the bits: through `start`, through cursor * stride + start, and inside batches of another size."""
    H = pkg().hip_ops
    shape, target = SHAPES[1], TARGETS[1]
    _, _, xd, yd = _data(shape, target)
    aug = H.Augment(table=_table("preset", 8), p_swap=0.7, freq_masks=1, freq_width=4, time_masks=2, time_width=100, device=DEV)
    idx = torch.tensor(INDEX, device=DEV)
    ax, ay = _buffers(shape, target)
    H.gather_rows_aug(xd, yd, idx, ax, ay, epoch=_epoch(2), seed=11, augment=aug, start=4)
    bx, by = _buffers(shape, target)
    H.gather_rows_aug(xd, yd, idx, bx, by, epoch=_epoch(2), seed=11, augment=aug, cursor=torch.tensor([2], device=DEV, dtype=torch.int32),
                      stride=1, start=2)
    assert torch.equal(ax, bx) and torch.equal(ay, by)
    cx, cy = torch.zeros((2,) + shape, device=DEV), torch.zeros((2, target[0], 4 * target[1]), device=DEV)
    H.gather_rows_aug(xd, yd, idx, cx, cy, epoch=_epoch(2), seed=11, augment=aug, start=6)
    assert torch.equal(cx, ax[2:4]) and torch.equal(cy, ay[2:4])
    H.gather_rows_aug(xd, yd, idx, bx, by, epoch=_epoch(3), seed=11, augment=aug, start=4)
    assert not torch.equal(ax, bx)                               # another epoch: other draws (checked against the reference below)


def _loader_reference(x, y, epoch, first, count, aug_kw, table, seed):
    zx, zy = np.zeros((count,) + x.shape[1:], np.float32), np.zeros((count,) + y.shape[1:], np.float32)
    return R.gather_aug(x, y, np.arange(x.shape[0]), first, count, zx, zy, seed=seed, epoch=epoch, table=table,
                        p_swap=aug_kw["p_swap"], n_fmask=aug_kw["freq_masks"], f_max=aug_kw["freq_width"],
                        n_tmask=aug_kw["time_masks"], t_max=aug_kw["time_width"], fill=aug_kw["fill"])


LOADER_AUG = dict(p_swap=0.6, freq_masks=1, freq_width=3, time_masks=2, time_width=5, fill=0.5)


def _loader_data():
    rng = np.random.default_rng(17)
    return rng.standard_normal((8, 4, 5, 8)).astype(np.float32), rng.standard_normal((8, 3, 8)).astype(np.float32)


def test_two_ranks_together_fetch_the_single_process_batch_and_epochs_differ():
    """world = 2, shuffle=False (no process group): rank 0's and rank 1's halves, concatenated, are the world = 1 batch, in
    epoch 0 and epoch 1, through the cursor and through batch=; both equal the reference and the epochs differ."""
    H, T = pkg().hip_ops, pkg().train
    x, y = _loader_data()
    table = H.foa_transforms()
    aug = H.Augment(table=table, device=DEV, **LOADER_AUG)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    one = T.ResidentLoader(xd, yd, 4, False, augment=aug, seed=21)
    ranks = [T.ResidentLoader(xd, yd, 4, False, r, 2, augment=aug, seed=21) for r in range(2)]
    assert int(one.epoch) == -1
    loss = torch.ones((), device=DEV)
    seen = []
    for epoch in range(2):
        for ld in [one] + ranks:
            ld.begin_epoch()
            assert int(ld.epoch) == epoch and int(ld.cursor) == 0
        for i in range(2):
            for ld in [one] + ranks:
                ld.fetch()
            want_x, want_y = _loader_reference(x, y, epoch, 4 * i, 4, LOADER_AUG, table, 21)
            assert torch.equal(one.x.cpu(), torch.from_numpy(want_x)) and torch.equal(one.target.cpu(), torch.from_numpy(want_y))
            assert torch.equal(torch.cat([ranks[0].x, ranks[1].x]), one.x)
            assert torch.equal(torch.cat([ranks[0].target, ranks[1].target]), one.target)
            seen.append(one.x.clone())
            for ld in [one] + ranks:
                ld.step_end(loss)
        got = [ld.fetch(batch=1)[0].clone() for ld in [one] + ranks]
        assert torch.equal(got[0], seen[-1]) and torch.equal(torch.cat(got[1:]), seen[-1])
    assert not torch.equal(seen[0], seen[2]) and not torch.equal(seen[1], seen[3])


def test_transform_indices_over_4096_positions_are_the_references():
    """One target row [1 | 1 2 3] (n_sed = 1) gathered at 4096 positions with the 16-row preset at p_swap = 1: the transformed
    location names the transform, the indices equal int(w[0], 16) of the reference word for word, and all 16 occur."""
    H = pkg().hip_ops
    table = H.foa_transforms()
    y = torch.tensor([[[1.0, 1.0, 2.0, 3.0]]], device=DEV)
    out = torch.zeros(4096, 1, 4, device=DEV)
    H.gather_rows_aug(None, y, torch.zeros(4096, dtype=torch.int64, device=DEV), None, out, epoch=_epoch(5), seed=77,
                      augment=H.Augment(table=table, p_swap=1.0, device=DEV))
    out = out.cpu().numpy().reshape(4096, 4)
    assert (out[:, 0] == 1).all()
    by_location = {tuple(float(table[k, 11 + a]) * (1.0, 2.0, 3.0)[table[k, 8 + a]] for a in range(3)): k for k in range(16)}
    assert len(by_location) == 16
    got = np.array([by_location[tuple(r)] for r in out[:, 1:].tolist()])
    counters = (np.uint64(5) << np.uint64(34)) | (np.arange(4096, dtype=np.uint64) << np.uint64(2))
    w = R.P.philox4x32_10(counters, np.uint64(77))
    assert (R.P.u01(w[:, 1]) < np.float32(1.0)).all()
    want = ((w[:, 0].astype(np.uint64) * np.uint64(16)) >> np.uint64(32)).astype(np.int64)
    assert np.array_equal(got, want)
    assert set(got.tolist()) == set(range(16))
    assert want[7] == R.draws(77, 5, 7, 16, 1.0, 0, 0, 1, 0, 0, 1)["k"]


def test_recorded_fetch_draws_anew_at_every_replay_and_epoch():
    """fetch() + step_end recorded in ONE graph (no parallel branch), replayed through two epochs with begin_epoch in
    between: every replayed batch is the reference's for its (epoch, position)."""
    H, T = pkg().hip_ops, pkg().train
    x, y = _loader_data()
    table = H.foa_transforms()
    loader = T.ResidentLoader(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), 4, False,
                              augment=H.Augment(table=table, device=DEV, **LOADER_AUG), seed=4)
    loss = torch.ones((), device=DEV)
    loader.fetch()                                              # module load outside the capture
    loader.step_end(loss)
    torch.cuda.synchronize()
    loader.cursor.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loader.fetch()
        loader.step_end(loss)
    assert int(loader.epoch) == -1 and int(loader.cursor) == 0  # recording ran nothing
    for epoch in range(2):
        loader.begin_epoch()
        for i in range(2):
            graph.replay()
            want_x, want_y = _loader_reference(x, y, epoch, 4 * i, 4, LOADER_AUG, table, 4)
            assert torch.equal(loader.x.cpu(), torch.from_numpy(want_x)), (epoch, i)
            assert torch.equal(loader.target.cpu(), torch.from_numpy(want_y)), (epoch, i)
        assert int(loader.cursor) == 2 and int(loader.epoch) == epoch


def test_bad_arguments_are_refused():
    H, L = pkg().hip_ops, pkg()._lib
    shape, target = SHAPES[0], TARGETS[0]
    C, F, T = shape
    _, _, xd, yd = _data(shape, target)
    ox, oy = _buffers(shape, target)
    idx = torch.arange(N_ROWS, device=DEV)
    ep = _epoch(0)
    table = torch.from_numpy(H.foa_transforms()).to(DEV)
    lib, s = L.lib(), L.current_stream()
    good = dict(x_all=L.ptr(xd), row_x=C * F * T, out_x=L.ptr(ox), y_all=L.ptr(yd), row_y=3 * 8, out_y=L.ptr(oy), index=L.ptr(idx),
                n_index=N_ROWS, n_rows=N_ROWS, cursor=None, stride=B, start=0, B=B, count=B, C=C, F=F, T=T, y_cols=8, epoch=L.ptr(ep),
                seed=1, table=L.ptr(table), K=16, p_swap=0.5, n_fmask=1, f_max=F, n_tmask=1, t_max=T, fill=0.0)
    bad = [dict(epoch=None), dict(K=65), dict(K=-1), dict(K=0), dict(table=None), dict(C=17, row_x=17 * F * T), dict(C=0),
           dict(F=0), dict(T=-1), dict(row_x=C * F * T + 4), dict(y_cols=6), dict(y_cols=0), dict(y_cols=16), dict(p_swap=1.5),
           dict(p_swap=-0.5), dict(p_swap=float("nan")), dict(n_fmask=3), dict(n_fmask=-1), dict(n_tmask=3), dict(f_max=F + 1),
           dict(f_max=-1), dict(t_max=T + 1), dict(t_max=-1), dict(n_index=2 ** 32 + 1), dict(count=B + 1), dict(count=0),
           dict(index=None), dict(out_x=None)]
    for change in bad:
        args = dict(good, **change)
        assert lib.seld_gather_rows_aug(*args.values(), s) == -1, change
    torch.cuda.synchronize()
    assert bool((ox == SENTINEL).all()) and bool((oy == SENTINEL).all())        # nothing was launched
    assert lib.seld_gather_rows_aug(*good.values(), s) == 0
    aug = H.Augment(table=H.foa_transforms(), p_swap=0.5, device=DEV)
    with pytest.raises(L.SeldHipError):
        H.gather_rows_aug(xd, yd, idx, ox, oy, epoch=ep, seed=1, augment=None)
    with pytest.raises(L.SeldHipError):
        H.gather_rows_aug(xd, yd, idx, ox, oy, epoch=ep.to(torch.int64), seed=1, augment=aug)
    with pytest.raises(L.SeldHipError):                                         # an 8-channel table on 4-channel predictors
        H.gather_rows_aug(xd, yd, idx, ox, oy, epoch=ep, seed=1, augment=H.Augment(table=H.foa_transforms(mics=2), device=DEV))
    with pytest.raises(L.SeldHipError, match="SELD_EINVAL"):                    # a mask wider than the axis
        H.gather_rows_aug(xd, yd, idx, ox, oy, epoch=ep, seed=1, augment=H.Augment(freq_masks=1, freq_width=F + 1, device=DEV))
    with pytest.raises(L.SeldHipError):
        H.gather_rows_aug(xd.reshape(N_ROWS, -1), yd, idx, ox.reshape(B, -1), oy, epoch=ep, seed=1, augment=aug)
    with pytest.raises(L.SeldHipError):
        H.Augment(table=np.zeros((2, 14), dtype=np.int32), device=DEV)          # axis is no permutation


def test_resident_loader_launches_the_plain_gather_unless_augment_is_given():
    H, T = pkg().hip_ops, pkg().train
    x, y = _loader_data()
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    plain = T.ResidentLoader(xd, yd, 4, False)
    augmented = T.ResidentLoader(xd, yd, 4, False, augment=H.Augment(freq_masks=1, freq_width=2, device=DEV))
    timer = H.kernel_timer
    was = timer.active, timer.only
    try:
        timer.active, timer.only = True, None
        for loader, label in ((plain, "gather_rows_kernel"), (augmented, "gather_rows_aug_kernel")):
            timer.reset()
            loader.begin_epoch()
            loader.fetch()
            loader.fetch(3, batch=1)
            torch.cuda.synchronize()
            assert [r[0] for r in timer.records] == [label, label]
    finally:
        timer.active, timer.only = was
        timer.reset()
    assert torch.equal(plain.x[:3], xd[4:7]) and torch.equal(plain.target[:3], yd[4:7])


def test_graphed_train_step_trains_on_augmented_batches():
    """GraphedTrainStep(loader=...) on the tiny DQ model with swap and masks on: three replays walk through the epoch, the loss
    is finite and the recorded input buffer holds the reference's batch after each."""
    from tests.golden.cases import MODEL_CASES
    H, T = pkg().hip_ops, pkg().train
    case = next(c for c in MODEL_CASES if c["name"] == "tiny_DQ")
    shape = (case["input_channels"], case["freq_dim"], case["time_dim"])
    rng = np.random.default_rng(23)
    x = rng.standard_normal((6,) + shape).astype(np.float32)
    y = np.concatenate([(rng.random((6, 8, 42)) < 0.1).astype(np.float32), rng.uniform(-1, 1, (6, 8, 126)).astype(np.float32)], 2)
    aug_kw = dict(p_swap=0.8, freq_masks=2, freq_width=16, time_masks=1, time_width=10, fill=0.0)
    table = H.foa_transforms(mics=2)
    loader = T.ResidentLoader(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), 2, False,
                              augment=H.Augment(table=table, device=DEV, **aug_kw), seed=6)
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    model = build_model(case).to(DEV).train()
    opt = T.FlatAdam(model.parameters(), lr=1e-3)
    snap = T.training_snapshot(model, opt)
    loader.fetch(batch=0)
    runner = T.GraphedTrainStep(model, opt, loader.x, loader.target, 42, 1.0, 5.0, warmup=1, loader=loader)
    T.training_restore(model, opt, snap)
    assert int(loader.epoch) == -1 and int(loader.cursor) == 0       # warm-up and recording moved neither
    loader.begin_epoch()
    for i in range(3):
        loss = runner()
        assert bool(torch.isfinite(loss).all())
        want_x, want_y = _loader_reference(x, y, 0, 2 * i, 2, aug_kw, table, 6)
        assert torch.equal(loader.x.cpu(), torch.from_numpy(want_x)), i
        assert torch.equal(loader.target.cpu(), torch.from_numpy(want_y)), i
    assert int(loader.cursor) == 3 and bool(torch.isfinite(loader.mean).all())
