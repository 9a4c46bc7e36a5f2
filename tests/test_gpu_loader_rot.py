"""hip_ops.gather_rows_rot (csrc/loader.hip, seld_gather_rows_rot), train.ResidentLoader with a rotating Augment and the
intensity-layout tables of hip_ops.foa_transforms on the existing kernels, against the numpy restatement of
include/seld_hip.h in tests/loader_rot_ref.py.

Bounds.  A rotated element is fma(R2, z, fma(R1, y, R0 * x)) or the same without contraction: three products and two
additions, each rounded to half an ulp (2^-24 relative), all of magnitude at most S = sum_j |R[a][j]| |v_j| up to second
order: explicit matrices are held to 4 * 2^-24 * S plus the smallest normal float (denormal results may be flushed).
Drawn rotations add the error of sincospif on the entries of R, documented as 2 ulp: |R| <= 1, so 2 * 2^-23 * sum_j |v_j|
more; they are held to 8 * 2^-24 * sum_j |v_j|.  Everything else the kernel moves is compared as bits."""
import functools

import numpy as np
import pytest
import torch

from tests import loader_aug_ref as A
from tests import loader_rot_ref as R
from tests.helpers import build_model, pkg
from tests.loader_helpers import DEV, SENTINEL, bits as _bits, buffers, epoch as _epoch, hold_rot as _hold, shifted

pytestmark = pytest.mark.gpu
N_ROWS, B = 5, 4
U24, TINY = R.U24, R.TINY
IV5 = [(3 * g, 3 * g + 2, 3 * g + 1) for g in range(5)]           # five groups [I1, I2, I3] of the order W X Z Y
# (C, F, T), triples, floats by which the resident predictors are shifted off 16-byte alignment
CASES = {
    "scalar_4x3x5": ((4, 3, 5), [(3, 1, 2)], 0),                    # quaternion, 1 microphone; T % 4 != 0
    "vector_8x8x64": ((8, 8, 64), [(3, 1, 2), (7, 5, 6)], 0),       # quaternion, 2 microphones; 16-byte path, 128 items per channel
    "five_triples_15x2x12": ((15, 2, 12), IV5, 0),                  # the most triples, no channel passes
    "misaligned_8x8x64": ((8, 8, 64), [(3, 1, 2), (7, 5, 6)], 1),   # T % 4 == 0 but the scalar path
}
TARGETS = [(7, 3), (5, 42)]                                         # (T_out, n_sed)
INDEX = [3, -1, 0, 4, 2, N_ROWS, 1, 1, 3]


@functools.lru_cache(maxsize=None)
def _data(name, target):
    shape, _, shift = CASES[name]
    rng = np.random.default_rng(sum(shape) + target[1])
    x = rng.standard_normal((N_ROWS,) + shape).astype(np.float32)
    x[:, :, 0, 0] = -0.0                                            # a signed zero must pass as it is
    y = rng.standard_normal((N_ROWS, target[0], 4 * target[1])).astype(np.float32)
    n_sed = target[1]
    y[:, 0, n_sed:n_sed + 6] = [1.0, 0.25, 0.5, -0.5, 1.0, 0.75]    # slots 0 and 1 of frame 0: they name the rotation (test 3)
    xd, yd = shifted(x, shift), torch.from_numpy(y).to(DEV)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, xd, yd


def _buffers(shape, target, rows=B):
    return buffers(shape, (target[0], 4 * target[1]), rows)


def _call(name, target, first, count, aug_kw, *, matrices=None, seed=3, epoch=0, index=INDEX, rows=B, via_cursor=False):
    """One call of gather_rows_rot and the reference of the same call: (out_x, out_y, reference)."""
    H = pkg().hip_ops
    shape, triples, _ = CASES[name]
    x, y, xd, yd = _data(name, target)
    aug = H.Augment(rot_triples=triples, device=DEV, **aug_kw)
    ox, oy = _buffers(shape, target, rows)
    idx = torch.as_tensor(index, dtype=torch.int64).to(DEV)
    md = None if matrices is None else torch.from_numpy(np.ascontiguousarray(matrices, dtype=np.float32)).to(DEV)
    kw = dict(epoch=_epoch(epoch), seed=seed, augment=aug, matrices=md, count=count)
    if via_cursor:
        stride = 3
        H.gather_rows_rot(xd, yd, idx, ox, oy, cursor=torch.tensor([first // stride], device=DEV, dtype=torch.int32), stride=stride,
                          start=first % stride, **kw)
    else:
        H.gather_rows_rot(xd, yd, idx, ox, oy, start=first, **kw)
    ref = R.gather_rot(x, y, np.asarray(index), first, count, np.full((rows,) + shape, SENTINEL, np.float32),
                       np.full((rows, target[0], 4 * target[1]), SENTINEL, np.float32), seed=seed, epoch=epoch, triples=triples,
                       p_rot=aug_kw.get("p_rot", 0.0), rot_mirror=aug_kw.get("rot_mirror", True), rot_zflip=aug_kw.get("rot_zflip", True),
                       matrices=matrices, n_fmask=aug_kw.get("freq_masks", 0), f_max=aug_kw.get("freq_width", 0),
                       n_tmask=aug_kw.get("time_masks", 0), t_max=aug_kw.get("time_width", 0), fill=aug_kw.get("fill", 0.0))
    return ox, oy, ref


def _orthogonal(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_explicit_matrices_within_the_rounding_of_three_products(name):
    """Random orthogonal matrices and one that is not, p_rot = 0 (the matrix decides), both target geometries, through
    `start` and through the cursor, count below B with invalid rows in between, the last call with masks over the rotated
    values: rotated elements within 4 * 2^-24 * S, everything else (channels outside the triples, activity, masked
    elements, rows >= count, zero rows) as bits."""
    rng = np.random.default_rng(len(name))
    mats = np.stack([_orthogonal(rng), rng.uniform(-2, 2, (3, 3)), _orthogonal(rng), _orthogonal(rng)]).reshape(4, 9).astype(np.float32)
    for i, (first, count) in enumerate(((0, 3), (2, 4), (6, 4))):
        masks = dict(freq_masks=1, freq_width=2, time_masks=2, time_width=3, fill=0.25) if i == 2 else {}     # masks over rotated values
        ox, oy, ref = _call(name, TARGETS[i % 2], first, count, masks, matrices=mats[:count], via_cursor=i == 1)
        _hold(ox, ref["x"], 4, "weight", (name, "x", first))
        _hold(oy, ref["y"], 4, "weight", (name, "y", first))
        invalid = [b for b, d in enumerate(ref["rows"]) if d is None]
        assert invalid and all(not ox[b].any() and not oy[b].any() for b in invalid)
        assert bool((ox[count:] == SENTINEL).all()) and bool((oy[count:] == SENTINEL).all())
        assert not ref["x"]["exact"][1:count].all() and not ref["y"]["exact"][0].all()   # something was rotated and left unmasked


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scalar_4x3x5", "vector_8x8x64"])
def test_signed_permutation_matrices_equal_the_table_rows_of_gather_rows_aug(name):
    """Every row k of foa_transforms(layout='quaternion') as an explicit matrix M[a][axis[a]] = sign[a] against
    gather_rows_aug with that one row at p_swap = 1: products with 0 and +-1 are exact, so the outputs compare == (a zero
    of either sign equals a zero), predictors and targets."""
    H = pkg().hip_ops
    shape, triples, _ = CASES[name]
    C = shape[0]
    table = H.foa_transforms(mics=C // 4, layout="quaternion")
    assert [tuple(t) for t in triples] == H.foa_triples(mics=C // 4, layout="quaternion")
    _, _, xd, yd = _data(name, TARGETS[1])
    idx = torch.tensor([4, 0, 2, 3], device=DEV)
    rot = H.Augment(rot_triples=triples, device=DEV)
    for k, row in enumerate(table):
        M = np.zeros((3, 3), dtype=np.float32)
        for a in range(3):
            M[a, row[2 * C + a]] = row[2 * C + 3 + a]
        mats = torch.from_numpy(np.tile(M.reshape(1, 9), (B, 1))).to(DEV)
        rx, ry = _buffers(shape, TARGETS[1])
        H.gather_rows_rot(xd, yd, idx, rx, ry, epoch=_epoch(0), seed=1, augment=rot, matrices=mats)
        ax, ay = _buffers(shape, TARGETS[1])
        H.gather_rows_aug(xd, yd, idx, ax, ay, epoch=_epoch(0), seed=1, augment=H.Augment(table=table[k:k + 1], p_swap=1.0, device=DEV))
        assert bool((rx == ax).all()) and bool((ry == ay).all()), k
        if k == 0:
            assert bool((rx == xd[idx]).all())                  # the identity matrix still multiplies: a -0 may come out as +0


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def _named_rotation(src_y, out_y, n_sed):
    """(rotated, mirror, zflip) read off a target row: rotated iff the bits moved; slots 0 and 1 of frame 0 hold two fixed
    vectors whose xy determinant changes sign under a mirror and whose z changes sign under a z-flip."""
    if R.bits_equal(out_y, src_y.astype(np.float64)).all():
        return False, None, None
    v, o = src_y[0, n_sed:n_sed + 6].astype(np.float64), out_y[0, n_sed:n_sed + 6].astype(np.float64)
    det = lambda w: w[0] * w[4] - w[1] * w[3]
    return True, bool(det(o) * det(v) < 0), bool(o[2] * v[2] < 0)


@pytest.mark.parametrize("name", ["scalar_4x3x5", "vector_8x8x64"])
def test_drawn_rotations_over_64_positions_and_two_epochs(name):
    """p_rot = 0.5 with mirror and z-flip on: which samples rotate and their two bits equal the reference's draws exactly,
    elements are within 8 * 2^-24 * sum_j |v_j|, unrotated samples are copies bit for bit; the two epochs differ."""
    target = TARGETS[0]
    index = [p % N_ROWS for p in range(64)]
    _, y, _, _ = _data(name, target)
    seen = []
    for epoch in (0, 1):
        ox, oy, ref = _call(name, target, 0, 64, dict(p_rot=0.5), seed=9, epoch=epoch, index=index, rows=64)
        got_y = oy.cpu().numpy()
        named = [_named_rotation(y[index[b]], got_y[b], target[1]) for b in range(64)]
        want = [(d["rotate"], d["mirror"] if d["rotate"] else None, d["zflip"] if d["rotate"] else None) for d in ref["rows"]]
        assert named == want, epoch
        assert 16 < sum(r for r, _, _ in named) < 48
        _hold(ox, ref["x"], 8, "plain", (name, "x", epoch))
        _hold(oy, ref["y"], 8, "plain", (name, "y", epoch))
        for b, d in enumerate(ref["rows"]):
            if not d["rotate"]:
                assert ref["x"]["exact"][b].all() and ref["y"]["exact"][b].all()
        seen.append([w[0] for w in want])
    assert seen[0] != seen[1]
    # the switches: without them no sample is mirrored or flipped
    _, oy, ref = _call(name, target, 0, 64, dict(p_rot=1.0, rot_mirror=False, rot_zflip=False), seed=9, index=index, rows=64)
    named = [_named_rotation(y[index[b]], oy[b].cpu().numpy(), target[1]) for b in range(64)]
    assert all(n == (True, False, False) for n in named)
    _hold(oy, ref["y"], 8, "plain", (name, "y", "no flips"))


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_without_rotation_it_is_the_masks_only_gather(name):
    H = pkg().hip_ops
    shape, triples, _ = CASES[name]
    C, F, T = shape
    _, _, xd, yd = _data(name, TARGETS[1])
    idx = torch.tensor(INDEX, device=DEV)
    masks = dict(freq_masks=2, freq_width=F, time_masks=2, time_width=T, fill=0.25)
    for count, start in ((1, 6), (4, 2)):
        for epoch in (0, 3):
            rx, ry = _buffers(shape, TARGETS[1])
            H.gather_rows_rot(xd, yd, idx, rx, ry, epoch=_epoch(epoch), seed=5, start=start, count=count,
                              augment=H.Augment(rot_triples=triples, p_rot=0.0, device=DEV, **masks))
            ax, ay = _buffers(shape, TARGETS[1])
            H.gather_rows_aug(xd, yd, idx, ax, ay, epoch=_epoch(epoch), seed=5, start=start, count=count,
                              augment=H.Augment(device=DEV, **masks))
            assert torch.equal(_bits(rx), _bits(ax)) and torch.equal(_bits(ry), _bits(ay)), (count, epoch)
    # nothing to apply at all: the plain gather
    rx, ry = _buffers(shape, TARGETS[1])
    H.gather_rows_rot(xd, yd, idx, rx, ry, epoch=_epoch(0), seed=5, augment=H.Augment(rot_triples=triples, device=DEV))
    px, py = _buffers(shape, TARGETS[1])
    H.gather_rows(xd, yd, idx, px, py)
    assert torch.equal(_bits(rx), _bits(px)) and torch.equal(_bits(ry), _bits(py))


def test_mask_edges_on_rotated_samples_write_the_fill_exactly():
    """Positions chosen from the reference's draws over 4096 positions of (4, 3, 5) rows: a frequency mask over all of F, a
    time mask over all of T, a mask of width 0 beside one that is not, two overlapping frequency masks, two overlapping
    time masks.  Each is gathered alone with p_rot = 1 and fill = -3.5: masked elements hold the fill as bits (they are
    `exact` in the reference), the others the rotated value."""
    name, target = "scalar_4x3x5", TARGETS[0]
    (C, F, T), _, _ = CASES[name]
    index = [p % N_ROWS for p in range(4096)]
    aug_kw = dict(p_rot=1.0, freq_masks=2, freq_width=F, time_masks=2, time_width=T, fill=-3.5)
    found = {}
    for p in range(4096):
        d = A.draws(3, 0, p, 0, 0.0, 2, F, F, 2, T, T)
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
        ox, oy, ref = _call(name, target, p, 1, aug_kw, index=index)
        assert ref["rows"][0]["rotate"]
        _hold(ox, ref["x"], 8, "plain", what)
        _hold(oy, ref["y"], 8, "plain", what)
        if what in ("all_f", "all_t"):
            assert bool((ox[0] == -3.5).all())
        else:
            assert bool((ox[0] == -3.5).any())
        assert bool((ox[1:] == SENTINEL).all())


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_draws_follow_the_position_not_the_form_of_the_call():
    H = pkg().hip_ops
    name, target = "vector_8x8x64", TARGETS[1]
    shape, triples, _ = CASES[name]
    _, _, xd, yd = _data(name, target)
    aug = H.Augment(rot_triples=triples, p_rot=0.7, freq_masks=1, freq_width=4, time_masks=2, time_width=20, device=DEV)
    idx = torch.tensor([3, 1, 0, 4, 2, 2, 1, 0, 3, 4, 1, 2], device=DEV)
    ax, ay = _buffers(shape, target)
    H.gather_rows_rot(xd, yd, idx, ax, ay, epoch=_epoch(2), seed=11, augment=aug, start=4)
    bx, by = _buffers(shape, target)
    H.gather_rows_rot(xd, yd, idx, bx, by, epoch=_epoch(2), seed=11, augment=aug, cursor=torch.tensor([2], device=DEV, dtype=torch.int32),
                      stride=1, start=2)
    assert torch.equal(_bits(ax), _bits(bx)) and torch.equal(_bits(ay), _bits(by))
    cx, cy = torch.zeros((2,) + shape, device=DEV), torch.zeros((2, target[0], 4 * target[1]), device=DEV)
    H.gather_rows_rot(xd, yd, idx, cx, cy, epoch=_epoch(2), seed=11, augment=aug, start=6)
    assert torch.equal(_bits(cx), _bits(ax[2:4])) and torch.equal(_bits(cy), _bits(ay[2:4]))
    H.gather_rows_rot(xd, yd, idx, bx, by, epoch=_epoch(3), seed=11, augment=aug, start=4)
    assert not torch.equal(ax, bx)                               # another epoch: other draws


def test_rotated_samples_over_4096_positions_are_the_references():
    """One target row [1 | 1 2 3] gathered alone (no predictors) at 4096 positions with p_rot = 0.3: a sample is rotated iff
    its location moved, and that set is u01(w[1]) < p_rot of the reference's group 3, word for word."""
    H = pkg().hip_ops
    y = torch.tensor([[[1.0, 1.0, 2.0, 3.0]]], device=DEV)
    out = torch.zeros(4096, 1, 4, device=DEV)
    H.gather_rows_rot(None, y, torch.zeros(4096, dtype=torch.int64, device=DEV), None, out, epoch=_epoch(5), seed=77,
                      augment=H.Augment(rot_triples=[(0, 1, 2)], p_rot=0.3, device=DEV))
    out = out.cpu().numpy().reshape(4096, 4)
    assert (out[:, 0] == 1).all()
    moved = (out[:, 1:] != np.array([1.0, 2.0, 3.0], dtype=np.float32)).any(axis=1)
    want = R.rotated_flags(77, 5, np.arange(4096), 0.3)
    assert np.array_equal(moved, want) and 1000 < want.sum() < 1500
    assert want[7] == R.rotation(77, 5, 7, 0.3)["rotate"]
    assert np.allclose(np.linalg.norm(out[:, 1:3], axis=1), np.sqrt(5.0), rtol=1e-6) and (np.abs(out[:, 3]) == 3).all()


# ---- 6, 7 ---------------------------------------------------------------------------------------------------------------
LOADER_AUG = dict(p_rot=0.6, freq_masks=1, freq_width=3, time_masks=2, time_width=5, fill=0.5)


def _loader_data():
    rng = np.random.default_rng(17)
    return (torch.from_numpy(rng.standard_normal((8, 4, 5, 8)).astype(np.float32)).to(DEV),
            torch.from_numpy(rng.standard_normal((8, 3, 8)).astype(np.float32)).to(DEV))


def test_recorded_fetch_draws_anew_at_every_replay_and_epoch():
    """fetch() + step_end recorded in ONE graph (no parallel branch), replayed through two epochs with begin_epoch in
    between: every replayed batch holds the bits of the eager gather_rows_rot of its (epoch, position)."""
    H, T = pkg().hip_ops, pkg().train
    xd, yd = _loader_data()
    aug = H.Augment(rot_triples=[(3, 1, 2)], device=DEV, **LOADER_AUG)
    loader = T.ResidentLoader(xd, yd, 4, False, augment=aug, seed=4)
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
    idx = torch.arange(8, device=DEV)
    seen = []
    for epoch in range(2):
        loader.begin_epoch()
        for i in range(2):
            graph.replay()
            ex, ey = torch.zeros_like(loader.x), torch.zeros_like(loader.target)
            H.gather_rows_rot(xd, yd, idx, ex, ey, epoch=_epoch(epoch), seed=4, augment=aug, start=4 * i)
            assert torch.equal(_bits(loader.x), _bits(ex)) and torch.equal(_bits(loader.target), _bits(ey)), (epoch, i)
            seen.append(loader.x.clone())
        assert int(loader.cursor) == 2 and int(loader.epoch) == epoch
    assert not torch.equal(seen[0], seen[2]) and not torch.equal(seen[1], seen[3])
    assert any(not torch.equal(s, xd[4 * (i % 2):4 * (i % 2) + 4]) for i, s in enumerate(seen))


def test_resident_loader_launches_the_rotating_gather_only_when_p_rot_is_positive():
    H, T = pkg().hip_ops, pkg().train
    xd, yd = _loader_data()
    loaders = ((T.ResidentLoader(xd, yd, 4, False), "gather_rows_kernel"),
               (T.ResidentLoader(xd, yd, 4, False, augment=H.Augment(freq_masks=1, freq_width=2, device=DEV)), "gather_rows_aug_kernel"),
               (T.ResidentLoader(xd, yd, 4, False, augment=H.Augment(rot_triples=[(3, 1, 2)], freq_masks=1, freq_width=2, device=DEV)),
                "gather_rows_aug_kernel"),
               (T.ResidentLoader(xd, yd, 4, False, augment=H.Augment(rot_triples=[(3, 1, 2)], p_rot=0.5, device=DEV)), "gather_rows_rot_kernel"))
    timer = H.kernel_timer
    was = timer.active, timer.only
    try:
        timer.active, timer.only = True, None
        for loader, label in loaders:
            timer.reset()
            loader.begin_epoch()
            loader.fetch()
            loader.fetch(3, batch=1)
            torch.cuda.synchronize()
            assert [r[0] for r in timer.records] == [label, label]
    finally:
        timer.active, timer.only = was
        timer.reset()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_graphed_train_step_on_rotated_quaternion_batches_reproduces_the_eager_losses(seld_env):
    """GraphedTrainStep(loader=...) on the tiny DQ model, input in the quaternion layout of 2 microphones (8 channels), with
    the Augment of --augment_rotate plus masks: three replays against three eager steps over the same positions in
    deterministic mode.  The losses are finite and equal bit for bit, and so are the batches the two runs trained on."""
    from tests.golden.cases import MODEL_CASES
    seld_env.set("SELD_DETERMINISTIC", "1")
    H, T = pkg().hip_ops, pkg().train
    case = next(c for c in MODEL_CASES if c["name"] == "tiny_DQ")
    shape = (case["input_channels"], case["freq_dim"], case["time_dim"])
    assert shape[0] == 8
    rng = np.random.default_rng(23)
    x = torch.from_numpy(rng.standard_normal((6,) + shape).astype(np.float32)).to(DEV)
    y = torch.from_numpy(np.concatenate([(rng.random((6, 8, 42)) < 0.1).astype(np.float32),
                                         rng.uniform(-1, 1, (6, 8, 126)).astype(np.float32)], 2)).to(DEV)
    aug = H.Augment(rot_triples=H.foa_triples(mics=2, layout="quaternion"), p_rot=0.8, freq_masks=2, freq_width=16, time_masks=1,
                    time_width=10, device=DEV)

    def fresh():
        H.philox.set_offset(0)
        H.hcq_weights.reset()
        model = build_model(case).to(DEV).train()
        return model, T.FlatAdam(model.parameters(), lr=1e-3), T.ResidentLoader(x, y, 2, False, augment=aug, seed=6)

    model, opt, loader = fresh()
    snap = T.training_snapshot(model, opt)
    loader.fetch(batch=0)
    runner = T.GraphedTrainStep(model, opt, loader.x, loader.target, 42, 1.0, 5.0, warmup=1, loader=loader)
    T.training_restore(model, opt, snap)
    assert int(loader.epoch) == -1 and int(loader.cursor) == 0       # warm-up and recording moved neither
    loader.begin_epoch()
    graphed, batches = [], []
    for _ in range(3):
        loss = runner()
        graphed.append(float(loss.item()))
        batches.append((loader.x.clone(), loader.target.clone()))
    assert int(loader.cursor) == 3 and bool(torch.isfinite(loader.mean).all())

    model, opt, loader = fresh()
    loader.begin_epoch()
    eager = []
    for i in range(3):
        bx, by = loader.fetch()
        assert torch.equal(_bits(bx), _bits(batches[i][0])) and torch.equal(_bits(by), _bits(batches[i][1])), i
        opt.zero_grad()
        sed, doa = model(bx)
        loss = T.seld_loss_fn(sed, doa, by, 42, 1.0, 5.0)
        loss.backward()
        opt.step()
        loader.step_end(loss.detach())
        eager.append(float(loss.item()))
    print("losses: graphed", graphed, "eager", eager)
    assert all(np.isfinite(graphed)) and graphed == eager, (graphed, eager)
    assert any(not torch.equal(bx_, x[2 * i:2 * i + 2]) for i, (bx_, _) in enumerate(batches))      # something was augmented


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_launch_nothing():
    H, L = pkg().hip_ops, pkg()._lib
    name, target = "scalar_4x3x5", (3, 2)
    (C, F, T), _, _ = CASES[name]
    _, _, xd, _ = _data(name, TARGETS[0])
    yd = torch.zeros(N_ROWS, 3, 8, device=DEV)
    ox, oy = _buffers((C, F, T), target)
    idx = torch.arange(N_ROWS, device=DEV)
    ep = _epoch(0)
    mats = torch.eye(3, device=DEV).reshape(1, 9).repeat(B, 1).contiguous()
    lib, s = L.lib(), L.current_stream()
    good = dict(x_all=L.ptr(xd), row_x=C * F * T, out_x=L.ptr(ox), y_all=L.ptr(yd), row_y=3 * 8, out_y=L.ptr(oy), index=L.ptr(idx),
                n_index=N_ROWS, n_rows=N_ROWS, cursor=None, stride=B, start=0, B=B, count=B, C=C, F=F, T=T, y_cols=8, epoch=L.ptr(ep),
                seed=1, triples=0x213, n_triples=1, p_rot=0.5, rot_mirror=1, rot_zflip=1, matrices=L.ptr(mats), n_fmask=1, f_max=F,
                n_tmask=1, t_max=T, fill=0.0)
    bad = [dict(n_triples=0), dict(n_triples=6), dict(n_triples=2), dict(n_triples=-1), dict(p_rot=1.5), dict(p_rot=-0.5),
           dict(p_rot=float("nan")), dict(epoch=None), dict(epoch=None, matrices=None), dict(count=B + 1), dict(count=B + 1, matrices=None),
           dict(triples=0x413), dict(triples=0x113), dict(triples=0x1213), dict(C=17, row_x=17 * F * T), dict(C=0), dict(C=2, row_x=2 * F * T),
           dict(F=0), dict(T=-1), dict(row_x=C * F * T + 4), dict(y_cols=6), dict(y_cols=0), dict(y_cols=16), dict(n_fmask=3),
           dict(n_fmask=-1), dict(n_tmask=3), dict(f_max=F + 1), dict(f_max=-1), dict(t_max=T + 1), dict(t_max=-1),
           dict(n_index=2 ** 32 + 1), dict(count=0), dict(index=None), dict(out_x=None), dict(stride=-1, cursor=L.ptr(ep))]
    for change in bad:
        args = dict(good, **change)
        assert lib.seld_gather_rows_rot(*args.values(), s) == -1, change
    torch.cuda.synchronize()
    assert bool((ox == SENTINEL).all()) and bool((oy == SENTINEL).all())        # nothing was launched
    assert lib.seld_gather_rows_rot(*good.values(), s) == 0
    assert lib.seld_gather_rows_rot(*dict(good, matrices=None).values(), s) == 0
    torch.cuda.synchronize()
    aug = H.Augment(rot_triples=[(3, 1, 2)], p_rot=0.5, device=DEV)
    call = lambda **kw: H.gather_rows_rot(**dict(dict(x_all=xd, y_all=yd, index=idx, out_x=ox, out_y=oy, epoch=ep, seed=1, augment=aug), **kw))
    for kw in (dict(augment=None), dict(augment=H.Augment(p_swap=0.0, device=DEV)), dict(epoch=ep.to(torch.int64)),
               dict(augment=H.Augment(rot_triples=[(3, 1, 4)], device=DEV)), dict(matrices=mats[:2]), dict(matrices=mats.double()),
               dict(matrices=mats.cpu()), dict(matrices=mats.reshape(-1)), dict(matrices=torch.zeros(B, 3, 4, device=DEV)),
               dict(x_all=xd.reshape(N_ROWS, -1), out_x=ox.reshape(B, -1))):
        with pytest.raises(L.SeldHipError):
            call(**kw)
    call(matrices=mats.reshape(B, 3, 3))


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_quaternion_table_through_gather_rows_aug_equals_the_host_reference():
    H = pkg().hip_ops
    name, target = "vector_8x8x64", TARGETS[0]
    shape, _, _ = CASES[name]
    x, y, xd, yd = _data(name, target)
    table = H.foa_transforms(mics=2, layout="quaternion")
    masks = dict(freq_masks=1, freq_width=3, time_masks=1, time_width=9, fill=0.5)
    ox, oy = _buffers(shape, target)
    H.gather_rows_aug(xd, yd, torch.tensor(INDEX, device=DEV), ox, oy, epoch=_epoch(1), seed=3, start=2,
                      augment=H.Augment(table=table, p_swap=1.0, device=DEV, **masks))
    want_x, want_y = A.gather_aug(x, y, np.asarray(INDEX), 2, B, np.full((B,) + shape, SENTINEL, np.float32),
                                  np.full((B, target[0], 4 * target[1]), SENTINEL, np.float32), seed=3, epoch=1, table=table, p_swap=1.0,
                                  n_fmask=1, f_max=3, n_tmask=1, t_max=9, fill=0.5)
    assert torch.equal(ox.cpu(), torch.from_numpy(want_x)) and torch.equal(oy.cpu(), torch.from_numpy(want_y))
    assert bool((ox[:, 1:4] < 0).any()) and not torch.equal(ox[0], xd[INDEX[2]])


def test_quaternion_table_through_the_window_ensemble_maps_every_doa_back():
    """One tiny recording (1, 4, 2, 8) in the quaternion layout, windows of 4 frames every 4, under the 16 rows of the
    quaternion table.  The "model" is a host function: activity 1 and, per frame, the DOA read off the intensity channels
    (their sum over f, in the (x, y, z) order of foa_triples).  Mapped back through its row, q[axis[a]] = sign[a] *
    doa[a], every member gives the untransformed window's DOA EXACTLY (moving and negating floats commutes with a sum
    taken in the same order); ensemble_combine's mean of 16 equal values (weights 1: 15 additions, one division,
    half an ulp each) is within 16 * 2^-24 of it, relative, plus the smallest normal float."""
    H = pkg().hip_ops
    rng = np.random.default_rng(31)
    x = rng.standard_normal((1, 4, 2, 8)).astype(np.float32)
    table = H.foa_transforms(layout="quaternion")
    (cx, cy, cz), = H.foa_triples(layout="quaternion")
    S, K, T = 2, 16, 4
    out = torch.empty(S * K, 4, 2, T, device=DEV)
    H.window_batch(torch.from_numpy(x).to(DEV), out, seg_len=T, hop=T, segments=S, table=table)
    members = out.cpu().numpy()

    def model(batch):                                           # (M, 4, 2, T) -> sed (M, T, 1), doa (M, T, 3)
        doa = np.stack([batch[:, c, 0] + batch[:, c, 1] for c in (cx, cy, cz)], axis=-1).astype(np.float32)
        return np.ones(doa.shape[:2] + (1,), np.float32), doa
    sed, doa = model(members)
    plain = model(x.reshape(1, 4, 2, S, T).transpose(0, 3, 1, 2, 4).reshape(S, 4, 2, T))[1]        # (S, T, 3)
    for m in range(S * K):
        row = table[m % K]
        back = np.empty((T, 3), np.float32)
        for a in range(3):
            back[:, row[8 + a]] = np.float32(row[11 + a]) * doa[m, :, a]
        assert np.array_equal(back, plain[m // K]), m
        assert m % K == 0 or not np.array_equal(doa[m], plain[m // K])
    got_sed, got_doa = H.ensemble_combine(torch.from_numpy(sed).to(DEV), torch.from_numpy(doa).to(DEV), recordings=1, segments=S,
                                          hop_out=T, frames=S * T, classes=1, overlaps=1, table=table, window="uniform", align=False)
    want = plain.reshape(1, S * T, 3).astype(np.float64)
    assert bool((got_sed == 1).all())
    assert (np.abs(got_doa.cpu().numpy().astype(np.float64) - want) <= 16 * U24 * np.abs(want) + TINY).all()
