"""hip_ops.gather_rows_polar (csrc/loader.hip, seld_gather_rows_polar) and train.ResidentLoader(polar_stats=...) against the
numpy restatement of include/seld_hip.h in tests/loader_polar_ref.py.

Bound.  What the kernel only moves (unrotated samples, channels outside the groups with W among them, masked cells, zero
rows, rows >= count, and every label of a call compared with seld_gather_rows_rot's) is compared as bits.  A rotated
position is compared on the COMPLEX value m e^(i phi) rebuilt in float64 from the destandardised output, which makes the
wrap of the phase at +-pi and the ill-conditioned phase of a small magnitude harmless:

    |got - z'_a| <= K * 2^-24 * Wt_a + TINY,    Wt_a = (sum_j |R[a][j]| (|m_j| + |mean_m|)) * (1 + pi + |mean_p|)

K = 8: the fp32 restatement of the kernel in numpy reaches 1.34 over these inputs (cancelling ones included) on the CPU;
K is 4 times that, rounded up to a power of two, the margin being for the device's sincosf and atan2f
(tests/test_loader_polar_host.py asserts the arithmetic).  Largest ratio seen on an MI355X: 1.33.  Range: m' >= 0 and |phi'| <= fp32 pi hold exactly on raw
output; standardised output is destandardised with two roundings, (v - mean) / sd, each half an ulp of |v| + |mean| at
most, so it is held to the same ranges within 2^-23 (|v| + |mean|)."""
import numpy as np
import pytest
import torch

from tests import loader_polar_ref as P
from tests.helpers import build_model, pkg
from tests.loader_helpers import DEV, SENTINEL, bits as _bits, buffers, epoch as _epoch, hold_polar as _hold_x, shifted

pytestmark = pytest.mark.gpu
B = 4
K, U24, TINY = P.K, P.U24, P.TINY
CASES, STATS, TARGET = P.CASES, P.STATS, P.TARGET
_resident = {}


def _data(name, si):
    """(x, y, groups, x on the device (shifted off alignment where the case says so), y on the device), made once."""
    if (name, si) not in _resident:
        x, y, groups = P.inputs(name, si)
        _resident[(name, si)] = (x, y, groups, shifted(x, CASES[name][2]), torch.tensor(y).to(DEV))
    return _resident[(name, si)]


def _stats_tensor(stats):
    return None if stats is None else torch.tensor(stats, device=DEV, dtype=torch.float32)


def _buffers(x, y, rows=B):
    return buffers(x.shape[1:], y.shape[1:], rows)


def _labels_of_the_rot_kernel(yd, idx, like, **kw):
    """The targets seld_gather_rows_rot writes for the same call (targets alone: its label path needs no predictors)."""
    H = pkg().hip_ops
    out = torch.full_like(like, SENTINEL)
    aug_kw = {k: kw.pop(k) for k in ("p_rot", "rot_mirror", "rot_zflip") if k in kw}
    H.gather_rows_rot(None, yd, idx, None, out, augment=H.Augment(rot_triples=[(0, 1, 2)], device=DEV, **aug_kw), **kw)
    return out


def _call(name, si, first, count, aug_kw, *, matrices=None, seed=3, epoch=0, index=None, rows=B, via_cursor=False):
    """One call of gather_rows_polar and the reference of the same call: (out_x, out_y, reference, groups, stats)."""
    H = pkg().hip_ops
    x, y, groups, xd, yd = _data(name, si)
    stats = STATS[si]
    index = list(range(x.shape[0])) if index is None else index
    aug = H.Augment(rot_polar=groups, device=DEV, **aug_kw)
    ox, oy = _buffers(x, y, rows)
    idx = torch.as_tensor(index, dtype=torch.int64).to(DEV)
    md = None if matrices is None else torch.from_numpy(np.ascontiguousarray(matrices, dtype=np.float32)).to(DEV)
    kw = dict(epoch=_epoch(epoch), seed=seed, matrices=md, count=count)
    if via_cursor:
        stride = 3
        where = dict(cursor=torch.tensor([first // stride], device=DEV, dtype=torch.int32), stride=stride, start=first % stride)
    else:
        where = dict(start=first)
    H.gather_rows_polar(xd, yd, idx, ox, oy, augment=aug, stats=_stats_tensor(stats), **kw, **where)
    rot_y = _labels_of_the_rot_kernel(yd, idx, oy, **{k: v for k, v in aug_kw.items() if k in ("p_rot", "rot_mirror", "rot_zflip")},
                                      **kw, **where)
    assert torch.equal(_bits(oy), _bits(rot_y)), (name, si, first, "labels differ from seld_gather_rows_rot's")
    ref = P.gather_polar(x, y, np.asarray(index), first, count, np.full((rows,) + x.shape[1:], SENTINEL, np.float32),
                         np.full((rows,) + y.shape[1:], SENTINEL, np.float32), seed=seed, epoch=epoch, groups=groups, stats=stats,
                         p_rot=aug_kw.get("p_rot", 0.0), rot_mirror=aug_kw.get("rot_mirror", True), rot_zflip=aug_kw.get("rot_zflip", True),
                         matrices=matrices, n_fmask=aug_kw.get("freq_masks", 0), f_max=aug_kw.get("freq_width", 0),
                         n_tmask=aug_kw.get("time_masks", 0), t_max=aug_kw.get("time_width", 0), fill=aug_kw.get("fill", 0.0))
    return ox, oy, ref, groups, stats


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(STATS)))
@pytest.mark.parametrize("name", list(CASES))
def test_explicit_general_rotations(name, si):
    """Rotations about random axes, every other one mirrored; through `start` and through the cursor, count below B, an
    invalid index and a position past the index in between; the last call with masks of fill -1.5 over rotated values."""
    n = CASES[name][0][0]
    index = [n - 1, -1, 0, 2, 1, n, 3, 1]
    mats = P.general_rotations(B, len(name))
    for i, (first, count) in enumerate(((0, 3), (2, 4), (5, 4))):
        masks = dict(freq_masks=1, freq_width=2, time_masks=2, time_width=3, fill=-1.5) if i == 2 else {}
        ox, oy, ref, groups, stats = _call(name, si, first, count, masks, matrices=mats[:count], index=index, via_cursor=i == 1)
        _hold_x(ox, ref["x"], groups, stats, (name, si, first))
        assert P.bits_equal(oy.cpu().numpy(), ref["y"]["ref"])[ref["y"]["exact"]].all()
        invalid = [b for b, d in enumerate(ref["rows"]) if d is None]
        assert invalid and all(not ox[b].any() and not oy[b].any() for b in invalid)
        assert bool((ox[count:] == SENTINEL).all()) and bool((oy[count:] == SENTINEL).all())
        assert not ref["x"]["exact"][:count].all()                      # something was rotated and left unmasked
        if i == 2:
            assert bool((ox[:count] == -1.5).any()) == bool((ref["x"]["ref"][:count] == -1.5).any())


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vector_8x5x12", "scalar_16x9x7"])
def test_signed_permutations_agree_with_the_table_rows_of_gather_rows_aug(name):
    """Every row k of foa_transforms(phase=True) as an explicit matrix M[a][axis[a]] = sign[a], on raw data, against
    gather_rows_aug with that one row at p_swap = 1: the same complex value within the bound (the table path permutes
    magnitudes and turns phases by pi; this one goes through sincosf and atan2f), labels equal."""
    H = pkg().hip_ops
    x, y, groups, xd, yd = _data(name, 0)
    mics = CASES[name][1]
    C = x.shape[1]
    table = H.foa_transforms(mics=mics, phase=True)
    assert table.shape == (16, 2 * C + 6)
    idx = torch.tensor([2, 0, 4, 3], device=DEV)
    rot = H.Augment(rot_polar=groups, device=DEV)
    for k, row in enumerate(table):
        M = np.zeros((3, 3), dtype=np.float32)
        for a in range(3):
            M[a, row[2 * C + a]] = row[2 * C + 3 + a]
        mats = np.tile(M.reshape(1, 9), (B, 1))
        rx, ry = _buffers(x, y)
        H.gather_rows_polar(xd, yd, idx, rx, ry, epoch=_epoch(0), seed=1, augment=rot, matrices=torch.from_numpy(mats).to(DEV))
        ax, ay = _buffers(x, y)
        H.gather_rows_aug(xd, yd, idx, ax, ay, epoch=_epoch(0), seed=1, augment=H.Augment(table=table[k:k + 1], p_swap=1.0, device=DEV))
        assert bool((ry == ay).all()), k
        ref = P.gather_polar(x, None, idx.cpu().numpy(), 0, B, np.zeros((B,) + x.shape[1:], np.float32), None, seed=1, epoch=0,
                             groups=groups, matrices=mats)["x"]
        za, _, _ = P.complex_of(ax.cpu().numpy(), groups, None)
        zr, _, _ = P.complex_of(rx.cpu().numpy(), groups, None)
        inexact = ~ref["exact"]
        bound = (K * U24 * ref["weight"] + TINY)[inexact]
        assert (np.abs(za - ref["z"])[inexact] <= bound).all(), k          # the table row is the same rotation
        assert (np.abs(zr - za)[inexact] <= bound).all(), k
        same = torch.from_numpy(ref["exact"]).to(DEV)
        assert torch.equal(_bits(rx)[same], _bits(ax)[same]), k           # W and everything else: bits


# ---- 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(STATS)))
@pytest.mark.parametrize("name", list(CASES))
def test_drawn_rotations_over_two_epochs(name, si):
    """p_rot = 0.6 over 12 positions and two epochs, through `start` and through the cursor, count below the buffer's rows:
    rotated positions within the bound, the rest as bits; the labels are seld_gather_rows_rot's bit for bit (in _call);
    which samples rotate is the reference's draw."""
    n = CASES[name][0][0]
    index = [p % n for p in range(12)]
    seen = []
    for epoch in (0, 1):
        ox, oy, ref, groups, stats = _call(name, si, 1 if epoch else 0, 11 if epoch else 12, dict(p_rot=0.6), seed=9, epoch=epoch,
                                           index=index, rows=12, via_cursor=bool(epoch))
        _hold_x(ox, ref["x"], groups, stats, (name, si, "epoch", epoch))
        flags = [d["rotate"] for d in ref["rows"]]
        want = P.rotated_flags(9, epoch, np.arange(len(flags)) + (1 if epoch else 0), 0.6)
        assert flags == list(want) and 0 < sum(flags) < len(flags)
        moved = [not torch.equal(_bits(oy[b]), _bits(_data(name, si)[4][index[(1 if epoch else 0) + b]])) for b in range(len(flags))]
        assert moved == flags
        seen.append(flags[:11] if not epoch else flags)
    assert seen[0] != seen[1]


def test_one_pair_alone():
    """The x pair only and the y pair only give what the call with both gives."""
    H = pkg().hip_ops
    name, si = "vector_8x5x12", 1
    x, y, groups, xd, yd = _data(name, si)
    aug = H.Augment(rot_polar=groups, p_rot=0.6, freq_masks=1, freq_width=2, device=DEV)
    idx = torch.tensor([3, 1, 0, 6, 2, 5], device=DEV)
    kw = dict(epoch=_epoch(1), seed=5, augment=aug, stats=_stats_tensor(STATS[si]), start=1)
    bx, by = _buffers(x, y)
    H.gather_rows_polar(xd, yd, idx, bx, by, **kw)
    ox, _ = _buffers(x, y)
    H.gather_rows_polar(xd, None, idx, ox, None, **kw)
    _, oy = _buffers(x, y)                      # targets alone have the geometry (C, 1, 1): no room for a mask, and no use
    H.gather_rows_polar(None, yd, idx, None, oy, **dict(kw, augment=H.Augment(rot_polar=groups, p_rot=0.6, device=DEV)))
    assert torch.equal(_bits(ox), _bits(bx)) and torch.equal(_bits(oy), _bits(by))
    assert not torch.equal(bx, xd[idx[1:5]]) and not torch.equal(by, yd[idx[1:5]])


def test_masks_after_a_rotation_write_the_fill():
    """p_rot = 1 with two frequency and two time masks of fill -1.5 on standardised data: masked cells hold the fill as bits
    in every channel, the others the rotated value."""
    name, si = "tiles_8x33x68", 2
    ox, oy, ref, groups, stats = _call(name, si, 0, 4, dict(p_rot=1.0, freq_masks=2, freq_width=9, time_masks=2, time_width=20, fill=-1.5),
                                       seed=12, epoch=2)
    assert all(d["rotate"] for d in ref["rows"])
    _hold_x(ox, ref["x"], groups, stats, "masks")
    masked = ref["x"]["exact"][:, groups[0][0]]
    assert masked.any() and not masked.all()
    assert bool((ox.cpu().numpy().transpose(0, 2, 3, 1)[masked] == -1.5).all())


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_launch_nothing():
    H, L = pkg().hip_ops, pkg()._lib
    x, _, groups, xd, _ = _data("vector_8x5x12", 0)
    n, C, F, T = x.shape
    yd = torch.zeros(n, 3, 8, device=DEV)
    ox, oy = torch.full((B, C, F, T), SENTINEL, device=DEV), torch.full((B, 3, 8), SENTINEL, device=DEV)
    idx = torch.arange(n, device=DEV)
    ep = _epoch(0)
    mats = torch.eye(3, device=DEV).reshape(1, 9).repeat(B, 1).contiguous()
    st = _stats_tensor(STATS[1])
    lib, s = L.lib(), L.current_stream()
    good = dict(x_all=L.ptr(xd), row_x=C * F * T, out_x=L.ptr(ox), y_all=L.ptr(yd), row_y=3 * 8, out_y=L.ptr(oy), index=L.ptr(idx),
                n_index=n, n_rows=n, cursor=None, stride=B, start=0, B=B, count=B, C=C, F=F, T=T, y_cols=8, epoch=L.ptr(ep),
                seed=1, groups=0x657213, n_groups=1, stats=L.ptr(st), p_rot=0.5, rot_mirror=1, rot_zflip=1, matrices=L.ptr(mats),
                n_fmask=1, f_max=F, n_tmask=1, t_max=T, fill=0.0)
    bad = [dict(n_groups=0), dict(n_groups=3), dict(n_groups=2), dict(n_groups=-1), dict(p_rot=1.5), dict(p_rot=-0.5),
           dict(p_rot=float("nan")), dict(epoch=None), dict(epoch=None, matrices=None), dict(count=B + 1), dict(count=B + 1, matrices=None),
           dict(groups=0x658213), dict(groups=0x651213), dict(groups=0x4657213), dict(groups=0x657213 | 1 << 60),
           dict(C=17, row_x=17 * F * T), dict(C=0), dict(C=5, row_x=5 * F * T), dict(C=7, row_x=7 * F * T), dict(F=0), dict(T=-1),
           dict(row_x=C * F * T + 4), dict(y_cols=6), dict(y_cols=0), dict(y_cols=16), dict(n_fmask=3), dict(n_fmask=-1),
           dict(n_tmask=3), dict(f_max=F + 1), dict(f_max=-1), dict(t_max=T + 1), dict(t_max=-1), dict(n_index=2 ** 32 + 1),
           dict(count=0), dict(index=None), dict(out_x=None), dict(stride=-1, cursor=L.ptr(ep))]
    for change in bad:
        args = dict(good, **change)
        assert lib.seld_gather_rows_polar(*args.values(), s) == -1, change
    torch.cuda.synchronize()
    assert bool((ox == SENTINEL).all()) and bool((oy == SENTINEL).all())        # nothing was launched
    assert lib.seld_gather_rows_polar(*good.values(), s) == 0
    assert lib.seld_gather_rows_polar(*dict(good, matrices=None, stats=None).values(), s) == 0
    torch.cuda.synchronize()
    aug = H.Augment(rot_polar=groups, p_rot=0.5, device=DEV)
    call = lambda **kw: H.gather_rows_polar(**dict(dict(x_all=xd, y_all=yd, index=idx, out_x=ox, out_y=oy, epoch=ep, seed=1, augment=aug), **kw))
    for kw in (dict(augment=None), dict(augment=H.Augment(rot_triples=[(3, 1, 2)], device=DEV)), dict(epoch=ep.to(torch.int64)),
               dict(augment=H.Augment(rot_polar=H.foa_polar(mics=2), device=DEV)), dict(matrices=mats[:2]), dict(matrices=mats.cpu()),
               dict(stats=st.cpu()), dict(stats=st.double()), dict(stats=st[:3]), dict(stats=[2.5, 3.1, 0.01, 1.8]),
               dict(stats=torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV)), dict(stats=torch.tensor([0.0, 1.0, 0.0, -1.0], device=DEV)),
               dict(stats=torch.tensor([float("nan"), 1.0, 0.0, 1.0], device=DEV)),
               dict(stats=torch.tensor([0.0, 1.0, float("inf"), 1.0], device=DEV)),
               dict(x_all=xd.reshape(n, -1), out_x=ox.reshape(B, -1))):
        with pytest.raises(L.SeldHipError):
            call(**kw)
    call(stats=st, matrices=mats.reshape(B, 3, 3))
    st.mul_(0)                                                                   # changed in place: looked at again
    with pytest.raises(L.SeldHipError):
        call(stats=st)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_loader_statistics_from_normalize_dataset():
    """normalize_dataset(..., stats=[]) on a small raw array, the loader over the standardised array with those statistics:
    an unrotated sample is the standardised row bit for bit, a rotated one is within the bound of the reference computed
    from the statistics the device reports."""
    import argparse
    H, T = pkg().hip_ops, pkg().train
    rng = np.random.default_rng(41)
    n, C, F, Tn = 8, 8, 6, 8
    raw = np.concatenate([np.abs(rng.standard_normal((n, 4, F, Tn))) * 3 + 1, rng.uniform(-np.pi, np.pi, (n, 4, F, Tn))], 1).astype(np.float32)
    xd = torch.from_numpy(raw).to(DEV)
    yd = torch.from_numpy(rng.standard_normal((n,) + TARGET).astype(np.float32)).to(DEV)
    args = argparse.Namespace(dataset_normalization="True", n_mics=1, phase=True, domain="DQ")
    got = []
    T.normalize_dataset(args, xd, stats=got)
    assert len(got) == 1 and len(got[0]) == 2
    off = []
    T.normalize_dataset(argparse.Namespace(dataset_normalization="False", n_mics=1, phase=True, domain="DQ"), xd, xd, stats=off)
    assert off == [None, None]
    st = T.polar_stats_from(got[0], DEV)
    stats = tuple(float(v) for v in st.tolist())
    assert abs(stats[0] - raw[:, :4].mean()) < 1e-4 and abs(stats[1] - raw[:, :4].std()) < 1e-4 and stats[3] > 1
    aug = H.Augment(rot_polar=H.foa_polar(), p_rot=0.6, device=DEV)
    loader = T.ResidentLoader(xd, yd, 8, False, augment=aug, seed=21, polar_stats=st)
    loader.begin_epoch()
    bx, by = loader.fetch()
    x = xd.cpu().numpy()
    ref = P.gather_polar(x, yd.cpu().numpy(), np.arange(n), 0, n, np.zeros_like(x), np.zeros((n,) + TARGET, np.float32), seed=21, epoch=0,
                         groups=H.foa_polar(), stats=stats, p_rot=0.6)
    flags = [d["rotate"] for d in ref["rows"]]
    assert 0 < sum(flags) < n
    for b, rotated in enumerate(flags):
        assert torch.equal(_bits(bx[b]), _bits(xd[b])) == (not rotated)
    _hold_x(bx, ref["x"], H.foa_polar(), stats, "loader statistics")
    assert P.bits_equal(by.cpu().numpy(), ref["y"]["ref"])[ref["y"]["exact"]].all()


def test_resident_loader_routes_polar_augments_to_the_polar_gather():
    H, T = pkg().hip_ops, pkg().train
    x, y, groups, xd, yd = _data("vector_8x5x12", 0)
    loaders = ((T.ResidentLoader(xd, yd, 4, False, augment=H.Augment(rot_polar=groups, freq_masks=1, freq_width=2, device=DEV)),
                "gather_rows_aug_kernel"),
               (T.ResidentLoader(xd, yd, 4, False, augment=H.Augment(rot_polar=groups, p_rot=0.5, device=DEV)), "gather_rows_polar_kernel"),
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


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_graphed_train_step_on_rotated_magphase_batches_reproduces_the_eager_losses(seld_env):
    """GraphedTrainStep(loader=...) on the tiny DQ model with 16 input channels (two microphones, magnitude and phase),
    standardised predictors with polar_stats, the Augment of --augment_rotate plus masks: three replays against three eager
    steps over the same positions in deterministic mode.  Losses and batches are equal bit for bit."""
    from tests.golden.cases import MODEL_CASES
    seld_env.set("SELD_DETERMINISTIC", "1")
    H, T = pkg().hip_ops, pkg().train
    case = next(c for c in MODEL_CASES if c["name"] == "tiny_DQ16")
    shape = (case["input_channels"], case["freq_dim"], case["time_dim"])
    assert shape[0] == 16
    rng = np.random.default_rng(29)
    stats = STATS[1]
    raw = np.concatenate([np.abs(rng.standard_normal((6, 8) + shape[1:])) * 3, rng.uniform(-np.pi, np.pi, (6, 8) + shape[1:])], 1)
    raw[:, :8] = (raw[:, :8] - stats[0]) / stats[1]
    raw[:, 8:] = (raw[:, 8:] - stats[2]) / stats[3]
    x = torch.from_numpy(raw.astype(np.float32)).to(DEV)
    y = torch.from_numpy(np.concatenate([(rng.random((6, 8, 42)) < 0.1).astype(np.float32),
                                         rng.uniform(-1, 1, (6, 8, 126)).astype(np.float32)], 2)).to(DEV)
    st = _stats_tensor(stats)
    aug = H.Augment(rot_polar=H.foa_polar(mics=2), p_rot=0.8, freq_masks=2, freq_width=16, time_masks=1, time_width=10, device=DEV)

    def fresh():
        H.philox.set_offset(0)
        H.hcq_weights.reset()
        model = build_model(case).to(DEV).train()
        return model, T.FlatAdam(model.parameters(), lr=1e-3), T.ResidentLoader(x, y, 2, False, augment=aug, seed=6, polar_stats=st)

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


# ---- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalization", ["True", "False"])
def test_main_trains_on_rotated_magnitude_phase_batches(tmp_path, normalization):
    """train.main on 5 pickled two-microphone magnitude-phase samples (16 channels), --phase=True --resident_loader=True
    --graph_step=True --augment_rotate=0.5, with and without dataset standardisation: one epoch of three steps (two
    replays and a partial eager batch) with finite losses, fetched by the polar gather with the training array's
    statistics (none on raw data)."""
    import pickle
    from tests.test_gpu_train_loader import MODEL_FLAGS
    T, H = pkg().train, pkg().hip_ops
    rng = np.random.default_rng(13)
    paths = {}
    for split, n in (("training", 5), ("validation", 2)):
        x = np.concatenate([rng.random((n, 8, 128, 64)) * 3 + 0.05, rng.uniform(-np.pi, np.pi, (n, 8, 128, 64))], 1).astype(np.float32)
        act = (rng.random((n, 8, 42)) < 0.15).astype(np.float32)
        loc = rng.uniform(-1, 1, (n, 8, 126)).astype(np.float32) * np.repeat(act, 3, axis=2)
        for kind, arr in (("predictors", x), ("target", np.concatenate([act, loc], axis=2))):
            paths[f"{split}_{kind}_path"] = str(tmp_path / f"{split}_{kind}.pkl")
            with open(paths[f"{split}_{kind}_path"], "wb") as f:
                pickle.dump(arr, f)
    paths["test_predictors_path"] = paths["test_target_path"] = str(tmp_path / "absent.pkl")
    flags = dict(MODEL_FLAGS, **paths, results_path=str(tmp_path / "res"), checkpoint_dir=str(tmp_path / "ck"), batch_size=2, epochs=1,
                 min_n_epochs=1, input_channels=16, phase="True", dataset_normalization=normalization, resident_loader="True",
                 graph_step="True", augment_rotate=0.5, augment_time_masks=1, augment_time_width=8)
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    made = []
    real = T.ResidentLoader

    class Recording(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    calls = []
    real_gather = H.gather_rows_polar

    def counting(*a, **kw):
        calls.append(kw.get("stats"))
        return real_gather(*a, **kw)
    T.ResidentLoader, H.gather_rows_polar = Recording, counting
    try:
        history = []
        state = T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]), history=history)
        torch.cuda.synchronize()
    finally:
        T.ResidentLoader, H.gather_rows_polar = real, real_gather
    assert state["epochs"] == 1 and state["step"] == 3
    assert len(history) == 1 and all(np.isfinite(v) for v in history[0][1:])
    train = made[0]
    assert train.augment.rot_polar == tuple(H.foa_polar(mics=2)) and train.augment.p_rot == 0.5
    assert all(m.augment is None and m.polar_stats is None for m in made[1:])           # validation sees the data as it is
    assert calls and all(c is train.polar_stats for c in calls)          # every training fetch, recorded or eager, went this way
    if normalization == "True":
        st = train.polar_stats.tolist()
        assert len(st) == 4 and st[1] > 0 and 1.5 < st[3] < 2.1 and abs(st[2]) < 0.1
        assert abs(float(train.x_all[:, :8].mean())) < 1e-3 and abs(float(train.x_all[:, 8:].std()) - 1) < 1e-3
    else:
        assert train.polar_stats is None
