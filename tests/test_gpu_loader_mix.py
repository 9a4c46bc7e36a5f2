"""hip_ops.gather_rows_mix and hip_ops.target_occupancy (csrc/loader.hip, seld_gather_rows_mix, seld_target_occupancy) and
train.ResidentLoader with an Augment of kind 'mix' against the numpy restatement of include/seld_hip.h in
tests/loader_mix_ref.py.

Bound.  What the kernel only moves (samples that are not mixed, masked cells, zero rows, rows >= count) and every target
element, merged or not, is compared as bits.  A mixed predictor position is compared on the COMPLEX value m e^(i phi)
rebuilt in float64 from the destandardised output, which makes the wrap of the phase at +-pi and the ill-conditioned phase
of a small magnitude (the engineered bins that cancel) harmless:

    |got - (z_A + g z_B)| <= K * 2^-24 * Wt + TINY,    Wt = ((|m_A| + |mean_m|) + g (|m_B| + |mean_m|)) * (1 + pi + |mean_p|)

K = 8: the fp32 restatement of the kernel in numpy reaches 1.29 over these inputs on the CPU; K is 4 times that, rounded up
to a power of two, the margin being for the device's sincosf and atan2f (tests/test_loader_mix_host.py asserts the
arithmetic).  Range: m' >= 0 and |phi'| <= fp32 pi hold exactly on raw output; standardised output is destandardised with
two roundings and held to the same ranges within 2^-23 (|v| + |mean|), as in tests/loader_helpers.hold_polar."""
import numpy as np
import pytest
import torch

from tests import loader_mix_ref as M
from tests.helpers import build_model, pkg
from tests.loader_helpers import DEV, PI32, SENTINEL, bits as _bits, buffers, epoch as _epoch, shifted

pytestmark = pytest.mark.gpu
B = 4
CASES, STATS = M.CASES, M.STATS
_resident = {}
_seen = {"ratio": 0.0}


def _data(name, si, overlaps=3):
    """(x, y, x on the device (shifted off alignment where the case says so), y on the device, occupancy of y), made once."""
    key = (name, si, overlaps)
    if key not in _resident:
        x = M.inputs(name, si)
        y = M.targets(x.shape[0], overlaps)
        _resident[key] = (x, y, shifted(x, CASES[name][2]), torch.tensor(y).to(DEV), M.occupancy(y, overlaps))
    return _resident[key]


def _stats_tensor(stats):
    return None if stats is None else torch.tensor(stats, device=DEV, dtype=torch.float32)


def _hold_x(got, side, stats, what):
    """Exact positions as bits; the complex value of the others within K * 2^-24 * Wt + TINY; the ranges."""
    got = got.cpu().numpy()
    exact = side["exact"]
    assert M.bits_equal(got, side["ref"])[exact].all(), what
    if exact.all():
        return
    z, Mg, Ph = M.complex_of(got, stats)
    err = np.abs(z - side["z"])[~exact]
    bound = (M.K * M.U24 * side["weight"] + M.TINY)[~exact]
    ratio = M.error_ratio(got, side, stats)
    _seen["ratio"] = max(_seen["ratio"], ratio)
    print(what, "largest |got - ref| / (2^-24 Wt):", ratio, "largest so far:", _seen["ratio"])
    assert (err <= bound).all(), (what, ratio)
    mean_m, _, mean_p, _ = M.NO_STATS if stats is None else stats
    slack_m = 0.0 if stats is None else 2.0 ** -23 * (np.abs(Mg[~exact]) + abs(mean_m))
    slack_p = 0.0 if stats is None else 2.0 ** -23 * (np.pi + abs(mean_p))
    assert (Mg[~exact] >= -slack_m).all() and (np.abs(Ph[~exact]) <= PI32 + slack_p).all(), what


def _hold_y(got, ref, what):
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), what


def _call(name, si, first, count, aug_kw, *, overlaps=3, partners=None, gains=None, occupancy=False, seed=3, epoch=0, index=None, rows=B,
          via_cursor=False, sides="xy"):
    """One call of gather_rows_mix and the reference of the same call: (out_x, out_y, reference, stats)."""
    H = pkg().hip_ops
    x, y, xd, yd, occ = _data(name, si, overlaps)
    stats = STATS[si]
    index = list(range(x.shape[0])) if index is None else index
    aug = H.Augment(device=DEV, **aug_kw)
    ox, oy = buffers(x.shape[1:], y.shape[1:], rows)
    idx = torch.as_tensor(index, dtype=torch.int64).to(DEV)
    kw = dict(epoch=_epoch(epoch), seed=seed, count=count, overlaps=overlaps, stats=_stats_tensor(stats))
    if partners is not None:
        kw.update(partners=torch.tensor(partners, dtype=torch.int64).to(DEV), gains=torch.tensor(np.asarray(gains, dtype=np.float32)).to(DEV))
    if occupancy:
        kw.update(occupancy=torch.from_numpy(occ).to(DEV))
    if via_cursor:
        stride = 3
        kw.update(cursor=torch.tensor([first // stride], device=DEV, dtype=torch.int32), stride=stride, start=first % stride)
    else:
        kw.update(start=first)
    use_x, use_y = "x" in sides, "y" in sides
    H.gather_rows_mix(xd if use_x else None, yd if use_y else None, idx, ox if use_x else None, oy if use_y else None, augment=aug, **kw)
    ref = M.gather_mix(x if use_x else None, y if use_y else None, np.asarray(index), first, count,
                       np.full((rows,) + x.shape[1:], SENTINEL, np.float32) if use_x else None,
                       np.full((rows,) + y.shape[1:], SENTINEL, np.float32) if use_y else None, seed=seed, epoch=epoch, overlaps=overlaps,
                       stats=stats, p_mix=aug_kw.get("p_mix", 0.0), mix_gain=aug_kw.get("mix_gain", (0.5, 1.0)), partners=partners, gains=gains,
                       occ=occ if occupancy else None, n_fmask=aug_kw.get("freq_masks", 0), f_max=aug_kw.get("freq_width", 0),
                       n_tmask=aug_kw.get("time_masks", 0), t_max=aug_kw.get("time_width", 0), fill=aug_kw.get("fill", 0.0))
    return ox, oy, ref, stats


def _explicit(index, first, count, n):
    """Partner positions and gains of a call: the sample of row r takes the position of row r + 1 (loader_mix_ref.explicit_pairs,
    whose bins at f = 0 are engineered for it) where `index` holds that row, else -1; samples of invalid rows get position 0."""
    where = {r: p for p, r in enumerate(index) if 0 <= r < n}
    pairs = M.explicit_pairs(n)
    partners, gains = [], []
    for b in range(count):
        p = first + b
        r = index[p] if p < len(index) else -1
        if 0 <= r < n:
            partners.append(where.get(pairs[r][0], -1))
            gains.append(pairs[r][1])
        else:
            partners.append(0)
            gains.append(1.0)
    return partners, gains


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(STATS)))
@pytest.mark.parametrize("name", list(CASES))
def test_explicit_partners_and_gains(name, si):
    """Every sample with its engineered partner and gain, O = 3 and O = 2, no occupancy table (an overflowing cell is cut as
    the reference cuts it); through `start` and through the cursor, count below B, an invalid index and a position past the
    index in between, a partner position of -1; the last call with masks of fill -1.5 over mixed values."""
    n = CASES[name][0][0]
    index = [n - 1, -1, 0, 2, 1, n, 3, 1]
    cut = False
    for overlaps in (3, 2):
        for i, (first, count) in enumerate(((0, 3), (2, 4), (5, 4))):
            masks = dict(freq_masks=1, freq_width=2, time_masks=2, time_width=3, fill=-1.5) if i == 2 else {}
            partners, gains = _explicit(index, first, count, n)
            ox, oy, ref, stats = _call(name, si, first, count, masks, overlaps=overlaps, partners=partners, gains=gains, index=index,
                                       via_cursor=i == 1)
            _hold_x(ox, ref["x"], stats, (name, si, overlaps, first))
            _hold_y(oy, ref["y"], (name, si, overlaps, first))
            invalid = [b for b, d in enumerate(ref["rows"]) if d is None]
            assert invalid and all(not ox[b].any() and not oy[b].any() for b in invalid)
            assert bool((ox[count:] == SENTINEL).all()) and bool((oy[count:] == SENTINEL).all())
            assert not ref["x"]["exact"][:count].all()                      # something was mixed and left unmasked
            if i == 2:
                assert bool((ox[:count] == -1.5).any()) and bool((ref["x"]["ref"][:count] == -1.5).any())
            y = _data(name, si, overlaps)[1]
            for b, d in enumerate(ref["rows"]):
                if d is not None and d["mixed"]:
                    both = M.active(y[index[first + b]], overlaps).sum(-1) + M.active(y[d["r2"]], overlaps).sum(-1)
                    cut = cut or bool((both > overlaps).any())
                    assert (M.active(oy[b].cpu().numpy(), overlaps).sum(-1) == np.minimum(both, overlaps)).all()
    assert cut                                                              # the truncation was exercised


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(STATS)))
@pytest.mark.parametrize("name", list(CASES))
def test_drawn_mixes_over_two_epochs_with_occupancy(name, si):
    """p_mix = 0.6 over 12 positions and two epochs (loader_mix_ref.DRAWN), through `start` and through the cursor, count below
    the buffer's rows, O = 3 and O = 2: partners, gains and the decisions of the occupancy test are the reference's (mixed
    positions within the bound, everything else and every target as bits); no cell loses an event; the epochs differ."""
    n = CASES[name][0][0]
    D = M.DRAWN
    index = [p % n for p in range(D["positions"])]
    for overlaps in (3, 2):
        seen = []
        for epoch in D["epochs"]:
            first, count = (1, 11) if epoch else (0, 12)
            ox, oy, ref, stats = _call(name, si, first, count, dict(p_mix=D["p_mix"], mix_gain=D["mix_gain"]), overlaps=overlaps,
                                       occupancy=True, seed=D["seed"], epoch=epoch, index=index, rows=12, via_cursor=bool(epoch))
            _hold_x(ox, ref["x"], stats, (name, si, overlaps, "epoch", epoch))
            _hold_y(oy, ref["y"], (name, si, overlaps, "epoch", epoch))
            assert ref["rows"] == M.drawn_rows(n, overlaps, epoch)[first:first + count]
            flags = [d["mixed"] for d in ref["rows"]]
            assert 0 < sum(flags) < len(flags)
            x, y, xd = _data(name, si, overlaps)[:3]
            for b, d in enumerate(ref["rows"]):
                assert torch.equal(_bits(ox[b]), _bits(xd[index[first + b]])) == (not d["mixed"])
                if d["mixed"]:                                              # with the table nothing is ever dropped
                    both = M.active(y[index[first + b]], overlaps).sum(-1) + M.active(y[d["r2"]], overlaps).sum(-1)
                    assert both.max() <= overlaps and (M.active(oy[b].cpu().numpy(), overlaps).sum(-1) == both).all()
            seen.append(flags[1:] if not epoch else flags)
        assert seen[0] != seen[1]


def test_the_result_does_not_depend_on_the_batch_the_count_or_the_form_of_the_call():
    name, si = "tiles_8x33x68", 1
    n = CASES[name][0][0]
    index = [p % n for p in range(12)]
    aug = dict(p_mix=0.7, freq_masks=1, freq_width=5, time_masks=1, time_width=9, fill=0.25)
    kw = dict(occupancy=True, seed=17, epoch=3, index=index)
    whole_x, whole_y, ref, _ = _call(name, si, 0, 12, aug, rows=12, **kw)
    assert any(d["mixed"] for d in ref["rows"][4:7])
    for first, count, rows, via_cursor in ((4, 3, 5, True), (4, 3, 3, False), (6, 1, 2, True)):
        ox, oy, _, _ = _call(name, si, first, count, aug, rows=rows, via_cursor=via_cursor, **kw)
        assert torch.equal(_bits(ox[:count]), _bits(whole_x[first:first + count])), (first, count, rows)
        assert torch.equal(_bits(oy[:count]), _bits(whole_y[first:first + count])), (first, count, rows)
        assert bool((ox[count:] == SENTINEL).all()) and bool((oy[count:] == SENTINEL).all())


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_edge_cases_leave_the_sample_as_it_is():
    """n_index == 1 at p_mix = 1 draws nothing; a partner whose index is invalid, a partner position of -1 and one past the
    index mix nothing: the rows move as bits."""
    H = pkg().hip_ops
    name, si = "vector_8x5x12", 1
    x, y, xd, yd, occ = _data(name, si)
    ox, oy, ref, _ = _call(name, si, 0, 1, dict(p_mix=1.0), index=[2], rows=2)
    assert ref["rows"] == [dict(p2=-1, g=np.float32(0), r2=-1, refused=False, mixed=False)]
    assert torch.equal(_bits(ox[0]), _bits(xd[2])) and torch.equal(_bits(oy[0]), _bits(yd[2])) and bool((ox[1] == SENTINEL).all())
    index = [0, -1, 1, 3, 99]
    ox, oy, ref, _ = _call(name, si, 0, 4, {}, index=index, partners=[1, 0, -1, 5], gains=[1.0, 1.0, 1.0, 1.0])
    assert [d and d["mixed"] for d in ref["rows"]] == [False, None, False, False]
    for b, r in ((0, 0), (2, 1), (3, 3)):
        assert torch.equal(_bits(ox[b]), _bits(xd[r])) and torch.equal(_bits(oy[b]), _bits(yd[r]))
    assert not ox[1].any() and not oy[1].any()
    ox, oy, ref, _ = _call(name, si, 0, 4, {}, index=index, partners=[4, 0, 0, 2], gains=[1.0, 1.0, 0.5, 2.0])      # 4: index 99
    assert [d and d["mixed"] for d in ref["rows"]] == [False, None, True, True]
    _hold_x(ox, ref["x"], STATS[si], "valid partners beside invalid ones")
    _hold_y(oy, ref["y"], "valid partners beside invalid ones")


def test_one_pair_alone():
    """The x pair only and the y pair only give what the call with both gives: both sides take the same decisions."""
    name, si = "vector_8x5x12", 1
    n = CASES[name][0][0]
    index = [p % n for p in range(12)]
    aug = dict(p_mix=0.7)
    kw = dict(occupancy=True, seed=5, epoch=1, index=index, rows=12)
    bx, by, ref, _ = _call(name, si, 0, 12, dict(aug, freq_masks=1, freq_width=2), **kw)
    assert any(d["mixed"] for d in ref["rows"]) and any(d["refused"] for d in ref["rows"])
    ox, _, _, _ = _call(name, si, 0, 12, dict(aug, freq_masks=1, freq_width=2), sides="x", **kw)
    _, oy, _, _ = _call(name, si, 0, 12, aug, sides="y", **kw)       # targets alone have the geometry (2, 1, 1): no room for a mask
    assert torch.equal(_bits(ox), _bits(bx)) and torch.equal(_bits(oy), _bits(by))


def test_two_calls_give_the_same_bytes():
    name, si = "tiles_8x33x68", 2
    aug = dict(p_mix=1.0, freq_masks=2, freq_width=9, time_masks=2, time_width=20, fill=-1.5)
    ax, ay, ref, stats = _call(name, si, 0, 4, aug, seed=12, epoch=2)
    bx, by, _, _ = _call(name, si, 0, 4, aug, seed=12, epoch=2)
    assert all(d["mixed"] for d in ref["rows"])
    assert torch.equal(_bits(ax), _bits(bx)) and torch.equal(_bits(ay), _bits(by))
    _hold_x(ax, ref["x"], stats, "masks")
    masked = ref["x"]["exact"][:, 0]
    assert masked.any() and not masked.all()
    assert bool((ax.cpu().numpy().transpose(0, 2, 3, 1)[masked] == -1.5).all())


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_target_occupancy_is_the_reference_bit_for_bit():
    H = pkg().hip_ops
    rng = np.random.default_rng(8)
    arrays = [(M.targets(n, o), o) for n in (5, 6, 7) for o in (2, 3)]
    for n, t_out, classes, o in ((70, 5, 14, 3), (3, 2, 64, 8), (9, 4, 1, 1)):
        n_sed = classes * o
        y = rng.standard_normal((n, t_out, 4 * n_sed)).astype(np.float32)
        y[..., :n_sed] = rng.choice(np.array([0, 1, 0.5, 0.75, np.nan, -1, np.inf], dtype=np.float32), (n, t_out, n_sed))
        arrays.append((y, o))
    for y, o in arrays:
        got = H.target_occupancy(torch.tensor(y).to(DEV), o)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), M.occupancy(y, o)), (y.shape, o)


def test_c_abi_refusals_launch_nothing():
    H, L = pkg().hip_ops, pkg()._lib
    x, y, xd, yd, occ = _data("vector_8x5x12", 1)
    n, C, F, T = x.shape
    ox, oy = buffers(x.shape[1:], y.shape[1:], B)
    idx = torch.arange(n, device=DEV)
    ep = _epoch(0)
    st = _stats_tensor(STATS[1])
    partners, gains = torch.tensor([1, 2, 3, 0], device=DEV), torch.ones(B, device=DEV)
    occ_d = torch.from_numpy(occ).to(DEV)
    lib, s = L.lib(), L.current_stream()
    good = dict(x_all=L.ptr(xd), row_x=C * F * T, out_x=L.ptr(ox), y_all=L.ptr(yd), row_y=3 * 24, out_y=L.ptr(oy), index=L.ptr(idx),
                n_index=n, n_rows=n, cursor=None, stride=B, start=0, B=B, count=B, C=C, F=F, T=T, y_cols=24, epoch=L.ptr(ep),
                seed=1, overlaps=3, stats=L.ptr(st), p_mix=0.5, gain_lo=0.5, gain_hi=1.0, partners=L.ptr(partners), gains=L.ptr(gains),
                occupancy=L.ptr(occ_d), n_fmask=1, f_max=F, n_tmask=1, t_max=T, fill=0.0)
    inf, nan = float("inf"), float("nan")
    bad = [dict(overlaps=0), dict(overlaps=-1), dict(overlaps=4), dict(overlaps=5), dict(p_mix=1.5), dict(p_mix=-0.5), dict(p_mix=nan),
           dict(gain_lo=0.0), dict(gain_lo=-1.0), dict(gain_lo=2.0), dict(gain_hi=inf), dict(gain_lo=nan), dict(gain_hi=nan),
           dict(partners=None), dict(gains=None), dict(epoch=None), dict(count=B + 1), dict(C=7, row_x=7 * F * T), dict(C=17, row_x=17 * F * T),
           dict(C=0), dict(F=0), dict(T=-1), dict(row_x=C * F * T + 4), dict(y_cols=0), dict(y_cols=6), dict(y_cols=8), dict(y_cols=16),
           dict(y_all=None, out_y=None, y_cols=16), dict(n_fmask=3), dict(n_tmask=-1), dict(f_max=F + 1), dict(t_max=-1),
           dict(n_index=2 ** 32 + 1), dict(count=0), dict(index=None), dict(out_x=None), dict(stride=-1, cursor=L.ptr(ep))]
    for change in bad:
        assert lib.seld_gather_rows_mix(*dict(good, **change).values(), s) == -1, change
    big = torch.zeros(1, 1, 4 * 65, device=DEV)
    unsupported = [dict(overlaps=12, y_all=L.ptr(big), out_y=L.ptr(big), row_y=4 * 60, y_cols=4 * 60, n_rows=1, occupancy=None),
                   dict(overlaps=1, y_all=L.ptr(big), out_y=L.ptr(big), row_y=4 * 65, y_cols=4 * 65, n_rows=1, occupancy=None)]
    for change in unsupported:
        assert lib.seld_gather_rows_mix(*dict(good, **change).values(), s) == -4, change
    occ_out = torch.full((n, 2), 200, device=DEV, dtype=torch.uint8)
    occ_good = dict(y_all=L.ptr(yd), n_rows=n, row_y=3 * 24, y_cols=24, overlaps=3, occ=L.ptr(occ_out))
    for change in (dict(y_all=None), dict(occ=None), dict(n_rows=0), dict(row_y=0), dict(y_cols=0), dict(overlaps=0), dict(overlaps=4),
                   dict(y_cols=20), dict(row_y=3 * 24 + 4)):
        assert lib.seld_target_occupancy(*dict(occ_good, **change).values(), s) == -1, change
    for change in (dict(y_all=L.ptr(big), n_rows=1, row_y=4 * 65, y_cols=4 * 65, overlaps=1), dict(y_cols=72, overlaps=9), dict(row_y=2 ** 31, y_cols=8, overlaps=2)):
        assert lib.seld_target_occupancy(*dict(occ_good, **change).values(), s) == -4, change
    torch.cuda.synchronize()
    assert bool((ox == SENTINEL).all()) and bool((oy == SENTINEL).all()) and bool((big == 0).all())     # nothing was launched
    assert bool((occ_out == 200).all())
    assert lib.seld_target_occupancy(*occ_good.values(), s) == 0
    assert lib.seld_gather_rows_mix(*good.values(), s) == 0
    assert lib.seld_gather_rows_mix(*dict(good, partners=None, gains=None, stats=None, occupancy=None).values(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(occ_out, occ_d)
    aug = H.Augment(p_mix=0.5, device=DEV)
    call = lambda **kw: H.gather_rows_mix(**dict(dict(x_all=xd, y_all=yd, index=idx, out_x=ox, out_y=oy, epoch=ep, seed=1, augment=aug,
                                                      overlaps=3), **kw))
    for kw in (dict(augment=None), dict(overlaps=0), dict(overlaps=9), dict(overlaps=4), dict(partners=partners), dict(gains=gains),
               dict(partners=partners[:2], gains=gains), dict(partners=partners.int(), gains=gains), dict(partners=partners.cpu(), gains=gains),
               dict(partners=partners, gains=gains.double()), dict(occupancy=occ_d[:3]), dict(occupancy=occ_d.int()), dict(occupancy=occ_d.cpu()),
               dict(occupancy=torch.zeros(n, 3, device=DEV, dtype=torch.uint8)), dict(stats=st.cpu()), dict(stats=st[:3]),
               dict(stats=torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV)), dict(epoch=ep.to(torch.int64)),
               dict(x_all=xd[:, :7].contiguous(), out_x=ox[:, :7].contiguous()), dict(x_all=xd.reshape(n, -1), out_x=ox.reshape(B, -1))):
        with pytest.raises(L.SeldHipError):
            call(**kw)
    for kw in (dict(y_all=yd.cpu()), dict(y_all=yd, overlaps=0), dict(y_all=yd, overlaps=4), dict(y_all=yd.double())):
        with pytest.raises(L.SeldHipError):
            H.target_occupancy(kw["y_all"], kw.get("overlaps", 3))
    call(stats=st, partners=partners, gains=gains, occupancy=occ_d)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_resident_loader_routes_mix_augments_and_a_recorded_fetch_equals_the_eager_ones():
    """ResidentLoader with kind 'mix' fetches with gather_rows_mix and its own occupancy table; a fetch recorded in a
    torch.cuda.graph and replayed for two batches in each of two epochs equals the eager gathers bit for bit."""
    H, T = pkg().hip_ops, pkg().train
    name, si = "vector_8x5x12", 1
    x, y, xd, yd, occ = _data(name, si)
    st = _stats_tensor(STATS[si])
    aug = H.Augment(p_mix=0.7, freq_masks=1, freq_width=2, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        T.ResidentLoader(xd, yd, 3, False, augment=aug, seed=4, polar_stats=st)
    loader = T.ResidentLoader(xd, yd, 3, False, augment=aug, seed=4, polar_stats=st, overlaps=3)
    assert loader.occupancy.dtype == torch.uint8 and np.array_equal(loader.occupancy.cpu().numpy(), occ)
    plain = T.ResidentLoader(xd, yd, 3, False, augment=H.Augment(freq_masks=1, freq_width=2, device=DEV), overlaps=3)
    assert plain.occupancy is None
    timer = H.kernel_timer
    was = timer.active, timer.only
    try:
        timer.active, timer.only = True, None
        for ld, label in ((loader, "gather_rows_mix_kernel"), (plain, "gather_rows_aug_kernel")):
            timer.reset()
            ld.fetch()
            ld.fetch(1, batch=2)
            torch.cuda.synchronize()
            assert [r[0] for r in timer.records] == [label, label]
    finally:
        timer.active, timer.only = was
        timer.reset()
    loss = torch.ones((), device=DEV)
    loader.step_end(loss)
    torch.cuda.synchronize()
    loader.cursor.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loader.fetch()
        loader.step_end(loss)
    assert int(loader.epoch) == -1 and int(loader.cursor) == 0  # recording ran nothing
    idx = torch.arange(x.shape[0], device=DEV)
    seen, mixed = [], 0
    for epoch in range(2):
        loader.begin_epoch()
        for i in range(2):
            graph.replay()
            ex, ey = torch.zeros_like(loader.x), torch.zeros_like(loader.target)
            H.gather_rows_mix(xd, yd, idx, ex, ey, epoch=_epoch(epoch), seed=4, augment=aug, overlaps=3, stats=st, occupancy=loader.occupancy,
                              start=3 * i)
            assert torch.equal(_bits(loader.x), _bits(ex)) and torch.equal(_bits(loader.target), _bits(ey)), (epoch, i)
            ref = M.gather_mix(x, y, np.arange(x.shape[0]), 3 * i, 3, np.zeros((3,) + x.shape[1:], np.float32), np.zeros((3,) + y.shape[1:], np.float32),
                               seed=4, epoch=epoch, overlaps=3, stats=STATS[si], p_mix=0.7, occ=occ, n_fmask=1, f_max=2)
            _hold_x(loader.x, ref["x"], STATS[si], ("loader", epoch, i))
            _hold_y(loader.target, ref["y"], ("loader", epoch, i))
            mixed += sum(d["mixed"] for d in ref["rows"])
            seen.append(loader.x.clone())
        assert int(loader.cursor) == 2 and int(loader.epoch) == epoch
    assert mixed and not torch.equal(seen[0], seen[2])


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_graphed_train_step_on_mixed_batches_reproduces_the_eager_losses(seld_env):
    """GraphedTrainStep(loader=...) on the tiny DQ model with 16 input channels (two microphones, magnitude and phase),
    standardised predictors with polar_stats, the Augment of --augment_mix plus masks: three replays against three eager
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
    aug = H.Augment(p_mix=0.8, freq_masks=2, freq_width=16, time_masks=1, time_width=10, device=DEV)

    def fresh():
        H.philox.set_offset(0)
        H.hcq_weights.reset()
        model = build_model(case).to(DEV).train()
        return model, T.FlatAdam(model.parameters(), lr=1e-3), T.ResidentLoader(x, y, 2, False, augment=aug, seed=6, polar_stats=st, overlaps=3)

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
    assert any(not torch.equal(by_, y[2 * i:2 * i + 2]) for i, (_, by_) in enumerate(batches))      # some targets were merged


# ---- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalization", ["True", "False"])
def test_main_trains_on_mixed_magnitude_phase_batches(tmp_path, normalization):
    """train.main on 5 pickled two-microphone magnitude-phase samples (16 channels), --phase=True --resident_loader=True
    --graph_step=True --augment_mix=0.5, with and without dataset standardisation: one epoch of three steps (two replays
    and a partial eager batch) with finite losses, fetched by the mixing gather with the training array's statistics (none
    on raw data) and the occupancy table of the training targets."""
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
        if split == "training":
            want_occ = M.occupancy(np.concatenate([act, loc], axis=2), 3)
    paths["test_predictors_path"] = paths["test_target_path"] = str(tmp_path / "absent.pkl")
    flags = dict(MODEL_FLAGS, **paths, results_path=str(tmp_path / "res"), checkpoint_dir=str(tmp_path / "ck"), batch_size=2, epochs=1,
                 min_n_epochs=1, input_channels=16, phase="True", dataset_normalization=normalization, resident_loader="True",
                 graph_step="True", augment_mix=0.5, augment_time_masks=1, augment_time_width=8)
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    made = []
    real = T.ResidentLoader

    class Recording(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    calls = []
    real_gather = H.gather_rows_mix

    def counting(*a, **kw):
        calls.append((kw.get("stats"), kw.get("occupancy"), kw.get("overlaps")))
        return real_gather(*a, **kw)
    T.ResidentLoader, H.gather_rows_mix = Recording, counting
    try:
        history = []
        state = T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]), history=history)
        torch.cuda.synchronize()
    finally:
        T.ResidentLoader, H.gather_rows_mix = real, real_gather
    assert state["epochs"] == 1 and state["step"] == 3
    assert len(history) == 1 and all(np.isfinite(v) for v in history[0][1:])
    train = made[0]
    assert train.augment.kind == "mix" and train.augment.p_mix == 0.5 and train.augment.mix_gain == (0.5, 1.0) and train.overlaps == 3
    assert np.array_equal(train.occupancy.cpu().numpy(), want_occ)
    assert all(m.augment is None and m.polar_stats is None and m.occupancy is None for m in made[1:])      # validation sees the data as it is
    assert calls and all(c[0] is train.polar_stats and c[1] is train.occupancy and c[2] == 3 for c in calls)
    if normalization == "True":
        st = train.polar_stats.tolist()
        assert len(st) == 4 and st[1] > 0 and 1.5 < st[3] < 2.1 and abs(st[2]) < 0.1
    else:
        assert train.polar_stats is None
