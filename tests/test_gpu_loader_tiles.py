"""The row walkers and the launch plan of the loader gathers (csrc/loader.hip) past their first tile: predictor rows of more
than one tile of either kind, grids at their cap so that a workgroup strides over several tiles, and the masks-only path
of the three augmenting kernels against each other.  References and bounds are those of the neighbouring tests:
tests/loader_rot_ref.py at 4 * 2^-24 (explicit matrices) and 8 * 2^-24 (drawn rotations), tests/loader_polar_ref.py at its K,
tests/loader_aug_ref.py and everything a kernel only moves as bits.

A tile of the rotating gathers holds 512 triple items, 256 group items or 1024 pass items of 16 bytes (4 bytes on the scalar
path); P is the number of items per channel."""
import functools

import numpy as np
import pytest
import torch

from tests import loader_aug_ref as A
from tests import loader_polar_ref as P
from tests import loader_rot_ref as R
from tests.helpers import pkg
from tests.loader_helpers import DEV, SENTINEL, bits, buffers, epoch, hold_polar, hold_rot, shifted

pytestmark = pytest.mark.gpu
N_ROWS = 7
INDEX = [3, -1, 0, 4, 2, N_ROWS, 1, 1, 3]
TARGET = (5, 42)                                                    # (T_out, n_sed)
Y_SHAPE = (TARGET[0], 4 * TARGET[1])
MASKS = dict(freq_masks=1, freq_width=6, time_masks=1, time_width=9, fill=0.25)
# (C, F, T), triples
ROT_CASES = {
    "two_triples_8x20x64": ((8, 20, 64), [(3, 1, 2), (7, 5, 6)]),   # P = 320: 640 triple items, the first tile straddles the triples
    "one_triple_8x20x64": ((8, 20, 64), [(3, 1, 2)]),               # one triple tile, then 1600 pass items: two tiles, the second partial
    "scalar_4x30x21": ((4, 30, 21), [(3, 1, 2)]),                   # T % 4 != 0, P = 630: two triple tiles, a partial pass tile
}
# (C, F, T), microphones of the layout; one group is rotated
POLAR_CASES = {
    "8x20x64": ((8, 20, 64), 1),                                    # 320 group items: two tiles of 256
    "16x20x64": ((16, 20, 64), 2),                                  # then 10 * 320 pass items: four pass tiles
    "scalar_8x30x21": ((8, 30, 21), 1),                             # T % 4 != 0: 630 group items, 1260 pass items
}


@functools.lru_cache(maxsize=None)
def _normal(shape, shift=0):
    """(x, y, x on the device `shift` floats off alignment, y on the device): N_ROWS rows of standard normal values."""
    rng = np.random.default_rng(sum(shape) + shift)
    x = rng.standard_normal((N_ROWS,) + shape).astype(np.float32)
    x[:, :, 0, 0] = -0.0                                            # a signed zero must pass as it is
    y = rng.standard_normal((N_ROWS,) + Y_SHAPE).astype(np.float32)
    xd, yd = shifted(x, shift), torch.from_numpy(y).to(DEV)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, xd, yd


@functools.lru_cache(maxsize=None)
def _polar(name, si):
    """(x, y, the first group, x on the device, y on the device) of a polar case with the statistics STATS[si]."""
    shape, mics = POLAR_CASES[name]
    x, y, groups = P.make_inputs((N_ROWS,) + shape, mics, si)
    return x, y, groups[:1], torch.tensor(x).to(DEV), torch.tensor(y).to(DEV)


def _stats_tensor(stats):
    return None if stats is None else torch.tensor(stats, device=DEV, dtype=torch.float32)


def _ref_kw(aug_kw):
    return dict(n_fmask=aug_kw.get("freq_masks", 0), f_max=aug_kw.get("freq_width", 0), n_tmask=aug_kw.get("time_masks", 0),
                t_max=aug_kw.get("time_width", 0), fill=aug_kw.get("fill", 0.0))


def _rot_kw(aug_kw):
    return dict(p_rot=aug_kw.get("p_rot", 0.0), rot_mirror=aug_kw.get("rot_mirror", True), rot_zflip=aug_kw.get("rot_zflip", True))


def _mixed(rows):
    """Rotated and unrotated valid samples and invalid rows are all in the batch."""
    flags = [d["rotate"] for d in rows if d is not None]
    return any(flags) and not all(flags) and any(d is None for d in rows)


# ---- 1, 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROT_CASES))
def test_rot_rows_of_several_triple_and_pass_tiles(name):
    """p_rot = 0.5 with one frequency and one time mask over INDEX (invalid entries included), count below the buffer's rows:
    rotated samples walk triple tiles and then pass tiles, unrotated ones pass tiles only (2560 items at (8, 20, 64): three
    tiles, the last half full).  Drawn rotations within 8 * 2^-24 * sum_j |v_j|, the same rows under explicit matrices
    within 4 * 2^-24 * S, everything else as bits."""
    H = pkg().hip_ops
    shape, triples = ROT_CASES[name]
    x, y, xd, yd = _normal(shape)
    idx = torch.tensor(INDEX, device=DEV)
    count, rows = len(INDEX), len(INDEX) + 1
    init = np.full((rows,) + shape, SENTINEL, np.float32), np.full((rows,) + Y_SHAPE, SENTINEL, np.float32)
    aug_kw = dict(MASKS, p_rot=0.5)
    ox, oy = buffers(shape, Y_SHAPE, rows)
    H.gather_rows_rot(xd, yd, idx, ox, oy, epoch=epoch(1), seed=9, count=count,
                      augment=H.Augment(rot_triples=triples, device=DEV, **aug_kw))
    ref = R.gather_rot(x, y, np.asarray(INDEX), 0, count, *init, seed=9, epoch=1, triples=triples, **_rot_kw(aug_kw), **_ref_kw(aug_kw))
    assert _mixed(ref["rows"])
    hold_rot(ox, ref["x"], 8, "plain", (name, "x"))
    hold_rot(oy, ref["y"], 8, "plain", (name, "y"))
    assert bool((ox[count:] == SENTINEL).all()) and bool((oy[count:] == SENTINEL).all())
    assert bool((ox[:count] == 0.25).any()) and not ref["x"]["exact"][:count].all()

    rng = np.random.default_rng(len(name))
    mats = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(count)]).reshape(count, 9).astype(np.float32)
    ox, oy = buffers(shape, Y_SHAPE, rows)
    H.gather_rows_rot(xd, yd, idx, ox, oy, epoch=epoch(1), seed=9, count=count, matrices=torch.from_numpy(mats).to(DEV),
                      augment=H.Augment(rot_triples=triples, device=DEV, **MASKS))
    ref = R.gather_rot(x, y, np.asarray(INDEX), 0, count, *init, seed=9, epoch=1, triples=triples, matrices=mats, **_ref_kw(MASKS))
    hold_rot(ox, ref["x"], 4, "weight", (name, "x", "matrices"))
    hold_rot(oy, ref["y"], 4, "weight", (name, "y", "matrices"))
    assert bool((ox[count:] == SENTINEL).all()) and bool((oy[count:] == SENTINEL).all())


# ---- 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [0, 1])
@pytest.mark.parametrize("name", list(POLAR_CASES))
def test_polar_rows_of_several_group_and_pass_tiles(name, si):
    """The same call on magnitude-phase predictors with ONE group, raw and standardised: group tiles of 256 items, then the
    pass tiles of the channels outside the group.  Rotated positions within the bound of tests/test_gpu_loader_polar.py, the
    rest as bits."""
    H = pkg().hip_ops
    x, y, groups, xd, yd = _polar(name, si)
    stats = P.STATS[si]
    idx = torch.tensor(INDEX, device=DEV)
    count, rows = len(INDEX), len(INDEX) + 1
    aug_kw = dict(MASKS, p_rot=0.5)
    ox, oy = buffers(x.shape[1:], y.shape[1:], rows)
    H.gather_rows_polar(xd, yd, idx, ox, oy, epoch=epoch(1), seed=9, count=count, stats=_stats_tensor(stats),
                        augment=H.Augment(rot_polar=groups, device=DEV, **aug_kw))
    ref = P.gather_polar(x, y, np.asarray(INDEX), 0, count, np.full((rows,) + x.shape[1:], SENTINEL, np.float32),
                         np.full((rows,) + y.shape[1:], SENTINEL, np.float32), seed=9, epoch=1, groups=groups, stats=stats,
                         **_rot_kw(aug_kw), **_ref_kw(aug_kw))
    assert _mixed(ref["rows"])
    hold_polar(ox, ref["x"], groups, stats, (name, si))
    assert P.bits_equal(oy.cpu().numpy(), ref["y"]["ref"])[ref["y"]["exact"]].all()
    hold_rot(oy, ref["y"], 8, "plain", (name, si, "y"))
    assert bool((ox[count:] == SENTINEL).all()) and bool((oy[count:] == SENTINEL).all())
    assert bool((ox[:count] == 0.25).any()) and not ref["x"]["exact"][:count].all()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
STRIDE_SHAPE = (8, 20, 64)
STRIDE_N, STRIDE_PART = 700, 100


def _stride_call(kind):
    """(gather(index, out_x, out_y, start, count), check(out_x, out_y) of the first STRIDE_PART positions) of one kernel."""
    H = pkg().hip_ops
    positions = np.random.default_rng(4).integers(0, N_ROWS, STRIDE_N)
    init = np.full((STRIDE_PART,) + STRIDE_SHAPE, SENTINEL, np.float32)
    kw = dict(epoch=epoch(2), seed=13)
    if kind == "polar":
        x, y, groups, xd, yd = _polar("8x20x64", 1)
        stats = P.STATS[1]
        aug_kw = dict(MASKS, p_rot=0.5)
        aug = H.Augment(rot_polar=groups, device=DEV, **aug_kw)
        st = _stats_tensor(stats)
        gather = lambda idx, ox, oy, start, count: H.gather_rows_polar(xd, yd, idx, ox, oy, augment=aug, stats=st, start=start,
                                                                       count=count, **kw)

        def check(ox, oy):
            ref = P.gather_polar(x, y, positions, 0, STRIDE_PART, init, np.full((STRIDE_PART,) + y.shape[1:], SENTINEL, np.float32),
                                 seed=13, epoch=2, groups=groups, stats=stats, **_rot_kw(aug_kw), **_ref_kw(aug_kw))
            flags = [d["rotate"] for d in ref["rows"]]
            assert any(flags) and not all(flags)
            hold_polar(ox, ref["x"], groups, stats, "stride polar")
            hold_rot(oy, ref["y"], 8, "plain", "stride polar y")
        return positions, y.shape[1:], gather, check
    x, y, xd, yd = _normal(STRIDE_SHAPE)
    init_y = np.full((STRIDE_PART,) + Y_SHAPE, SENTINEL, np.float32)
    if kind == "rot":
        triples = [(3, 1, 2), (7, 5, 6)]
        aug_kw = dict(MASKS, p_rot=0.5)
        aug = H.Augment(rot_triples=triples, device=DEV, **aug_kw)
        gather = lambda idx, ox, oy, start, count: H.gather_rows_rot(xd, yd, idx, ox, oy, augment=aug, start=start, count=count, **kw)

        def check(ox, oy):
            ref = R.gather_rot(x, y, positions, 0, STRIDE_PART, init, init_y, seed=13, epoch=2, triples=triples, **_rot_kw(aug_kw),
                               **_ref_kw(aug_kw))
            flags = [d["rotate"] for d in ref["rows"]]
            assert any(flags) and not all(flags)
            hold_rot(ox, ref["x"], 8, "plain", "stride rot x")
            hold_rot(oy, ref["y"], 8, "plain", "stride rot y")
        return positions, Y_SHAPE, gather, check
    table = H.foa_transforms(mics=2)
    aug_kw = dict(MASKS, p_swap=0.5)
    aug = H.Augment(table=table, device=DEV, **aug_kw)
    gather = lambda idx, ox, oy, start, count: H.gather_rows_aug(xd, yd, idx, ox, oy, augment=aug, start=start, count=count, **kw)

    def check(ox, oy):
        want_x, want_y = A.gather_aug(x, y, positions, 0, STRIDE_PART, init, init_y, seed=13, epoch=2, table=table, p_swap=0.5,
                                      **_ref_kw(aug_kw))
        assert torch.equal(ox.cpu(), torch.from_numpy(want_x)) and torch.equal(oy.cpu(), torch.from_numpy(want_y))
        assert not torch.equal(oy, yd[torch.from_numpy(positions[:STRIDE_PART]).to(DEV)])       # some sample was swapped
    return positions, Y_SHAPE, gather, check


@pytest.mark.parametrize("kind", ["aug", "rot", "polar"])
def test_a_grid_at_its_cap_strides_over_the_tiles(kind):
    """One launch of count = B = 700 (at most 2048 / 700 = 2 workgroups per predictor row against 3 tiles or more: every
    workgroup walks more than one) equals, bit for bit, the same 700 positions fetched as seven launches of count = 100
    (20 workgroups per row allowed: nothing strides); the draws are functions of the position.  The first small launch is
    held to the host reference."""
    positions, y_shape, gather, check = _stride_call(kind)
    idx = torch.from_numpy(positions).to(DEV)
    one_x, one_y = buffers(STRIDE_SHAPE, y_shape, STRIDE_N)
    gather(idx, one_x, one_y, 0, STRIDE_N)
    part_x, part_y = buffers(STRIDE_SHAPE, y_shape, STRIDE_N)
    for start in range(0, STRIDE_N, STRIDE_PART):
        gather(idx, part_x[start:start + STRIDE_PART], part_y[start:start + STRIDE_PART], start, STRIDE_PART)
    assert torch.equal(bits(one_x), bits(part_x)) and torch.equal(bits(one_y), bits(part_y))
    check(part_x[:STRIDE_PART], part_y[:STRIDE_PART])


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,shift", [((8, 20, 64), 0), ((16, 9, 7), 1)])
def test_masks_only_is_the_same_through_all_three_kernels(shape, shift):
    """No table, p_rot = 0, two frequency and two time masks: gather_rows_aug, gather_rows_rot and gather_rows_polar write the
    same bits, through the cursor, over INDEX with its invalid entries, rows >= count left alone."""
    H = pkg().hip_ops
    C, F, T = shape
    _, _, xd, yd = _normal(shape, shift)
    idx = torch.tensor(INDEX, device=DEV)
    masks = dict(freq_masks=2, freq_width=F, time_masks=2, time_width=T, fill=0.25)
    rows, count, stride = 6, 5, 3
    calls = ((H.gather_rows_aug, H.Augment(device=DEV, **masks)),
             (H.gather_rows_rot, H.Augment(rot_triples=[(3, 1, 2)], p_rot=0.0, device=DEV, **masks)),
             (H.gather_rows_polar, H.Augment(rot_polar=P.polar_groups(C // 8), p_rot=0.0, device=DEV, **masks)))
    for ep in (0, 3):
        got = []
        for gather, aug in calls:
            ox, oy = buffers(shape, Y_SHAPE, rows)
            gather(xd, yd, idx, ox, oy, epoch=epoch(ep), seed=5, augment=aug, cursor=torch.tensor([1], device=DEV, dtype=torch.int32),
                   stride=stride, start=1, count=count)
            got.append((ox, oy))
        (ax, ay), others = got[0], got[1:]
        for ox, oy in others:
            assert torch.equal(bits(ox), bits(ax)) and torch.equal(bits(oy), bits(ay)), ep
        invalid = [b for b in range(count) if not 0 <= INDEX[stride + 1 + b] < N_ROWS]
        assert invalid and all(not ax[b].any() and not ay[b].any() for b in invalid)
        assert bool((ax[count:] == SENTINEL).all()) and bool((ay[count:] == SENTINEL).all())
        assert bool((ax[:count] == 0.25).any())
