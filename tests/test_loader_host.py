"""Host side of the device-resident epoch loader: the sample order (hip_ops.epoch_permutation against torch's
RandomSampler) and the index arithmetic of an epoch (train.epoch_plan).  No GPU."""
import pytest
import torch
from torch.utils.data import RandomSampler

from tests.helpers import pkg


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_epoch_permutation_is_random_samplers_order(n):
    """Two consecutive epochs (each draws a fresh seed from the default generator) from the same torch.manual_seed: the
    same orders as RandomSampler's, and the default generator ends in the same state."""
    H = pkg().hip_ops
    torch.manual_seed(7)
    sampler = RandomSampler(range(n))
    ref = [list(sampler), list(sampler)]
    ref_state = torch.get_rng_state()
    torch.manual_seed(7)
    got = [H.epoch_permutation(n), H.epoch_permutation(n)]
    assert all(g.dtype == torch.int64 and not g.is_cuda for g in got)
    assert [g.tolist() for g in got] == ref
    assert torch.equal(torch.get_rng_state(), ref_state)


def test_epoch_permutation_with_a_generator_leaves_the_default_one_alone():
    H = pkg().hip_ops
    torch.manual_seed(3)
    before = torch.get_rng_state()
    got = H.epoch_permutation(9, generator=torch.Generator().manual_seed(11))
    assert got.tolist() == list(RandomSampler(range(9), generator=torch.Generator().manual_seed(11)))
    assert torch.equal(torch.get_rng_state(), before)


def _covered(T, plan, world):
    rows = []
    for start, count, _ in plan:
        ranges = [T.rank_rows(start, count, r) for r in range(world)]
        assert ranges[0][0] == start
        for (_, hi), (lo, _) in zip(ranges[:-1], ranges[1:]):
            assert hi == lo                              # disjoint, adjacent: together [start, start + world * count)
        assert all(hi - lo == count for lo, hi in ranges)
        rows += list(range(start, ranges[-1][1]))
    return rows


def test_epoch_plan_single_process_with_partial_batch():
    T = pkg().train
    plan = T.epoch_plan(5, 2, 1)
    assert plan == [(0, 2, True), (2, 2, True), (4, 1, False)]
    assert _covered(T, plan, 1) == list(range(5)) and T.epoch_left_out(5, 2, 1) == 0


def test_epoch_plan_two_ranks_cut_the_last_batch():
    T = pkg().train
    plan = T.epoch_plan(11, 4, 2)
    assert plan == [(0, 2, True), (4, 2, True), (8, 1, False)]          # the last global batch: 3 samples cut to 2
    assert _covered(T, plan, 2) == list(range(10)) and T.epoch_left_out(11, 4, 2) == 1
    assert T.rank_rows(4, 2, 0) == (4, 6) and T.rank_rows(4, 2, 1) == (6, 8) and T.rank_rows(8, 1, 1) == (9, 10)


def test_epoch_plan_without_remainder():
    T = pkg().train
    plan = T.epoch_plan(8, 4, 2)
    assert plan == [(0, 2, True), (4, 2, True)]
    assert _covered(T, plan, 2) == list(range(8)) and T.epoch_left_out(8, 4, 2) == 0


def test_epoch_plan_drops_a_batch_cut_to_nothing_and_handles_short_arrays():
    T = pkg().train
    assert T.epoch_plan(9, 4, 2) == [(0, 2, True), (4, 2, True)] and T.epoch_left_out(9, 4, 2) == 1
    assert T.epoch_plan(3, 4, 1) == [(0, 3, False)]
    assert T.epoch_plan(3, 4, 2) == [(0, 1, False)] and T.epoch_left_out(3, 4, 2) == 1


def test_epoch_plan_refuses_a_batch_the_ranks_cannot_share():
    T = pkg().train
    with pytest.raises(ValueError, match="not divisible"):
        T.epoch_plan(8, 5, 2)
    with pytest.raises(ValueError):
        T.epoch_plan(0, 2, 1)


def test_new_flags_default_to_off_and_parse_like_the_other_switches():
    T = pkg().train
    off = T.parse_args(["--TextArgs=none"])
    assert off.resident_loader is False and off.graph_step is False
    on = T.parse_args(["--TextArgs=none", "--resident_loader=True", "--graph_step=True"])
    assert on.resident_loader is True and on.graph_step is True


def test_recorded_step_refuses_an_exchange_it_could_not_replay(monkeypatch):
    """A sync over two ranks without the front-end cut (built without `model=`, or over a FlatAdam built without `late=`)
    would be recorded as one graph and replayed with no collective: refused first, before the device is touched.  The
    same for a sync that states its ranks only through average_scale() (dp.FlatGradSync has no `world`); a sync that states
    neither is an error, never taken for one rank."""
    import types
    T = pkg().train
    model = torch.nn.Linear(4, 3)
    opt = T.FlatAdam(model.parameters(), lr=1e-3)
    monkeypatch.setattr(torch.cuda, "_lazy_init", lambda *a, **k: pytest.fail("the device was touched"))
    call = lambda sync: T.GraphedTrainStep(model, opt, torch.zeros(2, 4), torch.zeros(2, 3), 3, sync=sync)     # noqa: E731
    with pytest.raises(ValueError, match="late"):
        call(types.SimpleNamespace(world=2, cut=None))
    with pytest.raises(ValueError, match="late"):
        call(types.SimpleNamespace(cut=None, average_scale=lambda: 0.5, all_reduce=lambda: None))
    with pytest.raises(AttributeError):
        call(types.SimpleNamespace(cut=None))
