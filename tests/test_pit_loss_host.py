"""The fp64 reference of the permutation-invariant loss (tests/pit_loss_ref.py) held to its own invariants, the input
generator's statistics the GPU test relies on, and the --pit_loss flag.  No GPU."""
import pytest
import torch

from tests import pit_loss_ref as R
from tests.helpers import pkg

SHAPES = [(1, 14, 3), (37, 14, 3), (64, 1, 3), (37, 14, 2)]


def _case(shape):
    rows, C, O = shape
    return R.pit_inputs(rows, C, O, seed=sum(shape))


def test_permutation_numbering():
    assert R.permutations(3) == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    assert R.permutations(2) == [(0, 1), (1, 0)] and R.permutations(1) == [(0,)]


@pytest.mark.parametrize("shape", SHAPES)
def test_one_slot_is_the_plain_loss(shape):
    """overlaps = 1 on the same data viewed as C * O classes: nothing to permute."""
    rows, C, O = shape
    sed, doa, tgt = _case(shape)
    ref = R.pit_reference(sed, doa, tgt, C * O, 1, 0.25, 3.0)
    loss, dsed, ddoa = R.plain_reference(sed, doa, tgt, 0.25, 3.0)
    assert abs(ref["loss"] - loss) <= 1e-12 * abs(loss)
    assert torch.equal(ref["dsed"], dsed) and torch.equal(ref["ddoa"], ddoa)
    assert not ref["perm"].any() and not ref["choice"].any()
    assert abs(sum(ref["parts"]) - loss) <= 1e-12 * abs(loss)


@pytest.mark.parametrize("shape", SHAPES)
def test_never_above_the_plain_loss_and_invariant_under_target_slot_permutations(shape):
    rows, C, O = shape
    sed, doa, tgt = _case(shape)
    ref = R.pit_reference(sed, doa, tgt, C, O)
    plain = R.plain_reference(sed, doa, tgt)[0]
    assert ref["loss"] <= plain * (1 + 1e-12)
    assert abs(sum(ref["parts"]) - ref["loss"]) <= 1e-12 * ref["loss"]
    order = R.random_orders(rows, C, O, torch.Generator().manual_seed(3))
    other = R.pit_reference(sed, doa, R.permute_target(tgt, C, O, order), C, O)
    assert abs(other["loss"] - ref["loss"]) <= 1e-12 * ref["loss"]
    keep = ~ref["ambiguous"]
    assert torch.equal(other["ambiguous"], ref["ambiguous"])
    for name, per in (("dsed", O), ("ddoa", 3 * O)):
        m = keep[..., None].expand(rows, C, per).reshape(rows, -1)
        assert torch.allclose(other[name][m], ref[name][m], rtol=1e-12, atol=0), name


@pytest.mark.parametrize("shape", SHAPES + [(4700, 14, 3)])
def test_generator_statistics(shape):
    """What tests/test_gpu_pit_loss.py asserts of the reference, checked without a GPU as well: no ambiguous cell at the
    small shapes (at most 0.1 % of the cells with a choice at the large one), and a target other than the given one wins
    in at least 20 % of the cells that have a choice."""
    rows, C, O = shape
    ref = R.pit_reference(*_case(shape), C, O)
    choice = int(ref["choice"].sum())
    ambiguous = int(ref["ambiguous"].sum())
    assert ambiguous <= (1e-3 * choice if rows == 4700 else 0), (ambiguous, choice)
    assert choice > 0 and int((ref["moved"] & ref["choice"]).sum()) >= 0.2 * choice


def test_a_two_track_swap_picks_index_2():
    """Two events of one class predicted in each other's slots, the third slot silent: permutation 2 = (1, 0, 2)."""
    a, b = [0.5, -0.25, 0.75], [-0.5, 0.125, 0.25]
    sed = torch.tensor([[0.9, 0.8, 0.1]])
    doa = torch.tensor([b + a + [0.0, 0.0, 0.0]])
    tgt = torch.tensor([[1.0, 1.0, 0.0] + a + b + [0.0, 0.0, 0.0]])
    ref = R.pit_reference(sed, doa, tgt, 1, 3)
    assert ref["perm"].tolist() == [[2]] and ref["moved"].all() and not ref["ambiguous"].any()
    assert ref["loss"] < R.plain_reference(sed, doa, tgt)[0]
    assert torch.equal(ref["ddoa"], torch.zeros(1, 9, dtype=torch.float64))


def test_pit_loss_flag():
    T = pkg().train
    assert T.parse_args(["--TextArgs=none", "--pit_loss=True"]).pit_loss is True
    assert T.parse_args(["--TextArgs=none"]).pit_loss is False


def test_more_than_three_slots_are_refused_before_any_gpu_work():
    T = pkg().train
    with pytest.raises(ValueError, match="at most 3 slots"):
        T.main(T.parse_args(["--TextArgs=none", "--pit_loss=True", "--class_overlaps=4"]))
