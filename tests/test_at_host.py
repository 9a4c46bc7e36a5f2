"""Temporal attention, the parts that need no device: the fp64 yardstick tests/at_ref.py against torch.autograd, the
conditions the case table must meet, the module's widths, the state-dict layout of models with the blocks on and off,
and the training flags with their refusals."""
import numpy as np
import pytest
import torch

from tests import at_ref as R
from tests.golden.cases import MODEL_CASES, model_kwargs
from tests.helpers import pkg

CASE = {c["name"]: c for c in MODEL_CASES}


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_at_ref_formulas_match_autograd(case):
    """read and the explicit dq | dk | dv of at_ref against autograd through its dense masked softmax, in fp64: 1e-12 of
    each tensor's largest entry (sums of at most 1040 terms of size O(1) round far below that)."""
    N, K, V, T, mask, W, lengths = case
    qkv, dread = R.make_case(case)
    f = R.at_forward(qkv, K, V, mask, W, lengths)
    dqkv = R.at_backward(qkv, dread, K, V, f["p"], f["read"])
    leaf = qkv.clone().requires_grad_(True)
    read = R.at_dense_autograd(leaf, K, V, mask, W, lengths)
    read.backward(dread)
    for name, got, want in (("read", f["read"], read.detach()), ("dq", dqkv[:, :K], leaf.grad[:, :K]),
                            ("dk", dqkv[:, K:2 * K], leaf.grad[:, K:2 * K]), ("dv", dqkv[:, 2 * K:], leaf.grad[:, 2 * K:])):
        assert got.shape == want.shape, name
        assert torch.isfinite(got).all(), name
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
    ok = R.allowed(N, T, mask, W, lengths)
    live = ok.any(dim=2)
    assert torch.equal(torch.isinf(f["lse"]), ~live)
    score = torch.einsum("ndt,nds->nts", qkv[:, :K], qkv[:, K:2 * K]) / K ** 0.5
    assert float((f["p"] - torch.exp(score - f["lse"].unsqueeze(2)))[ok].abs().max()) <= 1e-12     # lse is the log-sum-exp
    assert float((f["p"].sum(dim=2)[live] - 1.0).abs().max()) <= 1e-12
    assert float(f["p"][~ok].abs().max() if (~ok).any() else 0.0) == 0.0        # excluded keys weigh exactly 0


def test_table_has_rows_without_keys_and_they_give_zero():
    """At least one case has rows with no allowed key; those rows read zero and their dq is zero, and no key or value
    receives anything from them (dk, dv equal those of the same case with the rows' cotangent removed)."""
    found = 0
    for case in R.CASES:
        N, K, V, T, mask, W, lengths = case
        dead = ~R.allowed(N, T, mask, W, lengths).any(dim=2)
        if not dead.any():
            continue
        found += 1
        qkv, dread = R.make_case(case)
        f = R.at_forward(qkv, K, V, mask, W, lengths)
        g = R.at_backward(qkv, dread, K, V, f["p"], f["read"])
        sel = dead.unsqueeze(1)
        assert float(f["read"].masked_select(sel.expand_as(f["read"])).abs().max()) == 0.0
        assert float(g[:, :K].masked_select(sel.expand(N, K, T)).abs().max()) == 0.0
        g0 = R.at_backward(qkv, dread * (~sel), K, V, f["p"], f["read"])
        assert torch.equal(g0[:, K:], g[:, K:])
    assert found >= 1
    N, K, V, T, mask, W, lengths = R.CASES[8]
    dead = ~R.allowed(N, T, mask, W, lengths).any(dim=2)
    assert dead[1, 8:].all() and not dead[1, :8].any() and not dead[0].any()      # len 5, W 3: s <= 4 < t - 3


def test_table_has_a_fully_excluded_tile_on_each_side_of_the_band():
    """At least one band case has, for some 16-row query tile, a wholly excluded 16 x 16 tile in front of the band and one
    behind it (with allowed tiles between): the tiles a kernel must skip."""
    found = 0
    for case in R.CASES:
        N, K, V, T, mask, W, lengths = case
        if mask != "band" or T % 16:
            continue
        ok = R.allowed(N, T, mask, W, lengths)[0]
        tiles = ok.view(T // 16, 16, T // 16, 16).permute(0, 2, 1, 3).reshape(T // 16, T // 16, 256).any(dim=2)
        for row in tiles:
            idx = row.nonzero().flatten()
            if len(idx) and idx[0] > 0 and idx[-1] < len(row) - 1:
                found += 1
                break
    assert found >= 1


@pytest.mark.parametrize("channels, K, V", [(16, 8, 8), (24, 6, 10), (32, 16, 64), (5, 1, 1)])
def test_module_widths_and_parameter_names(channels, K, V):
    m = pkg().hip_nn.TemporalAttention(channels, K, V, "band", 3)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "qkv.weight": (2 * K + V, channels, 1), "qkv.bias": (2 * K + V,), "out.weight": (channels, V, 1),
        "out.bias": (channels,)}
    assert float(m.out.weight.detach().abs().max()) == 0.0 and float(m.out.bias.detach().abs().max()) == 0.0
    assert float(m.qkv.weight.detach().abs().max()) > 0.0


def test_module_qkv_initialisation_is_conv1d_default_from_the_global_rng():
    torch.manual_seed(7)
    m = pkg().hip_nn.TemporalAttention(16, 8, 12)
    torch.manual_seed(7)
    a = torch.nn.Conv1d(16, 28, 1)
    assert torch.equal(m.qkv.weight, a.weight) and torch.equal(m.qkv.bias, a.bias)


@pytest.mark.parametrize("bad", [dict(channels=16, key_size=0, value_size=8), dict(channels=16, key_size=8, value_size=65),
                                 dict(channels=16, key_size=8, value_size=8, mask="future"),
                                 dict(channels=16, key_size=8, value_size=8, mask="band", band=0),
                                 dict(channels=16, key_size=8, value_size=8, band=-1)])
def test_module_refuses_bad_arguments(bad):
    with pytest.raises(ValueError):
        pkg().hip_nn.TemporalAttention(**bad)


def _model(name, **kw):
    np.random.seed(1)           # the (dual-)quaternion layers draw from numpy, torch.nn's from torch
    torch.manual_seed(1)
    return pkg().model.SELD_Model(**dict(model_kwargs(CASE[name]), **kw))


def _at_keys(prefix, j):
    return {f"{prefix}.at.{j}.{m}.{p}" for m in ("qkv", "out") for p in ("weight", "bias")}


@pytest.mark.parametrize("D, blocks, firsts", [([2], 1, [0]), ([2, 2], 2, [0, 2]), ([[1, 2], [1]], 2, [0, 2])])
def test_one_block_per_dilation_stack(D, blocks, firsts):
    """at_key_size=8, at_value_size=12 adds tcn.at.{j}.{qkv,out}.{weight,bias}, one block per entry of D, and nothing
    else; the blocks come last in the state dict; every block has the TCN's channel count."""
    off, on = _model("tiny_DQ", D=D), _model("tiny_DQ", D=D, at_key_size=8, at_value_size=12)
    want = set()
    for j in range(blocks):
        want |= _at_keys("seld_block.tcn", j)
    keys_on, keys_off = list(on.state_dict()), list(off.state_dict())
    assert set(keys_on) - set(keys_off) == want and set(keys_off) - set(keys_on) == set()
    tcn_keys = [k for k in keys_on if k.startswith("seld_block.tcn.")]
    assert all(".at." in k for k in tcn_keys[-4 * blocks:]) and not any(".at." in k for k in tcn_keys[:-4 * blocks])
    tcn = on.seld_block.tcn
    assert sorted(tcn._at_before) == firsts and [tcn._at_before[i] for i in firsts] == list(range(blocks))
    sd = on.state_dict()
    C = sd["seld_block.tcn.ResBlocks.0.batch_filter1.weight"].shape[0]
    for j in range(blocks):
        assert tuple(sd[f"seld_block.tcn.at.{j}.qkv.weight"].shape) == (2 * 8 + 12, C, 1)
        assert tuple(sd[f"seld_block.tcn.at.{j}.out.weight"].shape) == (C, 12, 1)
    assert R.stack_starts(D) == firsts


def test_value_size_defaults_to_the_key_size():
    m = _model("tiny_DQ", at_key_size=6)
    blk = m.seld_block.tcn.at[0]
    assert (blk.key_size, blk.value_size, blk.mask, blk.band) == (6, 6, "causal", 0)


def test_two_stream_model_has_the_blocks_on_both_branches():
    m = _model("tiny_2stream", at_key_size=4)
    added = [k for k in m.state_dict() if ".at." in k]
    assert len(added) == 8 and sum(k.startswith("branch_A.tcn.at.0.") for k in added) == 4 \
        and sum(k.startswith("branch_B.tcn.at.0.") for k in added) == 4


@pytest.mark.parametrize("name", ["tiny_R", "tiny_DQ", "tiny_2stream"])
def test_at_off_draws_nothing_and_adds_nothing(name):
    """at_key_size=0 (given or defaulted, whatever the other arguments): the key set and, under one seed, the initial
    weights of the model without the arguments, bit for bit; the global RNGs end in the same state; and the reference's
    own three arguments stay inert."""
    base = _model(name)
    state, np_state = torch.get_rng_state(), np.random.get_state()[1].copy()
    for kw in (dict(at_key_size=0), dict(at_key_size=0, at_value_size=16, at_mask="band", at_band=4),
               dict(attention_type="self_attention", key_size=16)):
        m = _model(name, **kw)
        assert torch.equal(torch.get_rng_state(), state) and (np.random.get_state()[1] == np_state).all()
        a, b = base.state_dict(), m.state_dict()
        assert list(a) == list(b)
        assert all(torch.equal(a[k], b[k]) for k in a)
        assert not any(isinstance(x, pkg().hip_nn.TemporalAttention) for x in m.modules())


@pytest.mark.parametrize("name", ["tiny_R", "tiny_DQ", "tiny_2stream"])
def test_at_on_leaves_every_other_initial_weight(name):
    """The blocks are registered last: under one seed every non-AT tensor of the model with the blocks equals the model
    without them."""
    a, b = _model(name).state_dict(), _model(name, at_key_size=8, at_value_size=12, at_mask="band", at_band=5).state_dict()
    assert [k for k in b if ".at." not in k] == list(a)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kw", [dict(at_key_size=-1), dict(at_key_size=8, at_value_size=-2), dict(at_key_size=65),
                                dict(at_key_size=8, at_value_size=65), dict(at_key_size=8, at_mask="future"),
                                dict(at_key_size=8, at_mask="band"), dict(at_key_size=8, at_mask="band", at_band=0),
                                dict(at_key_size=8.0), dict(at_key_size=True), dict(at_key_size=8, at_band=-1)])
def test_model_refuses_bad_at_arguments(kw):
    M = pkg().model
    with pytest.raises(ValueError, match="at_"):
        _model("tiny_DQ", **kw)
    with pytest.raises(ValueError, match="at_"):
        M.TC_Block(16, D=[2], **kw)
    with pytest.raises(ValueError, match="at_"):
        M.ConvTC_Block(64, freq_dim=128, input_channels=8, cnn_filters=[16, 16, 16], D=[2], G=32, U=16, V=[16, 16], **kw)


def test_flags_parse_and_reach_the_model():
    T = pkg().train
    args = T.parse_args(["--TextArgs=none"])
    assert (args.at_key_size, args.at_value_size, args.at_mask, args.at_band) == (0, 0, "causal", 0)
    assert T.at_from_args(args) == dict(at_key_size=0, at_value_size=0, at_mask="causal", at_band=0)
    args = T.parse_args(["--TextArgs=none", "--at_key_size=16", "--at_value_size=64", "--at_mask=band", "--at_band=64"])
    assert T.at_from_args(args) == dict(at_key_size=16, at_value_size=64, at_mask="band", at_band=64)
    assert T.at_from_args(object()) == dict(at_key_size=0, at_value_size=0, at_mask="causal", at_band=0)
    flags = dict(domain="DQ", domain_classifier="DQ", input_channels=8, time_dim=64, freq_dim=128,
                 cnn_filters="[16, 16, 16]", G=32, U=16, V="[16, 16]", fc_layers="[16]", TextArgs="none")
    argv = [f"--{k}={v}" for k, v in flags.items()]
    m = T.model_from_args(T.parse_args(argv + ["--at_key_size=8", "--at_value_size=12", "--at_mask=band", "--at_band=5", "--D=[3,3,3]"]))
    blocks = list(m.seld_block.tcn.at)
    assert len(blocks) == 3
    assert all((b.key_size, b.value_size, b.mask, b.band) == (8, 12, "band", 5) for b in blocks)
    assert not any(".at." in k for k in T.model_from_args(T.parse_args(argv)).state_dict())


@pytest.mark.parametrize("argv, match", [(["--at_key_size=-2"], "at_key_size"), (["--at_key_size=80"], "at_key_size"),
                                         (["--at_key_size=8", "--at_value_size=70"], "at_value_size"),
                                         (["--at_key_size=8", "--at_mask=future"], "at_mask"),
                                         (["--at_key_size=8", "--at_mask=band"], "at_band")])
def test_main_refuses_bad_flags_before_the_device(argv, match, monkeypatch):
    """The refusal comes before anything asks for the device: torch.cuda.is_available is made to fail the test."""
    T = pkg().train

    def touched():
        raise AssertionError("the device was touched before the flags were refused")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    with pytest.raises(ValueError, match=match):
        T.main(T.parse_args(["--TextArgs=none"] + argv))
