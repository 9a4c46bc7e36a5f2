"""Squeeze-and-excitation, the parts that need no device: the fp64 yardstick tests/se_ref.py against torch.autograd, the
module's derived widths, the state-dict layout of models with se_reduction on and off, and the training flags."""
import numpy as np
import pytest
import torch

from tests import se_ref as R
from tests.golden.cases import MODEL_CASES, model_kwargs
from tests.helpers import pkg

CASE = {c["name"]: c for c in MODEL_CASES}


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_se_ref_formulas_match_autograd(case):
    """The formulas of se_ref (forward, intermediates and every gradient) against autograd on the same expression built
    from torch ops in fp64: 1e-12 relative to each tensor's largest entry (fp64 rounding of sums of at most 4099 x 8
    terms is below 1e-12)."""
    N, C, spatial, A, Hd = case
    x, dy, w1, b1, w2, b2 = R.make_case(case)
    f = R.se_forward(x, w1, b1, w2, b2, A)
    b = R.se_backward(x, dy, w1, w2, f["z"], f["h"], f["s"], A)
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    xa, w1a, b1a, w2a, b2a = leaves
    Cg = C // A
    z = xa.reshape(N, A, Cg, -1).mean(dim=(1, 3))
    h = torch.relu(torch.nn.functional.linear(z, w1a, b1a))
    s = torch.sigmoid(torch.nn.functional.linear(h, w2a, b2a))
    gate = torch.cat([s] * A, dim=1).reshape(N, C, *([1] * len(spatial)))
    y = xa * gate
    y.backward(dy)
    assert f["h"].max() > 0 and (Hd < 2 or f["h"].min() == 0), "the weights must reach both sides of the ReLU"
    for name, got, want in (("z", f["z"], z), ("h", f["h"], h), ("s", f["s"], s), ("y", f["y"], y),
                            ("dx", b["dx"], xa.grad), ("dw1", b["dw1"], w1a.grad), ("db1", b["db1"], b1a.grad),
                            ("dw2", b["dw2"], w2a.grad), ("db2", b["db2"], b2a.grad)):
        want = want.detach()
        assert got.shape == want.shape, name
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name


def test_case_inputs_span_the_gate_and_both_relu_sides():
    """Over the case table s reaches below 0.1 and above 0.9, and h has zeros and positive entries."""
    s_all, h_all = [], []
    for case in R.CASES:
        x, _, w1, b1, w2, b2 = R.make_case(case)
        f = R.se_forward(x, w1, b1, w2, b2, case[3])
        s_all.append(f["s"].flatten())
        h_all.append(f["h"].flatten())
    s_all, h_all = torch.cat(s_all), torch.cat(h_all)
    assert s_all.min() < 0.1 and s_all.max() > 0.9, (float(s_all.min()), float(s_all.max()))
    assert (h_all == 0).any() and (h_all > 0).any()


@pytest.mark.parametrize("channels, reduction, components, gated, hidden",
                         [(64, 4, 1, 64, 16), (64, 4, 4, 16, 4), (64, 4, 8, 8, 2), (32, 16, 8, 4, 1), (16, 1, 4, 4, 4),
                          (8, 4, 8, 1, 1)])
def test_module_widths_and_parameter_names(channels, reduction, components, gated, hidden):
    m = pkg().hip_nn.SqueezeExcite(channels, reduction, components)
    assert (m.gated, m.hidden) == (gated, hidden)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "fc1.weight": (hidden, gated), "fc1.bias": (hidden,), "fc2.weight": (gated, hidden), "fc2.bias": (gated,)}


def test_module_initialisation_is_nn_linear_default_from_the_global_rng():
    torch.manual_seed(7)
    m = pkg().hip_nn.SqueezeExcite(32, 4, 4)
    torch.manual_seed(7)
    a, b = torch.nn.Linear(8, 2), torch.nn.Linear(2, 8)
    for got, want in ((m.fc1.weight, a.weight), (m.fc1.bias, a.bias), (m.fc2.weight, b.weight), (m.fc2.bias, b.bias)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("bad", [dict(channels=12, reduction=4, components=8), dict(channels=16, reduction=0, components=4),
                                 dict(channels=16, reduction=4, components=2)])
def test_module_refuses_bad_arguments(bad):
    with pytest.raises(ValueError):
        pkg().hip_nn.SqueezeExcite(**bad)


def _model(name, **kw):
    np.random.seed(1)           # the (dual-)quaternion layers draw from numpy, torch.nn's from torch
    torch.manual_seed(1)
    return pkg().model.SELD_Model(**dict(model_kwargs(CASE[name]), **kw))


def _se_keys(prefix):
    return {f"{prefix}.fc{i}.{p}" for i in (1, 2) for p in ("weight", "bias")}


@pytest.mark.parametrize("name, components", [("tiny_R", 1), ("tiny_Q", 4), ("tiny_DQ", 8)])
def test_state_dict_gains_only_the_se_keys(name, components):
    """se_reduction=4 adds cnn.{i}.5.* and ResBlocks.{i}.se.* and nothing else; every module has the domain's component
    count and hidden width max(1, gated // 4)."""
    off, on = _model(name), _model(name, se_reduction=4)
    want = set()
    for i in range(3):
        want |= _se_keys(f"seld_block.cnn.{i}.5")
    for i in range(10):
        want |= _se_keys(f"seld_block.tcn.ResBlocks.{i}.se")
    assert set(on.state_dict()) - set(off.state_dict()) == want
    assert set(off.state_dict()) - set(on.state_dict()) == set()
    mods = [m for m in on.modules() if isinstance(m, pkg().hip_nn.SqueezeExcite)]
    assert len(mods) == 13 and all(m.components == components for m in mods)
    assert [m.channels for m in mods] == [16, 16, 16] + [32] * 10
    assert all(m.hidden == max(1, m.channels // components // 4) for m in mods)


@pytest.mark.parametrize("mode, cnn, tcn", [("cnn", 3, 0), ("tcn", 0, 10), ("both", 3, 10)])
def test_se_mode_selects_the_subset(mode, cnn, tcn):
    added = set(_model("tiny_DQ", se_reduction=2, se_mode=mode).state_dict()) - set(_model("tiny_DQ").state_dict())
    assert sum(".cnn." in k for k in added) == 4 * cnn and sum(".ResBlocks." in k for k in added) == 4 * tcn
    assert len(added) == 4 * (cnn + tcn)


def test_stage_without_batch_norm_keeps_key_5():
    m = _model("tiny_DQ", se_reduction=4, batch_norm="noBN")
    assert "seld_block.cnn.0.5.fc1.weight" in m.state_dict() and "seld_block.cnn.0.4.fc1.weight" not in m.state_dict()


@pytest.mark.parametrize("name", ["tiny_R", "tiny_DQ", "tiny_2stream"])
def test_se_off_draws_nothing_and_adds_nothing(name):
    """se_reduction=0 (given or defaulted, whatever the mode): the key set and, under one seed, the initial weights of the
    model without the arguments, bit for bit, and the global RNG ends in the same state."""
    base = _model(name)
    state, np_state = torch.get_rng_state(), np.random.get_state()[1].copy()
    for kw in (dict(se_reduction=0), dict(se_reduction=0, se_mode="cnn")):
        m = _model(name, **kw)
        assert torch.equal(torch.get_rng_state(), state) and (np.random.get_state()[1] == np_state).all()
        a, b = base.state_dict(), m.state_dict()
        assert list(a) == list(b)
        assert all(torch.equal(a[k], b[k]) for k in a)
        assert not any(isinstance(x, pkg().hip_nn.SqueezeExcite) for x in m.modules())


def test_late_parameters_hold_the_stage_se_parameters():
    """dp.late_parameters takes `cnn.parameters()`: the stages' SE parameters ride in the front-end bucket, the residual
    blocks' do not."""
    m = _model("tiny_DQ", se_reduction=4)
    late = {id(p) for p in pkg().dp.late_parameters(m)}
    names = dict(m.named_parameters())
    assert all(id(names[f"seld_block.cnn.{i}.5.fc1.weight"]) in late for i in range(3))
    assert id(names["seld_block.tcn.ResBlocks.0.se.fc1.weight"]) not in late


def test_model_refuses_bad_se_arguments():
    for kw in (dict(se_reduction=-1), dict(se_reduction=4, se_mode="all"), dict(se_reduction=2.0), dict(se_reduction=True)):
        with pytest.raises(ValueError, match="se_"):
            _model("tiny_DQ", **kw)


def test_flags_parse_and_reach_the_model():
    T = pkg().train
    args = T.parse_args(["--TextArgs=none"])
    assert (args.se_reduction, args.se_mode) == (0, "both")
    assert T.se_from_args(args) == dict(se_reduction=0, se_mode="both")
    args = T.parse_args(["--TextArgs=none", "--se_reduction=4", "--se_mode=tcn"])
    assert T.se_from_args(args) == dict(se_reduction=4, se_mode="tcn")
    flags = dict(domain="DQ", domain_classifier="DQ", input_channels=8, time_dim=64, freq_dim=128,
                 cnn_filters="[16, 16, 16]", G=32, U=16, V="[16, 16]", fc_layers="[16]", TextArgs="none")
    argv = [f"--{k}={v}" for k, v in flags.items()]
    m = T.model_from_args(T.parse_args(argv + ["--se_reduction=4", "--se_mode=tcn"]))
    keys = [k for k in m.state_dict() if ".fc1.weight" in k]
    assert len(keys) == 10 and all(".se." in k for k in keys)
    assert not any(".fc1." in k for k in T.model_from_args(T.parse_args(argv)).state_dict())


@pytest.mark.parametrize("argv, match", [(["--se_reduction=-2"], "se_reduction"), (["--se_reduction=4", "--se_mode=all"], "se_mode")])
def test_main_refuses_bad_flags_before_the_device(argv, match, monkeypatch):
    """The refusal comes before anything asks for the device: torch.cuda.is_available is made to fail the test."""
    T = pkg().train

    def touched():
        raise AssertionError("the device was touched before the flags were refused")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    with pytest.raises(ValueError, match=match):
        T.main(T.parse_args(["--TextArgs=none"] + argv))
