"""The optimiser's extras on the host: the fp64 chain the GPU tests compare with (tests/optim_ref.py) is
torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam / AdamW plus the moving average written out; bad flags are
refused before the device is touched; a checkpoint written without the flags has the keys it always had."""
import os

import pytest
import torch

from tests import optim_ref as R
from tests.golden.cases import MODEL_CASES
from tests.helpers import build_model, pkg

REF_CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_checkpoint_tiny_DQ.pt")


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_chain_is_torch_clip_then_adam_then_ema(decoupled):
    """Five steps in fp64, 1e-12 relative: coefficient, moments, weights and moving average.  The gradients are fp32
    values and grad_scale a power of two, so the fp32 product the reference norm forms is the exact one; their scale
    falls from step to step, so that early steps are clipped and late ones are not (both branches of the clamp)."""
    lr, wd, eps, gs, max_norm, decay = 1e-3, 1e-2, 1e-8, 0.25, 2.0, 0.999
    gen = torch.Generator().manual_seed(11)
    p = torch.nn.Parameter(torch.randn(64, generator=gen, dtype=torch.float64))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=lr, betas=(0.9, 0.999), eps=eps, weight_decay=wd)
    po, mo, vo = p.detach().clone(), torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    ema_t, ema_o = p.detach().clone(), p.detach().clone()
    clipped = []
    for step in range(1, 6):
        g32 = torch.randn(64, generator=gen) * 10.0 ** (2 - step)
        p.grad = g32.double() * gs
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        d = min(decay, (1 + step) / (10 + step))
        ema_t = d * ema_t + (1 - d) * p.detach()

        norm = R.grad_norm(g32, gs)
        coef = R.clip_coefficient(norm, max_norm)
        clipped.append(coef < 1.0)
        assert abs(norm - float(total)) <= 1e-12 * norm
        assert abs(coef - min(1.0, max_norm / (float(total) + 1e-6))) <= 1e-12 * coef
        po, mo, vo, ema_o = R.adam_ex_step(po, g32.double(), mo, vo, ema_o, step, lr=lr, eps=eps, weight_decay=wd,
                                           decoupled=decoupled, grad_scale=gs, coef=coef, ema_decay=decay)
        st = opt.state[p]
        for name, a, b in (("p", p.detach(), po), ("m", st["exp_avg"], mo), ("v", st["exp_avg_sq"], vo), ("ema", ema_t, ema_o)):
            assert torch.all((a - b).abs() <= 1e-12 * b.abs()), (decoupled, step, name, float((a - b).abs().max()))
    assert clipped[0] and not clipped[-1], clipped


def test_chain_without_extras_is_the_adam_oracle():
    from oracle import seld_oracle as O
    gen = torch.Generator().manual_seed(3)
    p, g, m = (torch.randn(32, generator=gen, dtype=torch.float64) for _ in range(3))
    v = torch.rand(32, generator=gen, dtype=torch.float64)
    got = R.adam_ex_step(p, g, m, v, None, 7, weight_decay=1e-2, grad_scale=0.25)
    ref = O.adam_step(p, g, m, v, 7, weight_decay=1e-2, grad_scale=0.25)
    assert got[3] is None and all(torch.equal(a, b) for a, b in zip(got[:3], ref))


def test_coefficient_propagates_inf_and_nan_as_torch_does():
    for bad in (float("inf"), float("nan")):
        g = torch.tensor([1.0, bad, -2.0])
        q = torch.nn.Parameter(torch.zeros(3))
        q.grad = g.clone()
        total = float(torch.nn.utils.clip_grad_norm_([q], 1.0))
        norm = R.grad_norm(g, 1.0)
        coef = R.clip_coefficient(norm, 1.0)
        assert (norm != norm) == (total != total) and (norm == total or norm != norm)
        # what torch multiplied the gradient by: grad[0] was 1.0
        assert (coef != coef and bool(torch.isnan(q.grad[0]))) or coef == float(q.grad[0])
    assert R.clip_coefficient(0.0, 3.0) == 1.0


REFUSALS = [(["--grad_clip=-1"], "grad_clip"), (["--grad_clip=nan"], "grad_clip"), (["--weight_decay=-0.01"], "weight_decay"),
            (["--ema_decay=1.0"], "ema_decay"), (["--ema_decay=-0.1"], "ema_decay"), (["--ema_decay=nan"], "ema_decay"),
            (["--warmup_steps=-5"], "warmup_steps")]


@pytest.mark.parametrize("argv,match", REFUSALS, ids=[a[0] for a, _ in REFUSALS])
def test_main_refuses_bad_flags_before_the_device(argv, match, monkeypatch):
    T = pkg().train

    def touched():
        raise AssertionError("the device was touched before the flags were refused")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    args = T.parse_args(["--TextArgs=none"] + argv)
    with pytest.raises(ValueError, match=match):
        T.optimizer_from_args(args)
    with pytest.raises(ValueError, match=match):
        T.main(args)


def test_flags_default_to_off_and_reach_the_optimiser():
    T = pkg().train
    off = T.parse_args(["--TextArgs=none"])
    assert (off.grad_clip, off.weight_decay, off.decoupled_weight_decay, off.ema_decay, off.warmup_steps) == (0., 0., False, 0., 0)
    assert T.optimizer_from_args(off) == dict(weight_decay=0.0, decoupled=False, max_grad_norm=0.0, ema_decay=0.0)
    on = T.parse_args(["--TextArgs=none", "--grad_clip=1.5", "--weight_decay=0.01", "--decoupled_weight_decay=True",
                       "--ema_decay=0.999", "--warmup_steps=100"])
    assert T.optimizer_from_args(on) == dict(weight_decay=0.01, decoupled=True, max_grad_norm=1.5, ema_decay=0.999)
    # decoupled decay of nothing is plain Adam: the step stays the launch it was
    assert T.optimizer_from_args(T.parse_args(["--TextArgs=none", "--decoupled_weight_decay=True"]))["decoupled"] is False
    assert [T.warmup_scale(s, 4) for s in (1, 2, 4, 9)] == [0.25, 0.5, 1.0, 1.0] and T.warmup_scale(1, 0) == 1.0


def test_flat_adam_without_extras_allocates_nothing_new():
    T = pkg().train
    model = torch.nn.Linear(4, 3)
    opt = T.FlatAdam(model.parameters(), lr=1e-3)
    assert opt.clip is None and opt.ema is None and not opt._extras and opt.lr_scale == 1.0
    assert opt.clip_stats() == (0.0, 0)
    before = opt.flat_param.clone()
    with opt.ema_weights():                      # no average: nothing moves
        assert torch.equal(opt.flat_param, before)
    for bad in (dict(max_grad_norm=-1.0), dict(ema_decay=1.0), dict(ema_decay=-0.5)):
        with pytest.raises(ValueError):
            T.FlatAdam(torch.nn.Linear(2, 2).parameters(), **bad)


def test_checkpoint_keys_without_the_flags_are_the_former_ones(tmp_path):
    """Against the reference's own checkpoint file: the same top-level keys in the same order, the same optimiser group
    keys.  With a moving average the file gains `ema_state_dict`, keyed like the model's parameters, and nothing else;
    load_model puts it back into the optimiser, and a file without one restarts the average from the loaded weights."""
    T = pkg().train
    case = next(c for c in MODEL_CASES if c["name"] == "tiny_DQ")
    ref = torch.load(REF_CKPT, map_location="cpu", weights_only=False)
    state = {"step": 7, "epochs": 3, "best_loss": 0.5, "worse_epochs": 0, "best_epoch": 3}

    m = build_model(case)
    opt = T.FlatAdam(m.parameters(), lr=1e-3)
    sch = T.StepLR(opt, 2, 0.5)
    plain = str(tmp_path / "plain")
    T.save_model(m, opt, state, plain, sch)
    ours = torch.load(plain, map_location="cpu", weights_only=False)
    assert list(ours.keys()) == list(ref.keys())
    assert set(ours["optimizer_state_dict"]["param_groups"][0]) == set(ref["optimizer_state_dict"]["param_groups"][0])

    m2 = build_model(case)
    opt2 = T.FlatAdam(m2.parameters(), lr=1e-3, ema_decay=0.999, max_grad_norm=1.0, weight_decay=1e-2, decoupled=True)
    sch2 = T.StepLR(opt2, 2, 0.5)
    assert torch.equal(opt2.ema, opt2.flat_param) and opt2.ema.data_ptr() != opt2.flat_param.data_ptr()
    opt2.ema.mul_(0.5)
    with_ema = str(tmp_path / "with_ema")
    T.save_model(m2, opt2, state, with_ema, sch2)
    theirs = torch.load(with_ema, map_location="cpu", weights_only=False)
    assert set(theirs.keys()) == set(ref.keys()) | {"ema_state_dict"}
    assert set(theirs["optimizer_state_dict"]["param_groups"][0]) == set(ref["optimizer_state_dict"]["param_groups"][0])
    params = dict(m2.named_parameters())
    assert list(theirs["ema_state_dict"]) == list(params)
    for k, v in theirs["ema_state_dict"].items():
        assert torch.equal(v, 0.5 * params[k].detach()), k
        assert torch.equal(theirs["model_state_dict"][k], params[k].detach()), k       # the training weights, not the average

    m3 = build_model(case)
    opt3 = T.FlatAdam(m3.parameters(), lr=1e-3, ema_decay=0.999)
    T.load_model(m3, opt3, with_ema, False, "cpu", T.StepLR(opt3, 2, 0.5))
    assert torch.equal(opt3.flat_param, opt2.flat_param) and torch.equal(opt3.ema, opt2.ema)
    opt3.ema.zero_()
    T.load_model(m3, opt3, plain, False, "cpu", T.StepLR(opt3, 2, 0.5))      # no average in the file: starts from its weights
    assert torch.equal(opt3.ema, opt3.flat_param) and torch.equal(opt3.flat_param, opt.flat_param)


def test_ema_scope_lends_the_average_to_any_prediction_call():
    """predict_test, predict_test_post and predict_recordings keep their pinned signatures; a caller wraps them in
    ema_scope(optimizer), which is ema_weights() for an optimiser with an average and nothing otherwise."""
    T = pkg().train
    model = torch.nn.Linear(4, 3)
    opt = T.FlatAdam(model.parameters(), lr=1e-3, ema_decay=0.9)
    opt.ema.mul_(2.0)
    weights = opt.flat_param.clone()
    with T.ema_scope(opt):
        assert torch.equal(opt.flat_param, 2.0 * weights) and torch.equal(model.weight.detach().reshape(-1), 2.0 * weights[:12])
    assert torch.equal(opt.flat_param, weights) and torch.equal(opt.ema, 2.0 * weights)
    plain = T.FlatAdam(torch.nn.Linear(4, 3).parameters(), lr=1e-3)
    for nothing in (None, plain, torch.optim.SGD(torch.nn.Linear(2, 2).parameters(), lr=0.1)):
        with T.ema_scope(nothing):
            pass
