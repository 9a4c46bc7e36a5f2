"""Quaternion rotation ops on the MI355X (csrc/quat_rotation.hip + the algebra-1 convolution / transposed convolution /
linear kernels): the reference fixture through the functional ops and the layers, the form kernels in both layouts,
model-width shapes against float64, run-to-run identity, a recorded training step and the kernels a forward issues."""
import collections

import numpy as np
import pytest
import torch

from oracle.seld_oracle import closed_form_input
from tests.golden.rotation_cases import (LAYER_CASES, all_variants, rotation_cotangent, rotation_inputs,
                                         rotation_matrix, rotation_reference64)
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VARIANTS = all_variants()


def _mods():
    P = pkg()
    return P, P._lib, P.hip_ops, P.quaternion.quaternion_ops, P.quaternion.quaternion_layers


def _close(got, ref, tol, what=""):
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= tol * max(ref.abs().max().item(), 1e-30), (what, err, ref.abs().max().item())


def _functional(Q, case, x, ws, bias, qformat):
    if case["kind"] == "conv":
        return Q.quaternion_conv_rotation(x, *ws, bias, case["stride"], case["padding"], 1, case["dilation"], qformat)
    if case["kind"] == "tconv":
        return Q.quaternion_transpose_conv_rotation(x, *ws, bias, case["stride"], case["padding"],
                                                    case["output_padding"], 1, case["dilation"], qformat)
    return Q.quaternion_linear_rotation(x, *ws, bias, qformat)


def _check_fixture(g, name, y, x, ws, bias):
    _close(y, g[name + ".y"], 1e-4, "y")
    _close(x.grad, g[name + ".dx"], 1e-4, "dx")
    for c, w in zip("rijk", ws):
        _close(w.grad, g[f"{name}.d{c}"], 1e-4, "d" + c)
    if bias is not None:
        _close(bias.grad, g[name + ".dbias"], 1e-4, "dbias")


@pytest.mark.parametrize("case,name,qformat,has_bias", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_fixture_functional(golden, case, name, qformat, has_bias):
    _, _, _, Q, _ = _mods()
    g = golden("rotation")
    x, ws, bias = rotation_inputs(case, qformat, has_bias)
    x = x.to(DEV).requires_grad_(True)
    ws = [w.to(DEV).requires_grad_(True) for w in ws]
    bias = bias.to(DEV).requires_grad_(True) if bias is not None else None
    y = _functional(Q, case, x, ws, bias, qformat)
    (y * rotation_cotangent(y.shape).to(DEV)).sum().backward()
    _check_fixture(g, name, y, x, ws, bias)


def _layer_from_case(Ql, case, qformat, has_bias):
    w = case["w"]
    if case["kind"] == "linear":
        m = Ql.QuaternionLinearAutograd(4 * w[0], 4 * w[1], bias=has_bias, seed=3, rotation=True,
                                        quaternion_format=qformat)
    else:
        nd = len(w) - 2
        k = w[2] if nd == 1 else tuple(w[2:])
        kw = dict(dilatation=case["dilation"], padding=case["padding"], bias=has_bias, seed=3,
                  operation=f"convolution{nd}d", rotation=True, quaternion_format=qformat)
        if case["kind"] == "conv":
            m = Ql.QuaternionConv(4 * w[1], 4 * w[0], k, case["stride"], **kw)
        else:
            m = Ql.QuaternionTransposeConv(4 * w[0], 4 * w[1], k, case["stride"], output_padding=case["output_padding"],
                                           **kw)
    _, ws, bias = rotation_inputs(case, True, has_bias)          # a layer's bias always holds 4*O elements
    with torch.no_grad():
        for p, t in zip((m.r_weight, m.i_weight, m.j_weight, m.k_weight), ws):
            p.copy_(t)
        if has_bias:
            m.bias.copy_(bias)
    return m.to(DEV)


@pytest.mark.parametrize("case,name,qformat,has_bias", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_fixture_through_layer(golden, case, name, qformat, has_bias):
    _, L, _, _, Ql = _mods()
    g = golden("rotation")
    m = _layer_from_case(Ql, case, qformat, has_bias)
    x = rotation_inputs(case, qformat, has_bias)[0].to(DEV).requires_grad_(True)
    if has_bias and not qformat:
        # the reference's layers fail here too: their bias has 4*O elements, the rotation op 3*O output channels
        with pytest.raises(L.SeldHipError, match="bias"):
            m(x)
        return
    y = m(x)
    (y * rotation_cotangent(y.shape).to(DEV)).sum().backward()
    _check_fixture(g, name, y, x, (m.r_weight, m.i_weight, m.j_weight, m.k_weight), m.bias)


def _seeded_layer(Ql, c):
    np.random.seed(c["np_seed"])
    return getattr(Ql, c["cls"])(**c["kwargs"]).to(DEV)


@pytest.mark.parametrize("c", LAYER_CASES, ids=[c["name"] for c in LAYER_CASES])
def test_seeded_layer(golden, c):
    _, _, _, _, Ql = _mods()
    g = golden("rotation")
    name = c["name"]
    m = _seeded_layer(Ql, c)
    x = closed_form_input(c["x"]).to(DEV).requires_grad_(True)
    y = m(x)
    _close(y, g[name + ".y"], 1e-4, "y")
    (y * rotation_cotangent(y.shape).to(DEV)).sum().backward()
    _close(x.grad, g[name + ".dx"], 1e-4, "dx")
    for k, p in m.named_parameters():
        _close(p.grad, g[f"{name}.grad.{k}"], 1e-4, k)


@pytest.mark.parametrize("layout,shape", [(0, (5, 7, 3)), (0, (2, 3, 4, 2)), (1, (37, 45)), (1, (3, 70))])
@pytest.mark.parametrize("qformat", [False, True])
def test_form_kernels(layout, shape, qformat):
    """seld_quat_rotation_form against the restated K (K^T for the linear layout), zero blocks exactly 0, and
    seld_quat_rotation_form_bwd against float64 autograd, storing and accumulating."""
    _, L, H, _, _ = _mods()
    gen = torch.Generator().manual_seed(17)
    ws = [torch.randn(shape, generator=gen, dtype=torch.float64) * 0.5 for _ in range(4)]
    for w in ws:
        w.requires_grad_(True)
    K64 = rotation_matrix(ws, qformat)
    if layout == L.SELD_ROT_LAYOUT_LINEAR:
        K64 = K64.t()
    wd = [w.detach().float().to(DEV) for w in ws]
    K = H.rotation_form(layout, qformat, wd)
    torch.cuda.synchronize()
    _close(K, K64.detach(), 2e-6, "K")
    if qformat:
        A, B = shape[0], shape[1]
        Kc = K.cpu() if layout == L.SELD_ROT_LAYOUT_CONV else K.cpu().t()
        assert torch.count_nonzero(Kc[:A]).item() == 0 and torch.count_nonzero(Kc[:, :B]).item() == 0
    dK = torch.randn(K64.shape, generator=gen, dtype=torch.float64)
    grads = torch.autograd.grad((K64 * dK).sum(), ws)
    dws = [torch.full_like(w, float("nan")) for w in wd]
    H.rotation_form_bwd(layout, qformat, wd, dK.float().to(DEV), dws, accumulate=False)
    for c, (got, ref) in enumerate(zip(dws, grads)):
        _close(got, ref, 1e-5, f"dw{c}")
    base = [torch.randn(shape, generator=gen) for _ in range(4)]
    acc = [b.to(DEV) for b in base]
    H.rotation_form_bwd(layout, qformat, wd, dK.float().to(DEV), acc, accumulate=True)
    for c, (got, ref) in enumerate(zip(acc, grads)):
        _close(got, ref + base[c].double(), 1e-5, f"dw{c} accumulated")


MODEL_SHAPES = [
    dict(name="conv1d_k3_d2", kind="conv", x=(8, 144, 512), w=(48, 48, 3), stride=1, padding=2, dilation=2,
         qformat=False, bias=True),
    dict(name="tconv2d_k4_s2", kind="tconv", x=(2, 96, 16, 32), w=(24, 24, 4, 4), stride=2, padding=1,
         output_padding=0, dilation=1, qformat=True, bias=True),
    dict(name="linear_4096x288", kind="linear", x=(4096, 288), w=(96, 96), qformat=False, bias=True),
]


@pytest.mark.parametrize("case", MODEL_SHAPES, ids=[c["name"] for c in MODEL_SHAPES])
def test_model_width_shapes(case):
    _, _, _, Q, _ = _mods()
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(case["x"], generator=gen, dtype=torch.float64)
    ws = [torch.randn(case["w"], generator=gen, dtype=torch.float64) * 0.3 for _ in range(4)]
    nout = (4 if case["qformat"] else 3) * (case["w"][0] if case["kind"] == "conv" else case["w"][1])
    bias = torch.randn(nout, generator=gen, dtype=torch.float64) * 0.1 if case["bias"] else None
    leaves = [x] + ws + ([bias] if bias is not None else [])
    dev = [t.float().to(DEV).requires_grad_(True) for t in leaves]
    for t in leaves:
        t.requires_grad_(True)
    yr = rotation_reference64(case, x, ws, bias, case["qformat"])
    y = _functional(Q, case, dev[0], dev[1:5], dev[5] if bias is not None else None, case["qformat"])
    _close(y, yr.detach(), 1e-4, "y")
    cot = torch.randn(yr.shape, generator=gen, dtype=torch.float64)
    (yr * cot).sum().backward()
    (y * cot.float().to(DEV)).sum().backward()
    _close(dev[0].grad, x.grad, 1e-4, "dx")
    for c in range(4):
        _close(dev[1 + c].grad, ws[c].grad, 2e-4, "rijk"[c])
    if bias is not None:
        _close(dev[5].grad, bias.grad, 1e-4, "dbias")


def _small_layers(Ql):
    np.random.seed(0)            # the quaternion initialiser draws its unit axes from numpy's global generator
    return [
        Ql.QuaternionConv(48, 64, 3, 1, dilatation=2, padding=2, seed=4, operation="convolution1d", rotation=True,
                          quaternion_format=True),
        Ql.QuaternionTransposeConv(32, 32, 4, 2, padding=1, seed=5, rotation=True, quaternion_format=True),
        Ql.QuaternionLinearAutograd(96, 64, bias=False, seed=6, rotation=True),
    ]


_SMALL_X = [(4, 48, 256), (2, 32, 16, 24), (512, 72)]


def test_deterministic_backward_repeats_bit_identical(seld_env):
    seld_env.set("SELD_DETERMINISTIC", "1")
    _, _, _, _, Ql = _mods()
    for m, xs in zip(_small_layers(Ql), _SMALL_X):
        m = m.to(DEV)
        x = closed_form_input(xs).to(DEV).requires_grad_(True)
        runs = []
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            x.grad = None
            y = m(x)
            (y * rotation_cotangent(y.shape).to(DEV)).sum().backward()
            torch.cuda.synchronize()
            runs.append([x.grad.clone()] + [p.grad.clone() for p in m.parameters()])
        for a, b in zip(*runs):
            assert torch.equal(a, b), type(m).__name__


@pytest.mark.parametrize("which", [0, 1, 2], ids=["conv", "tconv", "linear"])
def test_recorded_step_equals_eager(which):
    """A rotation layer's forward + backward + FlatAdam step recorded with torch.cuda.graph and replayed once, against the
    same step run eagerly from the same state."""
    P, _, _, _, Ql = _mods()
    T = P.train
    xs = _SMALL_X[which]

    def make():
        m = _small_layers(Ql)[which].to(DEV)
        return m, T.FlatAdam(m.parameters(), lr=1e-3)
    x = closed_form_input(xs).to(DEV)
    cot = None

    def step(m, opt, inp):
        opt.zero_grad()
        y = m(inp)
        (y * cot).sum().backward()
        opt.step()
        return y

    mE, oE = make()
    with torch.no_grad():
        cot = rotation_cotangent(mE(x).shape).to(DEV)
    yE = step(mE, oE, x).detach().clone()

    mG, oG = make()
    p0 = oG.flat_param.clone()
    xg = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(mG, oG, xg)                                   # warm-up: allocator pools, modules, host caches
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    oG.step_count = 0                                      # the recorded Adam launch is step 1, as the eager one
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yG = step(mG, oG, xg)
    with torch.no_grad():                                  # back to the state the eager step started from
        oG.flat_param.copy_(p0)
        oG.exp_avg.zero_()
        oG.exp_avg_sq.zero_()
    g.replay()
    torch.cuda.synchronize()
    _close(yG, yE.cpu(), 1e-6, "y")
    _close(oG.flat_grad, oE.flat_grad.cpu(), 1e-5, "gradients")
    _close(oG.flat_param, oE.flat_param.cpu(), 1e-6, "parameters after Adam")
    assert not torch.equal(oG.flat_param, p0)
    assert oE.flat_grad.abs().max().item() > 0


@pytest.mark.parametrize("which", [0, 1, 2], ids=["conv", "tconv", "linear"])
def test_forward_issues_only_library_kernels(which):
    from torch.profiler import ProfilerActivity, profile
    _, _, _, _, Ql = _mods()
    m = _small_layers(Ql)[which].to(DEV)
    x = closed_form_input(_SMALL_X[which]).to(DEV)
    m(x)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        m(x)
        torch.cuda.synchronize()
    names = collections.Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    assert any("rot_form" in k for k in names), names
    foreign = {k: v for k, v in names.items() if "seld::" not in k}
    assert not foreign, foreign
