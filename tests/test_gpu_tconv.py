"""Quaternion / real transposed convolution on the MI355X (csrc/hc_conv_transpose.hip): the reference fixture, the
benchmark shapes against a float64 restatement, algebra 1, the mirrored data-gradient entry, run-to-run identity,
refused descriptors and a recorded training step."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.seld_oracle import assemble_conv_weight
from tests.golden.tconv_cases import LAYER_CASE, TCONV_CASES, tconv_cotangent, tconv_inputs
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL, EUNSUPPORTED = -1, -4            # include/seld_hip.h


def _mods():
    P = pkg()
    return P, P._lib, P.hip_ops, P.quaternion.quaternion_ops, P.quaternion.quaternion_layers


def _close(got, ref, tol, what=""):
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= tol * max(ref.abs().max().item(), 1e-30), (what, err, ref.abs().max().item())


def _tconv64(x, ws, bias, stride, padding, output_padding, dilation):
    fn = F.conv_transpose1d if x.dim() == 3 else F.conv_transpose2d
    return fn(x, assemble_conv_weight(ws), bias, stride, padding, output_padding, 1, dilation)


@pytest.mark.parametrize("case", TCONV_CASES, ids=[c["name"] for c in TCONV_CASES])
def test_fixture_forward_backward(golden, case):
    _, _, _, Q, _ = _mods()
    g = golden("tconv")
    name = case["name"]
    x, ws, bias = tconv_inputs(case)
    x = x.to(DEV).requires_grad_(True)
    ws = [w.to(DEV).requires_grad_(True) for w in ws]
    bias = bias.to(DEV).requires_grad_(True) if bias is not None else None
    y = Q.quaternion_transpose_conv(x, *ws, bias, case["stride"], case["padding"], case["output_padding"], 1,
                                    case["dilation"])
    _close(y, g[name + ".y"], 1e-4, "y")
    (y * tconv_cotangent(y.shape).to(DEV)).sum().backward()
    _close(x.grad, g[name + ".du"], 1e-4, "du")
    for i, w in enumerate(ws):
        _close(w.grad, g[f"{name}.dw{i}"], 1e-4, f"dw{i}")
    if bias is not None:
        _close(bias.grad, g[name + ".dbias"], 1e-4, "dbias")


def _layer_from_case(Ql, case):
    x_dim = len(case["x"])
    k = case["k"][0] if x_dim == 3 else case["k"]
    op = "convolution1d" if x_dim == 3 else "convolution2d"
    m = Ql.QuaternionTransposeConv(case["x"][1], case["cout"], k, case["stride"], dilatation=case["dilation"],
                                   padding=case["padding"], output_padding=case["output_padding"], bias=case["bias"],
                                   seed=3, operation=op)
    _, ws, bias = tconv_inputs(case)
    with torch.no_grad():
        for p, w in zip((m.r_weight, m.i_weight, m.j_weight, m.k_weight), ws):
            p.copy_(w)
        if bias is not None:
            m.bias.copy_(bias)
    return m.to(DEV)


@pytest.mark.parametrize("case", TCONV_CASES, ids=[c["name"] for c in TCONV_CASES])
def test_fixture_through_layer(golden, case):
    _, _, _, _, Ql = _mods()
    g = golden("tconv")
    name = case["name"]
    m = _layer_from_case(Ql, case)
    x = tconv_inputs(case)[0].to(DEV).requires_grad_(True)
    y = m(x)
    _close(y, g[name + ".y"], 1e-4, "y")
    (y * tconv_cotangent(y.shape).to(DEV)).sum().backward()
    _close(x.grad, g[name + ".du"], 1e-4, "du")
    for i, p in enumerate((m.r_weight, m.i_weight, m.j_weight, m.k_weight)):
        _close(p.grad, g[f"{name}.dw{i}"], 1e-4, f"dw{i}")
    if case["bias"]:
        _close(m.bias.grad, g[name + ".dbias"], 1e-4, "dbias")


def test_seeded_layer_forward(golden):
    from oracle.seld_oracle import closed_form_input
    _, _, _, _, Ql = _mods()
    g = golden("tconv")
    c = LAYER_CASE
    np.random.seed(c["np_seed"])
    m = Ql.QuaternionTransposeConv(c["in_channels"], c["out_channels"], c["kernel_size"], c["stride"],
                                   dilatation=c["dilatation"], padding=c["padding"], output_padding=c["output_padding"],
                                   seed=c["seed"]).to(DEV)
    with torch.no_grad():
        y = m(closed_form_input(c["x"]).to(DEV))
    _close(y, g["layer.y"], 1e-4, "layer.y")


# the benchmark shapes of tools/tconv_bench.py, at a smaller batch (the float64 restatement runs on the host)
BENCH_SHAPES = [
    dict(name="up2d", x=(1, 64, 32, 128), cout=64, k=(4, 4), stride=2, padding=1),
    dict(name="up2d_freq", x=(1, 192, 8, 512), cout=192, k=(4, 3), stride=(2, 1), padding=(1, 1)),
    dict(name="up1d", x=(2, 192, 256), cout=192, k=(4,), stride=2, padding=1),
    dict(name="same1d", x=(2, 192, 512), cout=192, k=(3,), stride=1, padding=1),
]


@pytest.mark.parametrize("case", BENCH_SHAPES, ids=[c["name"] for c in BENCH_SHAPES])
def test_bench_shapes_random(case):
    _, _, H, _, _ = _mods()
    gen = torch.Generator().manual_seed(11)
    cin, cout = case["x"][1], case["cout"]
    x = torch.randn(case["x"], generator=gen, dtype=torch.float64)
    ws = [torch.randn((cin // 4, cout // 4) + case["k"], generator=gen, dtype=torch.float64) * 0.05 for _ in range(4)]
    bias = torch.randn(cout, generator=gen, dtype=torch.float64) * 0.1
    xd = x.float().to(DEV).requires_grad_(True)
    wd = [w.float().to(DEV).requires_grad_(True) for w in ws]
    bd = bias.float().to(DEV).requires_grad_(True)
    y = H.hyper_conv_transpose(xd, wd, bd, case["stride"], case["padding"], 0, 1)
    x.requires_grad_(True)
    for w in ws:
        w.requires_grad_(True)
    bias.requires_grad_(True)
    yr = _tconv64(x, ws, bias, case["stride"], case["padding"], 0, 1)
    _close(y, yr, 1e-4, "y")
    cot = torch.randn(yr.shape, generator=gen, dtype=torch.float64)
    (yr * cot).sum().backward()
    (y * cot.float().to(DEV)).sum().backward()
    _close(xd.grad, x.grad, 1e-4, "du")
    for i in range(4):
        _close(wd[i].grad, ws[i].grad, 1e-4, f"dw{i}")
    _close(bd.grad, bias.grad, 1e-4, "dbias")


@pytest.mark.parametrize("nd", [1, 2])
def test_real_algebra(nd):
    _, _, H, _, _ = _mods()
    gen = torch.Generator().manual_seed(5)
    if nd == 1:
        shape, k, s, p, op, d = (3, 6, 13), (5,), 3, 2, 1, 1
    else:
        shape, k, s, p, op, d = (2, 5, 7, 9), (3, 2), (2, 3), (1, 0), (1, 2), (2, 1)
    cout = 7
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    w = torch.randn((shape[1], cout) + k, generator=gen, dtype=torch.float64) * 0.2
    b = torch.randn(cout, generator=gen, dtype=torch.float64)
    fn = F.conv_transpose1d if nd == 1 else F.conv_transpose2d
    x.requires_grad_(True)
    w.requires_grad_(True)
    b.requires_grad_(True)
    yr = fn(x, w, b, s, p, op, 1, d)
    xd = x.detach().float().to(DEV).requires_grad_(True)
    wd = w.detach().float().to(DEV).requires_grad_(True)
    bd = b.detach().float().to(DEV).requires_grad_(True)
    y = H.hyper_conv_transpose(xd, (wd,), bd, s, p, op, d)
    _close(y, yr, 1e-4, "y")
    cot = torch.randn(yr.shape, generator=gen, dtype=torch.float64)
    (yr * cot).sum().backward()
    (y * cot.float().to(DEV)).sum().backward()
    _close(xd.grad, x.grad, 1e-4, "du")
    _close(wd.grad, w.grad, 1e-4, "dw")
    _close(bd.grad, b.grad, 1e-4, "dbias")


@pytest.mark.parametrize("shape,k,s,p,d", [((2, 16, 9, 20), (4, 4), 2, 1, 1), ((2, 8, 6, 7), (3, 3), 3, 1, 2),
                                           ((3, 32, 1, 40), (1, 4), (1, 2), (0, 1), 1)])
def test_phase_kernel_equals_mirrored_data_gradient(shape, k, s, p, d):
    """bias None and output_padding 0: the transposed convolution IS the data gradient of the mirrored convolution."""
    _, L, H, _, _ = _mods()
    gen = torch.Generator().manual_seed(2)
    cin, cout = shape[1], 16
    x = torch.randn(shape, generator=gen).to(DEV)
    ws = [(torch.randn((cin // 4, cout // 4) + k, generator=gen) * 0.1).to(DEV) for _ in range(4)]
    desc, out_pad = H.conv_transpose_desc(shape, cout, 4, k, s, p, 0, d)
    y = H.conv_transpose_fwd(desc, out_pad, x, ws)
    mdesc = H.make_conv_desc(tuple(y.shape), cin, 4, k, s, p, d)
    assert H.conv_out_shape(mdesc) == tuple(shape[2:])
    yd = torch.full_like(y, float("nan"))
    lib = L.lib()
    nbytes = int(lib.seld_hc_conv_bwd_data_workspace(ctypes.byref(mdesc)))
    wsb = torch.empty((nbytes + 3) // 4, device=DEV)
    L.check(lib.seld_hc_conv_bwd_data_ex(ctypes.byref(mdesc), L.ptr(x), L.ptr_array8(ws), L.ptr(yd), L.ptr(wsb), nbytes,
                                         L.current_stream()), "seld_hc_conv_bwd_data_ex")
    _close(y, yd.cpu(), 1e-6, "phase kernel vs mirrored data gradient")


def test_forward_bit_identical_repeat():
    _, _, H, _, _ = _mods()
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(4, 64, 16, 64, generator=gen).to(DEV)
    ws = [(torch.randn(16, 16, 4, 4, generator=gen) * 0.1).to(DEV) for _ in range(4)]
    b = torch.randn(64, generator=gen).to(DEV)
    y1 = H.hyper_conv_transpose(x, ws, b, 2, 1, 0, 1)
    y2 = H.hyper_conv_transpose(x, ws, b, 2, 1, 0, 1)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)


def test_unsupported_descriptors_return_errors():
    _, L, H, _, _ = _mods()
    lib = L.lib()

    def run(desc, out_pad, cin, cout, k, out_shape=(64,)):
        x = torch.zeros(desc.N * cin * desc.in_[0] * desc.in_[1], device=DEV)
        ws = [torch.zeros(max(1, (cin // desc.algebra) * (cout // desc.algebra) * k[0] * k[1]), device=DEV)
              for _ in range(desc.algebra)]
        y = torch.full(out_shape, 7.0, device=DEV)
        rc = lib.seld_hc_conv_transpose_fwd(ctypes.byref(desc), out_pad, L.ptr(x), L.ptr_array8(ws), None, L.ptr(y),
                                            L.current_stream())
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()), "output written by a refused call"
        return rc

    # stride beyond the phase tables
    d, op = H.conv_transpose_desc((1, 4, 3), 4, 4, (1,), 17, 0, 0, 1)
    assert run(d, op, 4, 4, (1, 1)) == EUNSUPPORTED
    # dual quaternion: no transposed form in the reference
    d, op = H.conv_transpose_desc((1, 8, 3), 8, 8, (3,), 2, 0, 0, 1)
    assert run(d, op, 8, 8, (1, 3)) == EUNSUPPORTED
    # groups
    d, op = H.conv_transpose_desc((1, 8, 3), 8, 4, (3,), 2, 0, 0, 1)
    d.groups = 2
    assert run(d, op, 8, 8, (1, 3)) == EUNSUPPORTED
    # output_padding >= stride and >= dilation
    d, op = H.conv_transpose_desc((1, 8, 3), 8, 4, (3,), 2, 0, 2, 1)
    assert run(d, op, 8, 8, (1, 3)) == EINVAL
    # an output image beyond 32-bit addressing
    d, op = H.conv_transpose_desc((1, 64, 1 << 16, 1 << 4), 64, 4, (1, 1), (4, 4), 0, 0, 1)
    assert lib.seld_hc_conv_transpose_fwd(ctypes.byref(d), op, None, None, None, None, None) == EINVAL
    x = torch.zeros(1, device=DEV)
    ws = [torch.zeros(256, device=DEV) for _ in range(4)]
    y = torch.full((64,), 7.0, device=DEV)
    rc = lib.seld_hc_conv_transpose_fwd(ctypes.byref(d), op, L.ptr(x), L.ptr_array8(ws), None, L.ptr(y), L.current_stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED and bool((y == 7.0).all())
    with pytest.raises(L.SeldHipError):
        H.hyper_conv_transpose(torch.zeros(1, 8, 3, device=DEV), [torch.zeros(1, 1, 3, device=DEV)] * 8, None, 2, 0, 0, 1)


def test_recorded_step_equals_eager():
    """QuaternionTransposeConv forward + backward + FlatAdam step recorded with torch.cuda.graph (one stream) and
    replayed once, against the same step run eagerly from the same state."""
    P, _, H, _, Ql = _mods()
    T = P.train
    case = dict(x=(2, 8, 6, 9), cout=12, k=(4, 4), stride=2, padding=1, output_padding=0, dilation=1, bias=True)

    def make():
        m = _layer_from_case(Ql, case)
        return m, T.FlatAdam(m.parameters(), lr=1e-3)
    x = tconv_inputs(case)[0].to(DEV)
    cot = None

    def step(m, opt, xs):
        opt.zero_grad()
        y = m(xs)
        (y * cot).sum().backward()
        opt.step()
        return y

    mE, oE = make()
    with torch.no_grad():
        cot = tconv_cotangent(mE(x).shape).to(DEV)
    yE = step(mE, oE, x).detach().clone()

    mG, oG = make()
    p0 = oG.flat_param.clone()
    xs = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(mG, oG, xs)                                   # warm-up: allocator pools, modules, host caches
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    oG.step_count = 0                                      # the recorded Adam launch is step 1, as the eager one
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yG = step(mG, oG, xs)
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
