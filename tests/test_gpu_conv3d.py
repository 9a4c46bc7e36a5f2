"""3-D convolution and transposed convolution on the MI355X (csrc/hc_conv3d.hip): the reference fixture through the
functional ops and the layers, larger shapes against float64 PyTorch, the 2-D path at kd = D = 1, accumulate semantics,
run-to-run identity, a recorded training step, the kernels a forward + backward launches, and refused descriptors."""
import collections
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.seld_oracle import assemble_conv_weight, closed_form_input
from tests.golden.conv3d_cases import (CONV3D_CASES, LAYER3D_CASES, conv3d_cotangent, conv3d_inputs, rot3d_inputs,
                                       rot3d_variants)
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL, EUNSUPPORTED = -1, -4            # include/seld_hip.h


def _mods():
    P = pkg()
    return P, P._lib, P.hip_ops


def _close(got, ref, tol, what=""):
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= tol * max(ref.abs().max().item(), 1e-30), (what, err, ref.abs().max().item())


def _op(case):
    P = pkg()
    Q, D = P.quaternion.quaternion_ops, P.dual_quaternion.dual_quaternion_ops
    if case["kind"] == "tconv":
        return lambda x, ws, b: Q.quaternion_transpose_conv(x, *ws, b, case["stride"], case["padding"],
                                                            case["output_padding"], 1, case["dilation"])
    if case["algebra"] == 8:
        return lambda x, ws, b: D.dual_quaternion_conv(x, *ws, b, case["stride"], case["padding"], 1, case["dilation"])
    return lambda x, ws, b: Q.quaternion_conv(x, *ws, b, case["stride"], case["padding"], 1, case["dilation"])


def _leaves(x, ws, bias):
    x = x.to(DEV).requires_grad_(True)
    ws = [w.to(DEV).requires_grad_(True) for w in ws]
    bias = bias.to(DEV).requires_grad_(True) if bias is not None else None
    return x, ws, bias


@pytest.mark.parametrize("case", CONV3D_CASES, ids=[c["name"] for c in CONV3D_CASES])
def test_fixture_functional(golden, case):
    g = golden("conv3d")
    name = case["name"]
    x, ws, bias = _leaves(*conv3d_inputs(case))
    y = _op(case)(x, ws, bias)
    (y * conv3d_cotangent(y.shape).to(DEV)).sum().backward()
    _close(y, g[name + ".y"], 1e-4, "y")
    _close(x.grad, g[name + ".dx"], 1e-4, "dx")
    for i, w in enumerate(ws):
        _close(w.grad, g[f"{name}.dw{i}"], 1e-4, f"dw{i}")
    if bias is not None:
        _close(bias.grad, g[name + ".dbias"], 1e-4, "dbias")


@pytest.mark.parametrize("case,name,qformat", rot3d_variants(), ids=[v[1] for v in rot3d_variants()])
def test_rotation_fixture_functional(golden, case, name, qformat):
    Q = pkg().quaternion.quaternion_ops
    g = golden("conv3d")
    x, ws, bias = _leaves(*rot3d_inputs(case, qformat))
    if case["kind"] == "conv":
        y = Q.quaternion_conv_rotation(x, *ws, bias, case["stride"], case["padding"], 1, case["dilation"], qformat)
    else:
        y = Q.quaternion_transpose_conv_rotation(x, *ws, bias, case["stride"], case["padding"], case["output_padding"],
                                                 1, case["dilation"], qformat)
    (y * conv3d_cotangent(y.shape).to(DEV)).sum().backward()
    _close(y, g[name + ".y"], 1e-4, "y")
    _close(x.grad, g[name + ".dx"], 1e-4, "dx")
    for c, w in zip("rijk", ws):
        _close(w.grad, g[f"{name}.d{c}"], 1e-4, c)
    _close(bias.grad, g[name + ".dbias"], 1e-4, "dbias")


def _seeded_layer(c):
    P = pkg()
    mod = P.dual_quaternion.dual_quaternion_layers if c["cls"].startswith("Dual") else P.quaternion.quaternion_layers
    np.random.seed(c["np_seed"])
    return getattr(mod, c["cls"])(**c["kwargs"]).to(DEV)


@pytest.mark.parametrize("c", LAYER3D_CASES, ids=[c["name"] for c in LAYER3D_CASES])
def test_fixture_through_layer(golden, c):
    g = golden("conv3d")
    name = c["name"]
    m = _seeded_layer(c)
    x = closed_form_input(c["x"]).to(DEV).requires_grad_(True)
    y = m(x)
    _close(y, g[name + ".y"], 1e-4, "y")
    (y * conv3d_cotangent(y.shape).to(DEV)).sum().backward()
    _close(x.grad, g[name + ".dx"], 1e-4, "dx")
    for k, p in m.named_parameters():
        if p.requires_grad:
            _close(p.grad, g[f"{name}.grad.{k}"], 1e-4, k)


# x, Cout, kernel, stride, padding, dilation, algebra, kind, output_padding: many tiles, edge workgroups, Cout not a
# multiple of the channel tile, 24 dual-quaternion block channels, strides 2 and 3
LARGE = [
    dict(x=(2, 64, 6, 20, 23), cout=48, k=3, s=1, p=1, d=1, A=4, kind="conv"),
    dict(x=(2, 32, 7, 17, 30), cout=80, k=(3, 3, 3), s=(2, 2, 2), p=1, d=1, A=4, kind="conv"),
    dict(x=(1, 48, 9, 16, 19), cout=36, k=(3, 1, 3), s=(3, 1, 3), p=(1, 0, 2), d=(1, 1, 2), A=4, kind="conv"),
    dict(x=(1, 192, 4, 9, 10), cout=192, k=3, s=1, p=1, d=1, A=8, kind="conv"),
    dict(x=(2, 128, 5, 8, 9), cout=64, k=(3, 3, 1), s=(2, 1, 2), p=(1, 1, 0), d=1, A=8, kind="conv"),
    dict(x=(2, 64, 4, 8, 8), cout=48, k=4, s=2, p=1, d=1, A=4, kind="tconv", op=0),
    dict(x=(1, 32, 3, 7, 6), cout=40, k=(3, 2, 3), s=(3, 2, 3), p=(0, 1, 1), d=1, A=4, kind="tconv", op=(2, 1, 0)),
    dict(x=(2, 24, 5, 6, 7), cout=24, k=3, s=1, p=1, d=(1, 2, 1), A=1, kind="conv"),
    dict(x=(1, 20, 4, 5, 6), cout=12, k=3, s=2, p=0, d=1, A=1, kind="tconv", op=1),
]


@pytest.mark.parametrize("c", LARGE, ids=[f"{c['kind']}{c['A']}_{'x'.join(map(str, c['x']))}" for c in LARGE])
def test_large_shapes_against_float64(c):
    _, _, H = _mods()
    gen = torch.Generator().manual_seed(11)
    A, cin, cout = c["A"], c["x"][1], c["cout"]
    k = c["k"] if isinstance(c["k"], tuple) else (c["k"],) * 3
    wshape = ((cout // A, cin // A) if c["kind"] == "conv" else (cin // A, cout // A)) + k
    x = torch.randn(c["x"], generator=gen)
    ws = [torch.randn(wshape, generator=gen) * 0.1 for _ in range(A)]
    b = torch.randn(cout, generator=gen)
    x64 = x.double().requires_grad_(True)
    ws64 = [w.double().requires_grad_(True) for w in ws]
    b64 = b.double().requires_grad_(True)
    M = assemble_conv_weight(ws64)
    if c["kind"] == "conv":
        y64 = F.conv3d(x64, M, b64, c["s"], c["p"], c["d"])
    else:
        y64 = F.conv_transpose3d(x64, M, b64, c["s"], c["p"], c["op"], 1, c["d"])
    cot = torch.randn(y64.shape, generator=gen)
    (y64 * cot.double()).sum().backward()

    xd, wsd, bd = _leaves(x, ws, b)
    if c["kind"] == "conv":
        y = H.hyper_conv(xd, wsd, bd, c["s"], c["p"], c["d"])
    else:
        y = H.hyper_conv_transpose(xd, wsd, bd, c["s"], c["p"], c["op"], c["d"])
    (y * cot.to(DEV)).sum().backward()
    _close(y, y64.detach(), 1e-4, "y")
    _close(xd.grad, x64.grad, 1e-4, "dx")
    for i, (w, w64) in enumerate(zip(wsd, ws64)):
        _close(w.grad, w64.grad, 1e-4, f"dw{i}")
    _close(bd.grad, b64.grad, 1e-4, "dbias")


@pytest.mark.parametrize("A", [4, 8])
def test_depth_one_equals_2d_path(A):
    _, _, H = _mods()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 1, 12, 14, generator=gen)
    ws = [torch.randn(24 // A, 16 // A, 1, 3, 3, generator=gen) * 0.2 for _ in range(A)]
    b = torch.randn(24, generator=gen)
    cot = torch.randn(2, 24, 1, 6, 7, generator=gen).to(DEV)
    x3, ws3, b3 = _leaves(x, ws, b)
    y3 = H.hyper_conv(x3, ws3, b3, (1, 2, 2), (0, 1, 1), 1)
    (y3 * cot).sum().backward()
    x2, ws2, b2 = _leaves(x.squeeze(2), [w.squeeze(2) for w in ws], b)
    y2 = H.hyper_conv(x2, ws2, b2, 2, 1, 1)
    (y2 * cot.squeeze(2)).sum().backward()
    _close(y3.squeeze(2), y2, 1e-5, "y")
    _close(x3.grad.squeeze(2), x2.grad, 1e-5, "dx")
    for w3, w2 in zip(ws3, ws2):
        _close(w3.grad.squeeze(2), w2.grad, 1e-5, "dw")
    _close(b3.grad, b2.grad, 1e-5, "dbias")


@pytest.mark.parametrize("kind", ["conv", "tconv"])
def test_weight_gradient_accumulates(kind):
    _, _, H = _mods()
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, 16, 5, 6, 7, generator=gen).to(DEV)
    ws = [(torch.randn(4, 4, 3, 3, 3, generator=gen) * 0.2).to(DEV) for _ in range(4)]
    if kind == "conv":
        desc, op = H.make_conv3d_desc(tuple(x.shape), 16, 4, 3, 2, 1, 1), None
    else:
        desc, op = H.conv3d_transpose_desc(tuple(x.shape), 16, 4, 3, 2, 1, 1, 1)
    dy = torch.randn((2, 16) + H.conv3d_out_shape(desc, op), generator=gen).to(DEV)
    fresh = [torch.zeros_like(w) for w in ws]
    fb = torch.zeros(16, device=DEV)
    H.conv3d_bwd_weight_acc(desc, op, x, dy, fresh, fb)
    pre = [torch.full_like(w, 0.5 + i) for i, w in enumerate(ws)]
    pb = torch.full((16,), -2.0, device=DEV)
    acc = [t.clone() for t in pre]
    ab = pb.clone()
    H.conv3d_bwd_weight_acc(desc, op, x, dy, acc, ab)
    torch.cuda.synchronize()
    assert fresh[0].abs().max().item() > 0 and fb.abs().max().item() > 0
    for a, p, f in zip(acc, pre, fresh):
        _close(a - p, f, 1e-5, "dw")
    _close(ab - pb, fb, 1e-5, "dbias")


def _net(Ql, Dl):
    torch.manual_seed(0)
    np.random.seed(3)
    return torch.nn.Sequential(
        Ql.QuaternionConv(8, 16, 3, 1, padding=1, seed=1, operation='convolution3d'),
        Dl.DualQuaternionConv(16, 16, (1, 3, 3), (1, 2, 2), padding=(0, 1, 1), seed=2, operation='convolution3d'),
        Ql.QuaternionTransposeConv(16, 8, 3, (1, 2, 2), padding=1, output_padding=(0, 1, 1), seed=3,
                                   operation='convolution3d')).to(DEV)


def _fwd_bwd(m, x, cot):
    y = m(x)
    (y * cot).sum().backward()
    return y


@pytest.mark.parametrize("det", ["0", "1"])
def test_forward_backward_bit_identical(seld_env, det):
    P, _, _ = _mods()
    seld_env.set("SELD_DETERMINISTIC", det)
    m = _net(P.quaternion.quaternion_layers, P.dual_quaternion.dual_quaternion_layers)
    x = closed_form_input((2, 8, 4, 10, 12)).to(DEV)
    with torch.no_grad():
        cot = conv3d_cotangent(m(x).shape).to(DEV)
    outs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        y = _fwd_bwd(m, xr, cot)
        torch.cuda.synchronize()
        outs.append([y.detach().clone(), xr.grad.clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None])
    assert len(outs[0]) == len(outs[1]) > 2
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_recorded_step_equals_eager():
    """Q conv -> DQ conv -> Q transposed conv + FlatAdam, one training step recorded with torch.cuda.graph (one stream)
    and replayed once, against the same step run eagerly from the same state."""
    P, _, _ = _mods()
    T = P.train
    Ql, Dl = P.quaternion.quaternion_layers, P.dual_quaternion.dual_quaternion_layers

    def make():
        m = _net(Ql, Dl)
        return m, T.FlatAdam(m.parameters(), lr=1e-3)
    x = closed_form_input((2, 8, 4, 10, 12)).to(DEV)
    cot = None

    def step(m, opt, xs):
        opt.zero_grad()
        y = m(xs)
        (y * cot).sum().backward()
        opt.step()
        return y

    mE, oE = make()
    with torch.no_grad():
        cot = conv3d_cotangent(mE(x).shape).to(DEV)
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
    assert oE.flat_grad.abs().max().item() > 0


@pytest.mark.parametrize("direct", [True, False], ids=["optimiser_slots", "autograd"])
def test_forward_backward_issues_only_library_kernels(direct):
    from torch.profiler import ProfilerActivity, profile
    P, _, H = _mods()
    m = _net(P.quaternion.quaternion_layers, P.dual_quaternion.dual_quaternion_layers)
    opt = P.train.FlatAdam(m.parameters(), lr=1e-3) if direct else None
    x = closed_form_input((2, 8, 4, 10, 12)).to(DEV)
    with torch.no_grad():
        cot = conv3d_cotangent(m(x).shape).to(DEV)

    def run():
        if opt is not None:
            opt.zero_grad()
        else:
            m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            m(x).backward(cot)
            torch.cuda.synchronize()
        return collections.Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    run()
    names = run()
    foreign = {k: v for k, v in names.items() if "seld::" not in k}
    assert not foreign, foreign
    first = H.make_conv3d_desc((2, 8, 4, 10, 12), 16, 4, 3, 1, 1, 1)          # the first layer's forward
    labels = [H.conv3d_label(first, None, 0), H.conv3d_label(first, None, 2), "hc_conv3d_fold_kernel",
              "hc_conv3d_phase_kernel"]
    for lab in labels:
        assert any(lab in k for k in names), (lab, names)


def test_refused_descriptors_launch_nothing():
    from torch.profiler import ProfilerActivity, profile
    _, L, H = _mods()
    lib = L.lib()
    x = torch.zeros(4096, device=DEV)
    ws = [torch.zeros(4096, device=DEV) for _ in range(8)]
    y = torch.full((4096,), 7.0, device=DEV)
    three = ctypes.c_int32 * 3
    cases = [
        (H.make_conv3d_desc((1, 8, 40, 4, 4), 8, 4, 1, (17, 1, 1), 0, 1), None, EUNSUPPORTED),      # stride > 16
        (H.make_conv3d_desc((1, 8, 4, 4, 4), 8, 4, 3, 1, 1, 1, groups=2), None, EUNSUPPORTED),
        (H.make_conv3d_desc((1, 6, 4, 4, 4), 8, 4, 3, 1, 1, 1), None, EINVAL),
        (H.conv3d_transpose_desc((1, 8, 4, 4, 4), 8, 4, 3, 2, 1, 0, 1)[0], three(0, 2, 0), EINVAL),  # out_pad rule
        (H.conv3d_transpose_desc((1, 8, 4, 4, 4), 8, 8, 3, 2, 1, 0, 1)[0], three(0, 0, 0), EUNSUPPORTED),  # DQ
    ]
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for desc, op, want in cases:
            st = L.current_stream()
            if op is None:
                rcs = [lib.seld_hc_conv3d_fwd(ctypes.byref(desc), L.ptr(x), L.ptr_array8(ws), None, L.ptr(y), st),
                       lib.seld_hc_conv3d_bwd_data(ctypes.byref(desc), L.ptr(x), L.ptr_array8(ws), L.ptr(y), st),
                       lib.seld_hc_conv3d_bwd_weight_acc(ctypes.byref(desc), L.ptr(x), L.ptr(x), L.ptr_array8([y] * 8),
                                                         L.ptr(y), L.ptr(x), 1 << 14, st)]
            else:
                rcs = [lib.seld_hc_conv3d_transpose_fwd(ctypes.byref(desc), op, L.ptr(x), L.ptr_array8(ws), None,
                                                        L.ptr(y), st),
                       lib.seld_hc_conv3d_transpose_bwd_data(ctypes.byref(desc), op, L.ptr(x), L.ptr_array8(ws),
                                                             L.ptr(y), st),
                       lib.seld_hc_conv3d_transpose_bwd_weight_acc(ctypes.byref(desc), op, L.ptr(x), L.ptr(x),
                                                                   L.ptr_array8([y] * 8), L.ptr(y), L.ptr(x), 1 << 14,
                                                                   st)]
            assert rcs == [want] * 3, (rcs, want)
        # a valid descriptor with too small a workspace
        desc = H.make_conv3d_desc((1, 8, 4, 4, 4), 8, 4, 3, 1, 1, 1)
        assert lib.seld_hc_conv3d_bwd_weight_acc(ctypes.byref(desc), L.ptr(x), L.ptr(x), L.ptr_array8([y] * 4),
                                                 L.ptr(y), L.ptr(x), 4, L.current_stream()) == -2
        torch.cuda.synchronize()
    launched = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    assert not launched, launched
    assert bool((y == 7.0).all()), "output written by a refused call"
    Q = pkg().quaternion.quaternion_ops
    with pytest.raises(L.SeldHipError):          # groups
        Q.quaternion_conv(torch.zeros(1, 8, 4, 4, 4, device=DEV), *[torch.zeros(2, 1, 3, 3, 3, device=DEV)] * 4, None,
                          1, 1, 2, 1)
    with pytest.raises(L.SeldHipError):          # component tensors that do not match the input's channels
        H.hyper_conv(torch.zeros(1, 8, 4, 4, 4, device=DEV), [torch.zeros(2, 1, 3, 3, 3, device=DEV)] * 4, None, 1, 1,
                     1)
