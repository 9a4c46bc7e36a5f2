"""Depthwise convolution on the MI355X (csrc/dwconv.hip): the reference fixture through DepthwiseSeparableConv2D / 1D in
train and eval mode, a functional sweep and a full-size case against float64 PyTorch, accumulate semantics, run-to-run
identity, the hip_nn convolution modules, a recorded training step, and refused descriptors."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests.golden.depthwise_cases import (DEPTHWISE_CASES, PARAMS, depthwise_cotangent, depthwise_input)
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4            # include/seld_hip.h


def _close(got, ref, tol, what="", scale=0.0):
    """max |got - ref| <= tol * max(max |ref|, scale); returns the error."""
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= tol * max(ref.abs().max().item(), scale, 1e-30), (what, err, ref.abs().max().item())
    return err


@pytest.mark.parametrize("case", DEPTHWISE_CASES, ids=[c["name"] for c in DEPTHWISE_CASES])
def test_fixture_through_layer(golden, case):
    g = golden("depthwise")
    name = case["name"]
    DL = pkg().dual_quaternion.dual_quaternion_layers
    torch.manual_seed(case["seed"])
    layer = getattr(DL, "DepthwiseSeparableConv" + case["cls"])(*case["args"]).to(DEV).train()
    x = depthwise_input(case).to(DEV).requires_grad_(True)
    y = layer(x)
    (y * depthwise_cotangent(y.shape).to(DEV)).sum().backward()
    # the layer's output and dx pass through train-mode BatchNorm, which scales float32 rounding by 1/std (d1_k3_s1_p0:
    # batch variance ~1.5e-3, dx off by 1.0e-4 of max |ref|): 1e-3 here; the depthwise op alone is held to 1e-5 below
    _close(y, g[name + ".y"], 1e-3, "y")
    _close(x.grad, g[name + ".dx"], 1e-3, "dx")
    params = dict(layer.named_parameters())
    # the two convolution biases feed a BatchNorm in train mode, so their exact gradients vanish (|ref| ~ 1e-14): they
    # are held to the scale of the layer's other parameter gradients, where float32 cancellation leaves ~1e-6; all
    # gradients here come through the BatchNorm's 1/std like dx (d1_k3_s1_p0: depthwise.weight off by 7e-4 of max |ref|)
    scale = max(float(abs(g[f"{name}.grad.{k}"]).max()) for k in PARAMS)
    for k in PARAMS:
        _close(params[k].grad, g[f"{name}.grad.{k}"], 1e-3, k, scale if k.endswith(".bias") else 0.0)
    _close(layer.bn.running_mean, g[name + ".train.bn.running_mean"], 1e-5, "running_mean")
    _close(layer.bn.running_var, g[name + ".train.bn.running_var"], 1e-5, "running_var")
    assert int(layer.bn.num_batches_tracked) == 1
    layer.eval()
    with torch.no_grad():
        _close(layer(x.detach()), g[name + ".y_eval"], 1e-4, "y_eval")


def _run(x, w, b, stride, padding, dilation, cot_seed=0):
    """depthwise_conv forward + backward on the device; returns y, dx, dw, dbias (float32, host)."""
    H = pkg().hip_ops
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if b is not None else None
    y = H.depthwise_conv(xd, wd, bd, stride, padding, dilation)
    cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(cot_seed)).to(DEV)
    y.backward(cot)
    return y, xd.grad, wd.grad, (bd.grad if bd is not None else None), cot


def _reference(x, w, b, stride, padding, dilation, cot):
    conv = F.conv2d if x.dim() == 4 else F.conv1d
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if b is not None else None
    y = conv(xr, wr, br, stride, padding, dilation, x.shape[1])
    y.backward(cot.double().cpu())
    return y, xr.grad, wr.grad, (br.grad if br is not None else None)


def _check(x, w, b, stride, padding, dilation, tol_w=1e-5):
    got = _run(x, w, b, stride, padding, dilation)
    ref = _reference(x, w, b, stride, padding, dilation, got[4])
    errs = [_close(got[0], ref[0], 1e-5, "y"), _close(got[1], ref[1], 1e-5, "dx"), _close(got[2], ref[2], tol_w, "dw")]
    if b is not None:
        errs.append(_close(got[3], ref[3], tol_w, "dbias"))
    return errs


def _sweep():
    cases = []
    # (x shape, m, kernel, stride, padding, dilation)
    for k, s, d in itertools.product([1, 2, 3, 5, 7, (1, 3), (3, 1), (5, 3)], [1, 2, 3, (2, 1)], [1, 2]):
        kk = (k, k) if isinstance(k, int) else k
        for pmode in ("0", "half", "km1"):
            p = {"0": 0, "half": (kk[0] // 2, kk[1] // 2), "km1": (kk[0] - 1, kk[1] - 1)}[pmode]
            cases.append(((2, 3, 13, 21), 1, k, s, p, d))
    for m, C, N in itertools.product([1, 2, 3], [1, 3, 64, 67], [1, 4]):
        cases.append(((N, C, 9, 70), m, 3, 1, 1, 1))
        cases.append(((N, C, 10, 35), m, (3, 5), 2, (1, 2), 1))
    for T, k, s, p, d in [(17, 3, 1, 1, 1), (333, 5, 2, 2, 1), (1029, 7, 1, 3, 2), (64, 4, 3, 0, 1), (5, 5, 1, 0, 1)]:
        for m in (1, 2):
            cases.append(((3, 5, T), m, k, s, p, d))
    cases.append(((2, 4, 3, 3), 1, 3, 1, 0, 1))                     # output 1 x 1
    cases.append(((2, 4, 257, 1030), 2, 3, 1, 1, 1))                # widths past one tile
    cases.append(((1, 2, 40, 40), 1, (15, 15), 1, 0, (2, 2)))       # window past the LDS budget
    return cases


SWEEP = _sweep()


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_sweep_against_float64(bias):
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for xs, m, k, s, p, d in SWEEP:
        C = xs[1]
        nd = len(xs) - 2
        kk = ((k, k) if isinstance(k, int) else k) if nd == 2 else ((k,) if isinstance(k, int) else (k[1],))
        if nd == 1 and (isinstance(s, tuple) or isinstance(p, tuple)):
            continue
        x = torch.randn(xs, generator=gen)
        w = torch.randn((m * C, 1) + tuple(kk), generator=gen) * 0.3
        b = torch.randn(m * C, generator=gen) if bias else None
        try:
            errs = _check(x, w, b, s, p, d)
        except AssertionError as e:
            raise AssertionError(f"case {(xs, m, k, s, p, d)}: {e}") from None
        worst = max([worst] + errs)
    print(f"depthwise sweep: {len(SWEEP)} cases, worst absolute error {worst:.3e}")


def test_full_size_against_float64():
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((32, 64, 128, 512), generator=gen)
    w = torch.randn((64, 1, 3, 3), generator=gen) * 0.3
    b = torch.randn(64, generator=gen)
    errs = _check(x, w, b, 1, 1, 1, tol_w=1e-4)
    print("full size (32, 64, 128, 512) 3x3: |err| y %.2e dx %.2e dw %.2e dbias %.2e" % tuple(errs))


def test_weight_gradient_accumulates():
    _, L, H = pkg(), pkg()._lib, pkg().hip_ops
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, 6, 11, 17, generator=gen).to(DEV)
    desc = H.make_dwconv_desc(tuple(x.shape), 12, 3, 2, 1, 1)
    dy = torch.randn((2, 12) + H.dwconv_out_shape(desc), generator=gen).to(DEV)
    fresh, fb = torch.zeros(12, 1, 3, 3, device=DEV), torch.zeros(12, device=DEV)
    H.dwconv_bwd_weight_acc(desc, x, dy, fresh, fb)
    acc, ab = torch.full((12, 1, 3, 3), 0.5, device=DEV), torch.full((12,), -2.0, device=DEV)
    H.dwconv_bwd_weight_acc(desc, x, dy, acc, ab)
    torch.cuda.synchronize()
    assert fresh.abs().max().item() > 0 and fb.abs().max().item() > 0
    _close(acc - 0.5, fresh, 1e-6, "dw")
    _close(ab + 2.0, fb, 1e-6, "dbias")
    # through autograd: a second backward adds to .grad
    w = torch.randn(12, 1, 3, 3, generator=gen).to(DEV).requires_grad_(True)
    b = torch.randn(12, generator=gen).to(DEV).requires_grad_(True)
    H.depthwise_conv(x, w, b, 2, 1, 1).backward(dy)
    g1, gb1 = w.grad.clone(), b.grad.clone()
    H.depthwise_conv(x, w, b, 2, 1, 1).backward(dy)
    _close(w.grad, 2 * g1, 1e-6, "dw twice")
    _close(b.grad, 2 * gb1, 1e-6, "dbias twice")


def test_bit_identical_repeats():
    gen = torch.Generator().manual_seed(9)
    x = torch.randn((4, 64, 64, 200), generator=gen)
    w = torch.randn((128, 1, 3, 3), generator=gen)
    b = torch.randn(128, generator=gen)
    a = _run(x, w, b, 2, 1, 1)
    c = _run(x, w, b, 2, 1, 1)
    for u, v in zip(a[:4], c[:4]):
        assert torch.equal(u, v)


def test_hip_nn_modules_equal_torch():
    P = pkg()
    hnn, L = P.hip_nn, P._lib
    gen = torch.Generator().manual_seed(10)
    C = 16
    for mod, ref, xs in [(hnn.Conv2d(C, C, 3, groups=C), torch.nn.Conv2d(C, C, 3, groups=C), (2, C, 20, 30)),
                         (hnn.Conv1d(C, 2 * C, 5, groups=C), torch.nn.Conv1d(C, 2 * C, 5, groups=C), (2, C, 50))]:
        ref.load_state_dict(mod.state_dict())
        x = torch.randn(xs, generator=gen)
        y = mod.to(DEV)(x.to(DEV))
        _close(y, ref.double()(x.double()), 1e-5, type(mod).__name__)
    with pytest.raises(L.SeldHipError):
        hnn.Conv2d(8, 8, 3, groups=2).to(DEV)(torch.zeros(1, 8, 6, 6, device=DEV))


def _separable_net():
    DL = pkg().dual_quaternion.dual_quaternion_layers
    torch.manual_seed(2)
    return torch.nn.Sequential(DL.DepthwiseSeparableConv2D(8, 16, 3, padding=1),
                               DL.DepthwiseSeparableConv2D(16, 16, 5, stride=2, padding=2)).to(DEV)


def test_recorded_training_steps_equal_eager():
    """DepthwiseSeparableConv2D x 2 + FlatAdam: three steps run eagerly against one step recorded with torch.cuda.graph
    and replayed three times, the step number and learning rate taken from the device-resident step state as
    GraphedTrainStep does."""
    import numpy as np
    T = pkg().train
    x = depthwise_input(dict(x=(4, 8, 24, 40))).to(DEV)
    with torch.no_grad():
        cot = depthwise_cotangent(_separable_net()(x).shape).to(DEV)

    def make():
        m = _separable_net()
        return m, T.FlatAdam(m.parameters(), lr=1e-3)

    def step(m, opt, xs, state=None):
        opt.zero_grad(state=state)
        y = m(xs)
        (y * cot).sum().backward()
        opt.step(state=state)
        return y

    mE, oE = make()
    for _ in range(3):
        yE = step(mE, oE, x).detach().clone()

    mG, oG = make()
    p0 = oG.flat_param.clone()
    bufs0 = [b.clone() for b in mG.buffers()]
    xs = x.clone()
    state = torch.zeros(4, device=DEV, dtype=torch.int64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(mG, oG, xs)                                   # warm-up: allocator pools, modules, host caches
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yG = step(mG, oG, xs, state)
    with torch.no_grad():                                  # back to the state the eager steps started from
        oG.flat_param.copy_(p0)
        oG.exp_avg.zero_()
        oG.exp_avg_sq.zero_()
        for b, b0 in zip(mG.buffers(), bufs0):
            b.copy_(b0)
        state.copy_(torch.tensor([0, 0, int(np.float32(1e-3).view(np.uint32)), 0], dtype=torch.int64))
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    _close(yG, yE, 1e-5, "y")
    _close(oG.flat_grad, oE.flat_grad, 1e-5, "gradients")
    # the convolution biases in front of a BatchNorm have gradients of pure rounding noise, which Adam normalises to
    # +-lr a step: they are only held to their range; every other parameter must agree
    for (n, pG), (_, pE) in zip(mG.named_parameters(), mE.named_parameters()):
        if n.endswith(("depthwise.bias", "pointwise.bias")):
            assert (pG - pE).abs().max().item() <= 6e-3 + 1e-6, n
        else:
            _close(pG, pE, 1e-5, n)
    # running_mean carries those biases (momentum 0.1): held to 0.1 * their range
    for bG, bE in zip(mG.buffers(), mE.buffers()):
        assert (bG.double() - bE.double()).abs().max().item() <= 1e-5 * bE.double().abs().max().item() + 6e-4
    assert int(state[1]) == 3
    assert not torch.equal(oG.flat_param, p0)


def test_refused_descriptors_launch_nothing():
    from torch.profiler import ProfilerActivity, profile
    L, H = pkg()._lib, pkg().hip_ops
    lib = L.lib()
    x = torch.zeros(1 << 16, device=DEV)
    y = torch.full((1 << 16,), 7.0, device=DEV)
    cases = []
    d = H.make_dwconv_desc((2, 8, 16, 16), 16, 3, 1, 1, 1)
    d.groups = 4
    cases.append((d, EINVAL))
    cases.append((H.make_dwconv_desc((2, 8, 16, 16), 12, 3, 1, 1, 1), EINVAL))
    cases.append((H.make_dwconv_desc((2, 8, 32, 32), 8, 16, 1, 0, 1), EUNSUPPORTED))
    cases.append((H.make_dwconv_desc((1, 64, 2048, 2048), 64, 1, 1, 0, 1), EUNSUPPORTED))
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for desc, want in cases:
            st = L.current_stream()
            rcs = [lib.seld_dwconv_fwd(ctypes.byref(desc), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(y), st),
                   lib.seld_dwconv_bwd_data(ctypes.byref(desc), L.ptr(x), L.ptr(x), L.ptr(y), st),
                   lib.seld_dwconv_bwd_weight_acc(ctypes.byref(desc), L.ptr(x), L.ptr(x), L.ptr(y), L.ptr(y), L.ptr(x),
                                                  1 << 16, st)]
            assert rcs == [want] * 3, (rcs, want)
        ok = H.make_dwconv_desc((2, 8, 16, 16), 16, 3, 1, 1, 1)
        assert lib.seld_dwconv_bwd_weight_acc(ctypes.byref(ok), L.ptr(x), L.ptr(x), L.ptr(y), L.ptr(y), L.ptr(x), 4,
                                              L.current_stream()) == EWORKSPACE
        torch.cuda.synchronize()
    launched = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    assert not launched, launched
    assert bool((y == 7.0).all()), "output written by a refused call"
