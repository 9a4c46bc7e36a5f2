"""The depthwise convolution kernels (csrc/dwconv.hip) on the MI355X against float64 F.conv1d / F.conv2d with groups = C,
EXACTLY: with integer inputs in [-2, 2], weights in {-1, 0, 1} and integer biases every float32 operation of the kernels
is exact in any order (tests/dwconv_exact.py), so every result must hold the oracle's integers bit for bit.  Cases:
tests/golden/dwconv_exact_cases.py -- one per plan (entry point, nr, div, staged, WC, candidate) of a search grid, plus
edge shapes.  Every test first asserts the labels the library reports and the restated plan behind them.

  A  the three C entry points: sources as views inside NaN-filled buffers, once 16-byte aligned (16-byte staging loads
     where the source width is a multiple of 4) and once 4 bytes off (scalar staging); outputs as NaN-prefilled views
     inside sentinel-filled buffers; the data gradient exactly 0.0 where no output reads the input; the weight gradient
     accumulating into quarter-valued slots, twice with identical bits, with and without the bias gradient
  B  depthwise_conv under autograd
  C  the case list once more with randn inputs at test_gpu_depthwise.py's 1e-5 of max|ref|; prints the worst ratio"""
import ctypes

import pytest
import torch

from tests import dwconv_exact as X
from tests.golden import dwconv_exact_cases as C
from tests.helpers import pkg
from tests.test_dwconv_exact_host import library_labels

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDS = [c["name"] for c in C.ALL_CASES]
REL = 1e-5                                  # tests/test_gpu_depthwise.py: of max|ref|


def _enter(case):
    P = pkg()
    assert library_labels(P, case) == case["labels"], case["name"]
    assert all(X.plan_key(case, w) == tuple(case["plans"][w]) for w in (0, 1, 2)), case["name"]
    return P, P.hip_ops, P._lib


def _source(t, band, shift):
    """A contiguous copy of `t` inside a NaN-filled buffer, `shift` floats past a 512-byte aligned address."""
    band = (band + 127) // 128 * 128
    buf = torch.full((2 * band + t.numel() + shift,), float("nan"), device=DEV)
    view = buf[band + shift:band + shift + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * shift
    return view


class Outputs:
    def __init__(self, case):
        self.band, self.held = X.guard_band(case), []

    def new(self, shape, fill=float("nan")):
        view, buf, b = X.sentinel_output(tuple(shape), self.band, DEV)
        view.fill_(fill)
        self.held.append((buf, b))
        return view

    def check(self, what):
        torch.cuda.synchronize()
        for i, (buf, b) in enumerate(self.held):
            X.assert_band_intact(f"{what} output {i}", buf, b)


def _bias_ref(y, bias):
    return y + bias.double().view(1, -1, *([1] * (y.dim() - 2)))


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_plain_launches_exact(case):
    P, H, L = _enter(case)
    lib, st, name = L.lib(), L.current_stream(), case["name"]
    d = X.desc(H, case)
    host, r, out = X.inputs(case), X.exact_oracle(case), Outputs(case)
    w, bias = host["w"].to(DEV), host["bias"].to(DEV)
    band = X.guard_band(case)
    unread = (~X.read_mask(case)).to(DEV)
    if X.ndim(case) == 1:
        unread = unread[0]
    ref = ctypes.byref(d)
    for shift in (0, 1):
        how = "aligned source" if shift == 0 else "source 4 bytes off"
        x, dy = _source(host["x"].to(DEV), band, shift), _source(host["dy"].to(DEV), band, shift)
        for b in (None, bias):
            y = out.new(X.y_shape(case))
            L.check(lib.seld_dwconv_fwd(ref, L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), st), "seld_dwconv_fwd")
            X.assert_exact(f"{name} forward ({case['labels'][0]}), {how}, bias {b is not None}", y,
                           r["y"] if b is None else _bias_ref(r["y"], host["bias"]))
        dx = out.new(case["x"])
        L.check(lib.seld_dwconv_bwd_data(ref, L.ptr(dy), L.ptr(w), L.ptr(dx), st), "seld_dwconv_bwd_data")
        X.assert_exact(f"{name} data gradient ({case['labels'][1]}), {how}", dx, r["dx"])
        assert bool((dx[..., unread] == 0.0).all()), f"{name}: input samples no output reads, {how}"
        runs = []
        for _ in range(2):
            dw, db = out.new(X.weight_shape(case), X.FILL), out.new((X.cout(case),), 0.75)
            H.dwconv_bwd_weight_acc(d, x, dy, dw, db)
            X.assert_exact(f"{name} weight gradient ({case['labels'][2]}), {how}", dw, r["dw"] + X.FILL)
            X.assert_exact(f"{name} bias gradient, {how}", db, r["db"] + 0.75)
            runs.append((dw, db))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), f"{name}: two runs, identical bits"
        dw = out.new(X.weight_shape(case), 0.0)
        H.dwconv_bwd_weight_acc(d, x, dy, dw, None)
        X.assert_exact(f"{name} weight gradient without the bias gradient, {how}", dw, r["dw"])
    x, dy = host["x"].to(DEV), host["dy"].to(DEV)
    X.assert_exact(f"{name} dwconv_fwd", H.dwconv_fwd(d, x, w, bias), _bias_ref(r["y"], host["bias"]))
    X.assert_exact(f"{name} dwconv_bwd_data", H.dwconv_bwd_data(d, dy, w, tuple(case["x"])), r["dx"])
    out.check(name)


# ---- B ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_autograd_entry_point_exact(case):
    P, H, L = _enter(case)
    name = case["name"]
    host, r = X.inputs(case), X.exact_oracle(case)
    x = host["x"].to(DEV).requires_grad_(True)
    w = host["w"].to(DEV).requires_grad_(True)
    bias = host["bias"].to(DEV).requires_grad_(True)
    y = H.depthwise_conv(x, w, bias, case["stride"], case["padding"], case["dilation"])
    y.backward(host["dy"].to(DEV))
    torch.cuda.synchronize()
    X.assert_exact(f"{name} y", y, _bias_ref(r["y"], host["bias"]))
    X.assert_exact(f"{name} x.grad", x.grad, r["dx"])
    X.assert_exact(f"{name} w.grad", w.grad, r["dw"])
    X.assert_exact(f"{name} bias.grad", bias.grad, r["db"])


# ---- C ---------------------------------------------------------------------------------------------------------------------
_worst = {"ratio": 0.0, "what": ""}


def _check(what, got, ref):
    g, w = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == w.shape, (what, tuple(g.shape), tuple(w.shape))
    err, scale = float((g - w).abs().max()), max(float(w.abs().max()), 1e-6)
    if err / scale > _worst["ratio"]:
        _worst["ratio"], _worst["what"] = err / scale, what
    print(f"{what}: max err {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e} (bound {REL:.0e}); "
          f"worst so far {_worst['ratio']:.2e} ({_worst['what']})")
    assert err <= REL * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_plain_launches_rounding(case):
    P, H, L = _enter(case)
    name = case["name"]
    host = X.inputs(case, "randn")
    r = X.oracle(case, host)
    t = {k: v.to(DEV) for k, v in host.items()}
    d = X.desc(H, case)
    _check(f"{name} forward", H.dwconv_fwd(d, t["x"], t["w"], t["bias"]), _bias_ref(r["y"], host["bias"]))
    _check(f"{name} data gradient", H.dwconv_bwd_data(d, t["dy"], t["w"], tuple(case["x"])), r["dx"])
    dw, db = torch.zeros(X.weight_shape(case), device=DEV), torch.zeros(X.cout(case), device=DEV)
    H.dwconv_bwd_weight_acc(d, t["x"], t["dy"], dw, db)
    _check(f"{name} weight gradient", dw, r["dw"])
    _check(f"{name} bias gradient", db, r["db"])
