"""The 3-D convolution kernels (csrc/hc_conv3d.hip) on the MI355X against the float64 oracle, EXACTLY: with integer
inputs in [-2, 2], weights in {-1, 0, 1} and integer biases every float32 operation of the kernels is exact in any order
(tests/conv3d_exact.py), so every result must hold the oracle's integers bit for bit.  Cases:
tests/golden/conv3d_exact_cases.py -- one per reachable (entry point, algebra, label), plus edge shapes.  Every test
first asserts the labels the library reports, so a case that drifted to another tile fails instead of passing.

  A  plain launches of the C entry points and of hip_ops.conv3d_fwd / conv3d_bwd_data / conv3d_bwd_weight_acc: sources
     as views inside NaN-filled buffers, outputs as NaN-prefilled views inside sentinel-filled ones; the forward with and
     without bias and into a view 4 bytes off a 16-byte boundary; the data gradient exactly 0.0 where no output reads the
     input; the weight gradient accumulating into quarter-valued slots, twice with identical bits, with and without the
     bias gradient
  B  hyper_conv and hyper_conv_transpose under autograd, and again after an in-place edit of the weights
  C  the case list once more with randn inputs at test_gpu_conv3d.py's 1e-4 of max|ref| (integers are exact in any
     reduced-precision format too: exactness alone would not notice a loss of precision); prints the worst ratio"""
import ctypes

import pytest
import torch

from tests import conv3d_exact as X
from tests.golden import conv3d_exact_cases as C
from tests.helpers import pkg
from tests.test_conv3d_exact_host import library_labels

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDS = [c["name"] for c in C.ALL_CASES]
FULL_CASES = [c for c in C.ALL_CASES if c["run"] == (0, 1, 2)]
REL = 1e-4                                  # tests/test_gpu_conv3d.py: of max|ref|
OFFSET_LIMIT = 1 << 22                      # outputs up to this many floats are also written 4 bytes off alignment


def _to_dev(t):
    return {k: ([w.to(DEV) for w in v] if isinstance(v, list) else v.to(DEV)) for k, v in t.items()}


def _enter(case):
    P = pkg()
    assert library_labels(P, case) == case["labels"], case["name"]
    return P, P.hip_ops, P._lib


class Outputs:
    """Outputs as views in the middle of sentinel-filled buffers (NaN-prefilled unless `fill` says otherwise); `shift`
    floats past the 512-byte aligned start of the view."""

    def __init__(self, case):
        self.band, self.held = X.guard_band(case), []

    def new(self, shape, fill=float("nan"), shift=0):
        n = 1
        for e in shape:
            n *= e
        _, buf, b = X.sentinel_output((n + shift,), self.band, DEV)
        view = buf[b + shift:b + shift + n].view(tuple(shape))
        assert view.data_ptr() % 16 == 4 * shift
        view.fill_(fill)
        self.held.append((buf, b, shift, n))
        return view

    def slots(self, case, fill):
        return [self.new(X.weight_shape(case), fill * (i + 1)) for i in range(case["algebra"])]

    def check(self, what):
        torch.cuda.synchronize()
        for i, (buf, b, shift, n) in enumerate(self.held):
            X.assert_band_intact(f"{what} output {i}", buf, b)
            assert bool((buf[b:b + shift] == -7777.25).all()), f"{what} output {i}: written before a shifted view"


def _guarded_inputs(case):
    t = _to_dev(X.inputs(case))
    band = X.guard_band(case)
    for n in ("x", "dy"):
        view, buf = X.guarded(t[n], band)
        assert bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[-band:]).all())
        t[n] = view
    return t


def _fwd(L, d, op, x, ws, bias, y):
    lib, st = L.lib(), L.current_stream()
    if op is None:
        L.check(lib.seld_hc_conv3d_fwd(ctypes.byref(d), L.ptr(x), L.ptr_array8(ws), L.ptr(bias), L.ptr(y), st),
                "seld_hc_conv3d_fwd")
    else:
        L.check(lib.seld_hc_conv3d_transpose_fwd(ctypes.byref(d), op, L.ptr(x), L.ptr_array8(ws), L.ptr(bias), L.ptr(y), st),
                "seld_hc_conv3d_transpose_fwd")


def _bwd_data(L, d, op, dy, ws, dx):
    lib, st = L.lib(), L.current_stream()
    if op is None:
        L.check(lib.seld_hc_conv3d_bwd_data(ctypes.byref(d), L.ptr(dy), L.ptr_array8(ws), L.ptr(dx), st),
                "seld_hc_conv3d_bwd_data")
    else:
        L.check(lib.seld_hc_conv3d_transpose_bwd_data(ctypes.byref(d), op, L.ptr(dy), L.ptr_array8(ws), L.ptr(dx), st),
                "seld_hc_conv3d_transpose_bwd_data")


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_plain_launches_exact(case):
    P, H, L = _enter(case)
    name = case["name"]
    d, op = X.desc(H, case)
    r, t, out = X.exact_oracle(case), _guarded_inputs(case), Outputs(case)
    bias = t["bias"].cpu()
    if 0 in case["run"]:
        lab = case["labels"][0]
        for b in (None, t["bias"]):
            y = out.new(X.y_shape(case))
            _fwd(L, d, op, t["x"], t["ws"], b, y)
            X.assert_exact(f"{name} forward ({lab}), bias {b is not None}", y,
                           X.epilogue_reference(r["y"], None if b is None else bias))
        if y.numel() <= OFFSET_LIMIT:
            y = out.new(X.y_shape(case), shift=1)
            _fwd(L, d, op, t["x"], t["ws"], t["bias"], y)
            X.assert_exact(f"{name} forward into a view 4 bytes off a 16-byte boundary", y, X.epilogue_reference(r["y"], bias))
        X.assert_exact(f"{name} conv3d_fwd", H.conv3d_fwd(d, op, t["x"], t["ws"], t["bias"]), X.epilogue_reference(r["y"], bias))
    if 1 in case["run"]:
        dx = out.new(case["x"])
        _bwd_data(L, d, op, t["dy"], t["ws"], dx)
        X.assert_exact(f"{name} data gradient ({case['labels'][1]})", dx, r["dx"])
        if not X.is_tconv(case):
            unread = ~X.read_mask(case)
            assert bool((dx[:, :, unread.to(DEV)] == 0.0).all()), f"{name}: input samples no output reads"
        X.assert_exact(f"{name} conv3d_bwd_data", H.conv3d_bwd_data(d, op, t["dy"], t["ws"], tuple(case["x"])), r["dx"])
    if 2 in case["run"]:
        runs = []
        for _ in range(2):
            dws, db = out.slots(case, X.FILL_STEP), out.new((case["cout"],), 0.75)
            H.conv3d_bwd_weight_acc(d, op, t["x"], t["dy"], dws, db)
            X.assert_slots_exact(f"{name} weight gradient, accumulating", dws, r["dw"], X.FILL_STEP)
            X.assert_exact(f"{name} bias gradient, accumulating", db, r["db"] + 0.75)
            runs.append(dws + [db])
        assert all(torch.equal(a, b) for a, b in zip(*runs)), f"{name}: two runs, identical bits"
        dws = out.slots(case, 0.0)
        H.conv3d_bwd_weight_acc(d, op, t["x"], t["dy"], dws, None)
        X.assert_slots_exact(f"{name} weight gradient without the bias gradient", dws, r["dw"])
    out.check(name)


# ---- B ---------------------------------------------------------------------------------------------------------------------
def _autograd(H, case, x, ws, bias, dy):
    if X.is_tconv(case):
        y = H.hyper_conv_transpose(x, ws, bias, case["stride"], case["padding"], case["output_padding"], case["dilation"])
    else:
        y = H.hyper_conv(x, ws, bias, case["stride"], case["padding"], case["dilation"])
    (y * dy).sum().backward()
    H.deferred_wgrads.flush()
    H.join_side_stream()
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("case", FULL_CASES, ids=[c["name"] for c in FULL_CASES])
def test_autograd_entry_points_exact(case):
    """hyper_conv / hyper_conv_transpose: y, x.grad, every component's grad and bias.grad -- and once more after the
    weights changed in place (component 0 negated, the last one rolled along its first axis)."""
    P, H, L = _enter(case)
    name = case["name"]
    host = X.inputs(case)
    r, t = X.exact_oracle(case), _to_dev(host)
    x = t["x"].clone().requires_grad_(True)
    ws = [w.clone().requires_grad_(True) for w in t["ws"]]
    bias = t["bias"].clone().requires_grad_(True)
    y = _autograd(H, case, x, ws, bias, t["dy"])
    X.assert_exact(f"{name} y", y, X.epilogue_reference(r["y"], host["bias"]))
    X.assert_exact(f"{name} x.grad", x.grad, r["dx"])
    X.assert_slots_exact(f"{name} w.grad", [w.grad for w in ws], r["dw"])
    X.assert_exact(f"{name} bias.grad", bias.grad, r["db"])
    edited = dict(host, ws=[w.clone() for w in host["ws"]])
    edited["ws"][0].neg_()
    edited["ws"][-1].copy_(torch.roll(host["ws"][-1], 1, 0) if host["ws"][-1].shape[0] > 1 else -host["ws"][-1].flip(1))
    with torch.no_grad():
        for w, e in zip(ws, edited["ws"]):
            w.copy_(e.to(DEV))
    for leaf in [x, bias] + ws:
        leaf.grad = None
    r2 = X.oracle(case, edited)
    assert not torch.equal(r2["y"], r["y"])
    y = _autograd(H, case, x, ws, bias, t["dy"])
    X.assert_exact(f"{name} y after the edit", y, X.epilogue_reference(r2["y"], host["bias"]))
    X.assert_exact(f"{name} x.grad after the edit", x.grad, r2["dx"])
    X.assert_slots_exact(f"{name} w.grad after the edit", [w.grad for w in ws], r2["dw"])
    X.assert_exact(f"{name} bias.grad after the edit", bias.grad, r2["db"])


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
    r, t = X.oracle(case, host), _to_dev(host)
    d, op = X.desc(H, case)
    if 0 in case["run"]:
        _check(f"{name} forward", H.conv3d_fwd(d, op, t["x"], t["ws"], t["bias"]), X.epilogue_reference(r["y"], host["bias"]))
    if 1 in case["run"]:
        _check(f"{name} data gradient", H.conv3d_bwd_data(d, op, t["dy"], t["ws"], tuple(case["x"])), r["dx"])
    if 2 in case["run"]:
        dws = [torch.zeros(X.weight_shape(case), device=DEV) for _ in range(case["algebra"])]
        db = torch.zeros(case["cout"], device=DEV)
        H.conv3d_bwd_weight_acc(d, op, t["x"], t["dy"], dws, db)
        _check(f"{name} weight gradient", torch.stack(dws), torch.stack(r["dw"]))
        _check(f"{name} bias gradient", db, r["db"])
