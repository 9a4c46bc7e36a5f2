"""The block-matrix convolution kernels (csrc/hc_conv_fwd.hip, hc_conv_vec.hip, hc_conv_smallk.hip, hc_wgrad.hip,
hc_wgrad_row.hip, hc_conv_transpose.hip) on the MI355X against the float64 oracle, EXACTLY: with integer inputs in [-2, 2]
and weights in {-1, 0, 1} every float32 operation of the kernels is exact in any order (tests/hc_exact.py), so every
result must hold the oracle's integers bit for bit.  Cases: tests/golden/hc_exact_cases.py -- one per (query, label) pair
the dispatch fixture records, plus edge shapes per kernel family.  Every test runs under its case's environment and first
asserts the labels the library reports, so a case that drifted to another kernel fails instead of passing.

  A  plain launches of the low-level entry points, sources as views inside NaN-filled buffers, outputs as NaN-prefilled
     views inside sentinel-filled ones: forward; the data gradient three ways (with the transposed-weight workspace,
     without it, from a workspace filled ahead), zero where no output reads the input; the weight gradient overwriting
     (with and without the bias gradient), accumulating into non-zero slots, and twice with identical bits; the transposed
     convolution's three entry points
  B  the forward epilogues: bias, bias + statistics, bias + addend + statistics, accumulate -- the statistics exact, no
     tolerance
  C  the pair launches against the oracle and against two single launches
  D  hyper_conv and hyper_conv_transpose under autograd
  E  the case list once more with randn inputs at test_gpu_conv.py's 1e-4 of max|ref| (integers are exact in any
     reduced-precision format too: exactness alone would not notice a loss of precision); prints the worst ratio
  F  the fused BatchNorm/ReLU/MaxPool form of the row kernel (seld_hc_conv_bwd_weight_bnpool_drop_acc) against the plain
     launch fed the gradient it forms, and both against the oracle"""
import ctypes

import pytest
import torch

from tests import hc_exact as X
from tests.golden import hc_exact_cases as C
from tests.golden.conv_geometry_cases import untouched_mask
from tests.helpers import pkg
from tests.test_gpu_conv import REL
from tests.test_hc_exact_host import library_labels, set_case_env

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDS = [c["name"] for c in C.ALL_CASES]
CONV = [c for c in C.ALL_CASES if not X.is_tconv(c)]
FWD_CASES = [c for c in CONV if 0 in c["run"]]
PAIR_CASES = [c for c in CONV if c["pair"]]
FULL_CASES = [c for c in C.ALL_CASES if c["run"] == (0, 1, 2)]
GARBAGE = 123.5


def _ids(cases):
    return [c["name"] for c in cases]


def _to_dev(t):
    return {k: ([w.to(DEV) for w in v] if isinstance(v, list) else v.to(DEV)) for k, v in t.items()}


def _enter(case, seld_env):
    """The case's environment, and the labels the library reports under it."""
    P = pkg()
    set_case_env(case, seld_env)
    assert library_labels(P, case) == case["labels"], case["name"]
    return P, P.hip_ops, P._lib


class Outputs:
    """Outputs as views in the middle of sentinel-filled buffers (NaN-prefilled unless `fill` says otherwise)."""

    def __init__(self, case):
        self.band, self.held = X.guard_band(case), []

    def new(self, shape, fill=float("nan")):
        view, buf, b = X.sentinel_output(tuple(shape), self.band, DEV)
        view.fill_(fill)
        self.held.append((buf, b))
        return view

    def slots(self, case, fill):
        return [self.new(X.weight_shape(case), fill * (i + 1) if fill == X.FILL_STEP else fill) for i in range(case["algebra"])]

    def check(self, what):
        torch.cuda.synchronize()
        for i, (buf, b) in enumerate(self.held):
            X.assert_band_intact(f"{what} output {i}", buf, b)


def _guarded_inputs(case):
    t = _to_dev(X.inputs(case))
    band = X.guard_band(case)
    for n in ("x", "dy", "dyB", "addA"):
        view, buf = X.guarded(t[n], band)
        assert bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[-band:]).all())
        t[n] = view
    return t


def _workspace(L, d):
    nbytes = int(L.lib().seld_hc_conv_bwd_data_workspace(ctypes.byref(d)))
    return torch.empty((nbytes + 3) // 4, device=DEV), nbytes


def _dgrad_three_ways(L, d, dy, ws, new):
    """dx by seld_hc_conv_bwd_data_ex with the transposed-weight workspace (the labelled launch), by
    seld_hc_conv_bwd_data without one, and by seld_hc_conv_transpose_weights + seld_hc_conv_bwd_data_wt."""
    lib, st = L.lib(), L.current_stream()
    wsb, nbytes = _workspace(L, d)
    a, b, c = new(), new(), new()
    L.check(lib.seld_hc_conv_bwd_data_ex(ctypes.byref(d), L.ptr(dy), L.ptr_array8(ws), L.ptr(a), L.ptr(wsb), nbytes, st),
            "seld_hc_conv_bwd_data_ex")
    L.check(lib.seld_hc_conv_bwd_data(ctypes.byref(d), L.ptr(dy), L.ptr_array8(ws), L.ptr(b), st), "seld_hc_conv_bwd_data")
    wt, nbytes = _workspace(L, d)
    L.check(lib.seld_hc_conv_transpose_weights(ctypes.byref(d), L.ptr_array8(ws), L.ptr(wt), nbytes, st),
            "seld_hc_conv_transpose_weights")
    L.check(lib.seld_hc_conv_bwd_data_wt(ctypes.byref(d), L.ptr(dy), L.ptr(wt), L.ptr(c), st), "seld_hc_conv_bwd_data_wt")
    return {"with the workspace": a, "without a workspace": b, "from a workspace filled ahead": c}


def _wgrad_overwrite(L, d, x, dy, dws, dbias):
    L.check(L.lib().seld_hc_conv_bwd_weight(ctypes.byref(d), L.ptr(x), L.ptr(dy), L.ptr_array8(dws), L.ptr(dbias), None, 0,
                                            L.current_stream()), "seld_hc_conv_bwd_weight")


def _wgrad_acc(L, d, x, dy, dws, dbias):
    L.check(L.lib().seld_hc_conv_bwd_weight_acc(ctypes.byref(d), L.ptr(x), L.ptr(dy), L.ptr_array8(dws), L.ptr(dbias),
                                                L.current_stream()), "seld_hc_conv_bwd_weight_acc")


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CONV, ids=_ids(CONV))
def test_plain_launches_exact(case, seld_env):
    P, H, L = _enter(case, seld_env)
    name = case["name"]
    d = X.desc(H, case)
    r, t, out = X.exact_oracle(case), _guarded_inputs(case), Outputs(case)
    if 0 in case["run"]:
        y = out.new(X.y_shape(case))
        L.check(L.lib().seld_hc_conv_fwd_ex(ctypes.byref(d), L.ptr(t["x"]), L.ptr_array8(t["wA"]), None, L.ptr(y), 0, None, None,
                                            L.current_stream()), "seld_hc_conv_fwd_ex")
        X.assert_exact(f"{name} forward ({case['labels'][0]})", y, r["yA"])
        y = H.conv_fwd(d, t["x"], t["wA"], out=out.new(X.y_shape(case)))
        X.assert_exact(f"{name} conv_fwd", y, r["yA"])
    if 1 in case["run"]:
        mask = untouched_mask(case)
        for how, dx in _dgrad_three_ways(L, d, t["dy"], t["wA"], lambda: out.new(case["x"])).items():
            X.assert_exact(f"{name} data gradient {how} ({case['labels'][1]})", dx, r["dx"])
            assert bool((dx[:, :, mask.to(DEV)] == 0.0).all()), f"{name}: input samples no output reads, {how}"
        X.assert_exact(f"{name} conv_bwd_data", H.conv_bwd_data(d, t["dy"], t["wA"], tuple(case["x"])), r["dx"])
    if 2 in case["run"]:
        lab = case["labels"][2]
        # overwriting: the zero-fill comes first, whatever the slots held
        dws, db = out.slots(case, GARBAGE), out.new((case["cout"],), GARBAGE)
        _wgrad_overwrite(L, d, t["x"], t["dy"], dws, db)
        X.assert_slots_exact(f"{name} weight gradient, overwriting ({lab})", dws, r["dwA"])
        X.assert_exact(f"{name} bias gradient, overwriting", db, r["dbA"])
        again = out.slots(case, -GARBAGE)
        _wgrad_overwrite(L, d, t["x"], t["dy"], again, None)
        X.assert_slots_exact(f"{name} weight gradient without the bias gradient", again, r["dwA"])
        assert all(torch.equal(a, b) for a, b in zip(dws, again)), f"{name}: two runs, identical bits"
        # accumulating into non-zero slots
        dws, db = out.slots(case, X.FILL_STEP), out.new((case["cout"],), 0.75)
        _wgrad_acc(L, d, t["x"], t["dy"], dws, db)
        X.assert_slots_exact(f"{name} weight gradient, accumulating", dws, r["dwA"], X.FILL_STEP)
        X.assert_exact(f"{name} bias gradient, accumulating", db, r["dbA"] + 0.75)
        got, _ = H.conv_bwd_weight(d, t["x"], t["dy"], X.weight_shape(case), False)
        X.assert_slots_exact(f"{name} conv_bwd_weight", got, r["dwA"])
    out.check(name)


TCONV = [c for c in C.ALL_CASES if X.is_tconv(c)]


@pytest.mark.parametrize("case", TCONV, ids=_ids(TCONV))
def test_transposed_launches_exact(case, seld_env):
    P, H, L = _enter(case, seld_env)
    name, lib, st = case["name"], L.lib(), L.current_stream()
    d, op = X.desc(H, case)
    r, t, out = X.exact_oracle(case), _guarded_inputs(case), Outputs(case)
    if 0 in case["run"]:
        for bias in (None, t["biasA"]):
            y = out.new(X.y_shape(case))
            L.check(lib.seld_hc_conv_transpose_fwd(ctypes.byref(d), op, L.ptr(t["x"]), L.ptr_array8(t["wA"]), L.ptr(bias),
                                                   L.ptr(y), st), "seld_hc_conv_transpose_fwd")
            X.assert_exact(f"{name} forward ({case['labels'][0]}), bias {bias is not None}", y,
                           X.epilogue_reference(r["yA"], None if bias is None else bias.cpu()))
        X.assert_exact(f"{name} conv_transpose_fwd", H.conv_transpose_fwd(d, op, t["x"], t["wA"], t["biasA"]),
                       X.epilogue_reference(r["yA"], t["biasA"].cpu()))
    if 1 in case["run"]:
        dx = out.new(case["x"])
        L.check(lib.seld_hc_conv_transpose_bwd_data(ctypes.byref(d), op, L.ptr(t["dy"]), L.ptr_array8(t["wA"]), L.ptr(dx), st),
                "seld_hc_conv_transpose_bwd_data")
        X.assert_exact(f"{name} data gradient ({case['labels'][1]})", dx, r["dx"])
    if 2 in case["run"]:
        runs = []
        for _ in range(2):
            dws, db = out.slots(case, X.FILL_STEP), out.new((case["cout"],), 0.75)
            H.conv_transpose_bwd_weight_acc(d, op, t["x"], t["dy"], dws, db)
            X.assert_slots_exact(f"{name} weight gradient ({case['labels'][2]})", dws, r["dwA"], X.FILL_STEP)
            X.assert_exact(f"{name} bias gradient", db, r["dbA"] + 0.75)
            runs.append(dws)
        assert all(torch.equal(a, b) for a, b in zip(*runs)), f"{name}: two runs, identical bits"
        dws = out.slots(case, 0.0)
        H.conv_transpose_bwd_weight_acc(d, op, t["x"], t["dy"], dws, None)
        X.assert_slots_exact(f"{name} weight gradient without the bias gradient", dws, r["dwA"])
    out.check(name)


# ---- B ---------------------------------------------------------------------------------------------------------------------
def _stats(P, case):
    return torch.zeros(P.hip_ops.STATS_REPLICAS * 2 * case["cout"], device=DEV)


def _assert_stats(P, case, what, st, o):
    assert X.assert_stats(f"{case['name']} {what}", st, o, P.hip_ops.STATS_REPLICAS), "no fallback to the tolerance"


@pytest.mark.parametrize("case", FWD_CASES, ids=_ids(FWD_CASES))
def test_forward_epilogues_exact(case, seld_env):
    P, H, L = _enter(case, seld_env)
    name = case["name"]
    d = X.desc(H, case)
    r, t, out = X.exact_oracle(case), _guarded_inputs(case), Outputs(case)
    bias, add, target = t["biasA"].cpu(), t["addA"].cpu(), t["target"].cpu()
    y = H.conv_fwd(d, t["x"], t["wA"], t["biasA"], out=out.new(X.y_shape(case)))
    X.assert_exact(f"{name} bias", y, X.epilogue_reference(r["yA"], bias))
    y = H.conv_fwd(d, t["x"], t["wA"], t["biasA"], out=out.new(X.y_shape(case)), epilogue=L.SELD_EPI_ADD, addend=t["addA"])
    X.assert_exact(f"{name} bias + addend", y, X.epilogue_reference(r["yA"], bias, add))
    y = H.conv_fwd(d, t["x"], t["wA"], None, out=out.new(X.y_shape(case), 0.0).copy_(t["target"]), epilogue=L.SELD_EPI_ACCUMULATE)
    X.assert_exact(f"{name} accumulate", y, X.epilogue_reference(r["yA"], target=target))
    if case["stats"]:
        st = _stats(P, case)
        y = H.conv_fwd(d, t["x"], t["wS"], t["biasA"], out=out.new(X.y_shape(case)), epilogue=L.SELD_EPI_STATS, stats=st)
        o = X.epilogue_reference(r["yS"], bias)
        X.assert_exact(f"{name} bias + statistics", y, o)
        _assert_stats(P, case, "bias + statistics", st, o)
        st = _stats(P, case)
        y = H.conv_fwd(d, t["x"], t["wS"], t["biasA"], out=out.new(X.y_shape(case)),
                       epilogue=L.SELD_EPI_ADD | L.SELD_EPI_STATS, addend=t["addA"], stats=st)
        o = X.epilogue_reference(r["yS"], bias, add)
        X.assert_exact(f"{name} bias + addend + statistics", y, o)
        _assert_stats(P, case, "bias + addend + statistics", st, o)
    out.check(name)


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PAIR_CASES, ids=_ids(PAIR_CASES))
def test_pair_launches_exact(case, seld_env):
    """Each pair form against the oracle AND against the two single launches it stands for."""
    P, H, L = _enter(case, seld_env)
    name, lib, st = case["name"], L.lib(), L.current_stream()
    d = X.desc(H, case)
    r, t, out = X.exact_oracle(case), _guarded_inputs(case), Outputs(case)
    ref = ctypes.byref(d)
    assert tuple(int(lib.seld_hc_conv_pair_supported(ref, w)) for w in (0, 1, 2)) == case["pair_ok"]
    if 0 in case["pair"]:
        ya, yb = out.new(X.y_shape(case)), out.new(X.y_shape(case))
        L.check(lib.seld_hc_conv_pair_fwd(ref, L.ptr(t["x"]), L.ptr_array8(t["wA"]), L.ptr_array8(t["wB"]), None, None,
                                          L.ptr(ya), L.ptr(yb), 0, 0, None, None, None, None, st), "seld_hc_conv_pair_fwd")
        X.assert_exact(f"{name} forward pair, set A", ya, r["yA"])
        X.assert_exact(f"{name} forward pair, set B", yb, r["yB"])
        singles = [H.conv_fwd(d, t["x"], t[w], out=out.new(X.y_shape(case))) for w in ("wA", "wB")]
        assert torch.equal(ya, singles[0]) and torch.equal(yb, singles[1]), f"{name}: forward pair against single launches"
        # a different epilogue per set: bias + addend + statistics | accumulate + statistics
        ya, yb = out.new(X.y_shape(case)), out.new(X.y_shape(case), 0.0).copy_(t["target"])
        sa, sb = _stats(P, case), _stats(P, case)
        want_stats = L.SELD_EPI_STATS if case["stats"] else 0
        L.check(lib.seld_hc_conv_pair_fwd(ref, L.ptr(t["x"]), L.ptr_array8(t["wS"]), L.ptr_array8(t["wB"]), L.ptr(t["biasA"]),
                                          None, L.ptr(ya), L.ptr(yb), L.SELD_EPI_ADD | want_stats,
                                          L.SELD_EPI_ACCUMULATE | want_stats, L.ptr(t["addA"]), None, L.ptr(sa), L.ptr(sb), st),
                "seld_hc_conv_pair_fwd")
        oa = X.epilogue_reference(r["yS"] if case["stats"] else r["yA"], t["biasA"].cpu(), t["addA"].cpu())
        ob = X.epilogue_reference(r["yB"], target=t["target"].cpu())
        X.assert_exact(f"{name} forward pair, set A: bias + addend + statistics", ya, oa)
        X.assert_exact(f"{name} forward pair, set B: accumulate + statistics", yb, ob)
        if case["stats"]:
            _assert_stats(P, case, "forward pair, set A", sa, oa)
            _assert_stats(P, case, "forward pair, set B", sb, ob)
    if 1 in case["pair"]:
        wsb, nbytes = _workspace(L, d)
        wsb = torch.cat([wsb, wsb])
        dx = out.new(case["x"])
        L.check(lib.seld_hc_conv_pair_bwd_data(ref, L.ptr(t["dy"]), L.ptr(t["dyB"]), L.ptr_array8(t["wA"]), L.ptr_array8(t["wB"]),
                                               L.ptr(dx), L.ptr(wsb), 2 * nbytes, st), "seld_hc_conv_pair_bwd_data")
        X.assert_exact(f"{name} data gradient of a pair", dx, r["dx_pair"])
        wts = []
        for w in ("wA", "wB"):
            wt, nbytes = _workspace(L, d)
            L.check(lib.seld_hc_conv_transpose_weights(ref, L.ptr_array8(t[w]), L.ptr(wt), nbytes, st),
                    "seld_hc_conv_transpose_weights")
            wts.append(wt)
        dx2 = out.new(case["x"])
        L.check(lib.seld_hc_conv_pair_bwd_data_wt(ref, L.ptr(t["dy"]), L.ptr(t["dyB"]), L.ptr(wts[0]), L.ptr(wts[1]), L.ptr(dx2),
                                                  st), "seld_hc_conv_pair_bwd_data_wt")
        X.assert_exact(f"{name} data gradient of a pair from workspaces filled ahead", dx2, r["dx_pair"])
        single = H.conv_bwd_data(d, t["dy"], t["wA"], tuple(case["x"])) + H.conv_bwd_data(d, t["dyB"], t["wB"], tuple(case["x"]))
        assert torch.equal(dx, single), f"{name}: data gradient of a pair against the sum of single launches"
        X.assert_exact(f"{name} conv_pair_bwd_data", H.conv_pair_bwd_data(d, t["dy"], t["dyB"], t["wA"], t["wB"], tuple(case["x"])),
                       r["dx_pair"])
    if 2 in case["pair"]:
        assert case["labels"][2].startswith("hc_wgrad_row_kernel<")
        runs = []
        for _ in range(2):
            da, dbs = out.slots(case, X.FILL_STEP), out.slots(case, X.FILL_STEP)
            ba, bb = out.new((case["cout"],), 0.75), out.new((case["cout"],), 0.75)
            L.check(lib.seld_hc_conv_pair_bwd_weight_acc(ref, L.ptr(t["x"]), L.ptr(t["dy"]), L.ptr(t["dyB"]), L.ptr_array8(da),
                                                         L.ptr_array8(dbs), L.ptr(ba), L.ptr(bb), st),
                    "seld_hc_conv_pair_bwd_weight_acc")
            X.assert_slots_exact(f"{name} weight gradient of a pair, set A", da, r["dwA"], X.FILL_STEP)
            X.assert_slots_exact(f"{name} weight gradient of a pair, set B", dbs, r["dwB"], X.FILL_STEP)
            X.assert_exact(f"{name} bias gradient of a pair, set A", ba, r["dbA"] + 0.75)
            X.assert_exact(f"{name} bias gradient of a pair, set B", bb, r["dbB"] + 0.75)
            runs.append(da + dbs)
        assert all(torch.equal(a, b) for a, b in zip(*runs)), f"{name}: two runs, identical bits"
        for dy, pair_slots in ((t["dy"], runs[0][:case["algebra"]]), (t["dyB"], runs[0][case["algebra"]:])):
            single = out.slots(case, X.FILL_STEP)
            _wgrad_acc(L, d, t["x"], dy, single, None)
            assert all(torch.equal(a, b) for a, b in zip(single, pair_slots)), f"{name}: pair against single launches"
    out.check(name)


# ---- D ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FULL_CASES, ids=_ids(FULL_CASES))
def test_autograd_entry_points_exact(case, seld_env):
    """hyper_conv / hyper_conv_transpose under the case's environment: y, x.grad, every component's grad and bias.grad."""
    P, H, L = _enter(case, seld_env)
    name = case["name"]
    r, t = X.exact_oracle(case), _to_dev(X.inputs(case))
    x = t["x"].clone().requires_grad_(True)
    ws = [w.clone().requires_grad_(True) for w in t["wA"]]
    bias = t["biasA"].clone().requires_grad_(True)
    if X.is_tconv(case):
        y = H.hyper_conv_transpose(x, ws, bias, case["stride"], case["padding"], case["output_padding"], case["dilation"])
    else:
        y = H.hyper_conv(x, ws, bias, case["stride"], case["padding"], case["dilation"])
    (y * t["dy"]).sum().backward()
    H.deferred_wgrads.flush()
    H.join_side_stream()
    torch.cuda.synchronize()
    X.assert_exact(f"{name} y", y, X.epilogue_reference(r["yA"], t["biasA"].cpu()))
    X.assert_exact(f"{name} x.grad", x.grad, r["dx"])
    X.assert_slots_exact(f"{name} w.grad", [w.grad for w in ws], r["dwA"])
    X.assert_exact(f"{name} bias.grad", bias.grad, r["dbA"])


# ---- E ---------------------------------------------------------------------------------------------------------------------
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
def test_plain_launches_rounding(case, seld_env):
    P, H, L = _enter(case, seld_env)
    name = case["name"]
    host = X.inputs(case, "randn")
    r, t = X.oracle(case, host), _to_dev(host)
    if X.is_tconv(case):
        d, op = X.desc(H, case)
        if 0 in case["run"]:
            _check(f"{name} forward", H.conv_transpose_fwd(d, op, t["x"], t["wA"]), r["yA"])
        if 1 in case["run"]:
            _check(f"{name} data gradient", H.conv_transpose_bwd_data(d, op, t["dy"], t["wA"], tuple(case["x"])), r["dx"])
        if 2 in case["run"]:
            dws = X.slots(case, 0.0, DEV)
            H.conv_transpose_bwd_weight_acc(d, op, t["x"], t["dy"], dws)
            _check(f"{name} weight gradient", torch.stack(dws), torch.stack(r["dwA"]))
        return
    d = X.desc(H, case)
    if 0 in case["run"]:
        _check(f"{name} forward", H.conv_fwd(d, t["x"], t["wA"]), r["yA"])
    if 1 in case["run"]:
        _check(f"{name} data gradient", H.conv_bwd_data(d, t["dy"], t["wA"], tuple(case["x"])), r["dx"])
    if 2 in case["run"]:
        dws, _ = H.conv_bwd_weight(d, t["x"], t["dy"], X.weight_shape(case), False)
        _check(f"{name} weight gradient", torch.stack(dws), torch.stack(r["dwA"]))
    if 1 in case["pair"]:
        _check(f"{name} data gradient of a pair",
               H.conv_pair_bwd_data(d, t["dy"], t["dyB"], t["wA"], t["wB"], tuple(case["x"])), r["dx_pair"])


# ---- F ---------------------------------------------------------------------------------------------------------------------
FUSED_CASE = C._c("fused_q_3x3_c4_o8_4x32", "conv", 4, (1, 4, 4, 32), 8, (3, 3), (1, 1),
                  labels={2: "hc_wgrad_row_kernel<2, 2, 2, 3, 3, 0>"},
                  why="hc_wgrad_row_kernel<2, 2, 2, 3, 3, 1>: the gradient formed while the operand is staged")
FUSED_POOL = 2


def test_fused_bnpool_weight_gradient_exact(seld_env):
    """hc_wgrad_row_kernel<..., FUSED = 1> forms dy = y*c1 + (pooled > 0 and idx == row ? dpooled*a : 0) + c0 while it
    stages.  With y, dpooled, c1 | a | c0 and x integers in [-2, 2], |dy| <= 2*2 + 2*2 + 2 = 10 and a Hamilton block's sum
    over the 128 positions stays below 10 * 2 * 128 < 2^12, a component's over its 4 blocks plus the slot's fill below 2^24
    in quarters: every operation is exact in any order.  So the fused entry, the plain entry fed the host's float64 dy, and
    the oracle's dw hold the same bits."""
    case, ph = FUSED_CASE, FUSED_POOL
    P, H, L = _enter(case, seld_env)
    name, lib, st = case["name"], L.lib(), L.current_stream()
    d = X.desc(H, case)
    N, Co, Ho, Wo = X.y_shape(case)
    gen = torch.Generator().manual_seed(X.W._seed(case, None))
    draw = lambda s: torch.randint(-2, 3, s, generator=gen).float()
    x, y, dpooled, coef = draw(tuple(case["x"])), draw((N, Co, Ho, Wo)), draw((N, Co, Ho // ph, Wo)), draw((3, Co))
    win = y.view(N, Co, Ho // ph, ph, Wo)
    pooled, idx = win.max(dim=3)                                       # window max and its row
    c1, a, c0 = (coef[i].double().view(1, Co, 1, 1, 1) for i in range(3))
    row = torch.arange(ph).view(1, 1, 1, ph, 1)
    hit = (pooled.unsqueeze(3) > 0) & (idx.unsqueeze(3) == row)
    dy64 = (win.double() * c1 + torch.where(hit, dpooled.double().unsqueeze(3) * a, torch.zeros((), dtype=torch.float64))
            + c0).reshape(N, Co, Ho, Wo)
    assert bool(hit.any()) and not bool(hit.any(dim=3).all()), "both branches of the arg-max term"
    # the bound, as assert_exactness_bound states it
    assert float(dy64.abs().max()) <= 10 and float(x.abs().max()) <= 2
    block = 10 * 2 * X.positions(case)
    assert block < 2 ** 12 and 4 * (X.blocks_per_component(case["algebra"]) * block + 1) < X.EXACT_LIMIT
    r = X.oracle(case, {"x": x, "dy": dy64, "wA": [torch.zeros(X.weight_shape(case)) for _ in range(case["algebra"])]})
    assert all(bool((w == w.round()).all()) for w in r["dwA"])

    out, band = Outputs(case), X.guard_band(case)
    g = {n: X.guarded(v.to(DEV), band)[0] for n, v in (("x", x), ("y", y), ("pooled", pooled), ("dpooled", dpooled),
                                                        ("dy", dy64.float()))}
    idx8, coef_d = idx.to(torch.uint8).to(DEV), coef.to(DEV).contiguous()
    fused, plain = out.slots(case, X.FILL_STEP), out.slots(case, X.FILL_STEP)
    L.check(lib.seld_hc_conv_bwd_weight_bnpool_drop_acc(ctypes.byref(d), L.ptr(g["x"]), L.ptr(g["y"]), L.ptr(g["pooled"]),
                                                        L.ptr(g["dpooled"]), L.ptr(idx8), ph, L.ptr(coef_d),
                                                        L.ptr_array8(fused), 0.0, 0, 0, None, st),
            "seld_hc_conv_bwd_weight_bnpool_drop_acc")
    _wgrad_acc(L, d, g["x"], g["dy"], plain, None)
    torch.cuda.synchronize()
    X.assert_slots_exact(f"{name} fused weight gradient", fused, r["dwA"], X.FILL_STEP)
    X.assert_slots_exact(f"{name} plain weight gradient of the host's dy ({case['labels'][2]})", plain, r["dwA"], X.FILL_STEP)
    assert all(torch.equal(f, p) for f, p in zip(fused, plain)), f"{name}: fused against plain, identical bits"
    out.check(name)
