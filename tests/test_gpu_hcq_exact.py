"""The fast-product forward and data-gradient kernels (csrc/hcq_conv.hip: hcq_conv_kernel, csrc/hcq_first.hip:
hcq_first_kernel) on the MI355X against the float64 oracle, EXACTLY: with integer inputs in [-2, 2] and weights in {-1, 0, 1} every float32 operation of
the kernels is exact in any order (tests/hcq_exact.py), so every output must hold the oracle's integers bit for bit.
Cases: tests/golden/hcq_exact_cases.py -- one per launch (mode, npair, kernel label, ring slot kind) that the dispatch
fixture records, plus edge shapes.

  A  hcq_pack + hcq_conv into NaN-prefilled outputs: every launch a case lists, label and slot kind as recorded
  B  the forward epilogues (bias, addend + statistics, accumulate; another epilogue per set of a pair), directly and
     through conv_fwd, where the first-layer kernel must give way to hcq_conv_kernel for an addend or an accumulate;
     the statistics exact where the oracle says they can be
  C  inputs as views into NaN-filled buffers, outputs as views into sentinel-filled ones: exact, and no sentinel touched
  D  hyper_conv, hyper_conv_add and hyper_conv_pair under autograd, in the default environment, with SELD_DETERMINISTIC=1
     and with SELD_CONV_NO_HCQ=1 (integers are exact on the block-matrix kernels too), again after an in-place edit of
     the weights
  E  the case list once more with randn inputs at test_gpu_conv.py's 1e-4 of max|ref| (integers are exact in any
     reduced-precision format too: exactness alone would not notice a loss of precision)"""
import pytest
import torch

from tests import hcq_exact as X
from tests.golden import hcq_exact_cases as C
from tests.helpers import pkg
from tests.test_gpu_conv import REL, _close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDS = [c["name"] for c in C.ALL_CASES]
FWD_CASES = [c for c in C.ALL_CASES if C.FWD in c["launch"]]
PAIR_CASES = [c for c in C.ALL_CASES if C.FWD_PAIR in c["launch"]]


def _P():
    return pkg()


def _to_dev(t):
    return {k: ([w.to(DEV) for w in v] if isinstance(v, list) else v.to(DEV)) for k, v in t.items()}


def _nan(shape):
    return torch.full(shape, float("nan"), device=DEV)


def _check(what, got, ref):
    """_close with the figure on record first, as tests/test_gpu_wgrad_exact.py prints it."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    err, scale = float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)
    print(f"{what}: max err {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e} (bound {REL:.0e})")
    _close(got, ref)


def _plain_launches(P, case, t, new_out=_nan):
    """Every launch the case lists, through hcq_pack and hcq_conv with the plain epilogue: {(mode, npair): outputs}."""
    H = P.hip_ops
    d = X.desc(H, case)
    res = {}
    for (mode, npair), (label, slot) in case["launch"].items():
        assert X.launch_key(P, d, mode, npair) == (label, slot), (case["name"], mode, npair)
        assert H.hcq_label(d, mode, npair) == label
        wp = H.hcq_pack(d, mode, t["wA"], t["wB"] if npair == 2 else None)
        assert wp is not None, (case["name"], mode, npair)
        if mode == 0:
            outs = tuple(new_out(X.y_shape(case)) for _ in range(npair))
            H.hcq_conv(d, 0, t["x"], wp, outs)
        else:
            outs = (new_out(tuple(case["x"])),)
            H.hcq_conv(d, 1, t["dy"], wp, outs, x2=t["dyB"] if npair == 2 else None)
        res[(mode, npair)] = outs
    torch.cuda.synchronize()
    return res


def _expected(r):
    return {C.FWD: (r["yA"],), C.FWD_PAIR: (r["yA"], r["yB"]), C.DGRAD: (r["dx"],), C.DGRAD_PAIR: (r["dx_pair"],)}


WHAT = {C.FWD: "forward", C.FWD_PAIR: "forward pair", C.DGRAD: "data gradient", C.DGRAD_PAIR: "data gradient of a pair"}


def _compare(case, res, r, cmp):
    want = _expected(r)
    for combo, outs in res.items():
        for s, (g, w) in enumerate(zip(outs, want[combo])):
            cmp(f"{case['name']} {WHAT[combo]} ({case['launch'][combo][0]}), output {s}", g, w)


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_plain_launches_exact(case):
    P = _P()
    r = X.exact_oracle(case)
    res = _plain_launches(P, case, _to_dev(X.inputs(case)))
    assert set(res) == set(case["launch"])
    _compare(case, res, r, X.assert_exact)


# ---- B ---------------------------------------------------------------------------------------------------------------------
def _stats(P, case):
    return torch.zeros(P.hip_ops.STATS_REPLICAS * 2 * case["cout"], device=DEV)


def _assert_stats(P, case, what, st, o, must_be_exact):
    exact = X.assert_stats(f"{case['name']} {what}", st, o, P.hip_ops.STATS_REPLICAS)
    print(f"{case['name']} {what}: statistics compared {'exactly' if exact else 'at rtol 1e-4, atol 2e-3'}")
    if must_be_exact:
        assert exact, "the case records statistics that can be exact"


@pytest.mark.parametrize("case", FWD_CASES, ids=[c["name"] for c in FWD_CASES])
def test_forward_epilogues_exact(case):
    P = _P()
    H, L = P.hip_ops, P._lib
    d = X.desc(H, case)
    t, r = _to_dev(X.inputs(case)), X.exact_oracle(case)
    name = case["name"]
    wp, wps = H.hcq_pack(d, 0, t["wA"]), H.hcq_pack(d, 0, t["wS"])   # (wS: thinned where the case says so, else wA again)
    # bias alone (a first-layer shape stays on hcq_first_kernel)
    y = _nan(X.y_shape(case))
    H.hcq_conv(d, 0, t["x"], wp, (y,), (t["biasA"],))
    X.assert_exact(f"{name} bias", y, X.epilogue_reference(r["yA"], t["biasA"].cpu()))
    # bias + statistics (still the first-layer kernel where the shape has one)
    y, st = _nan(X.y_shape(case)), _stats(P, case)
    H.hcq_conv(d, 0, t["x"], wps, (y,), (t["biasA"],), (L.SELD_EPI_STATS,), stats=(st,))
    o = X.epilogue_reference(r["yS"], t["biasA"].cpu())
    X.assert_exact(f"{name} bias + statistics", y, o)
    _assert_stats(P, case, "bias + statistics", st, o, False)
    # bias + addend + statistics
    y, st = _nan(X.y_shape(case)), _stats(P, case)
    H.hcq_conv(d, 0, t["x"], wps, (y,), (t["biasA"],), (L.SELD_EPI_ADD | L.SELD_EPI_STATS,), (t["addA"],), (st,))
    o = X.epilogue_reference(r["yS"], t["biasA"].cpu(), t["addA"].cpu())
    X.assert_exact(f"{name} bias + addend + statistics", y, o)
    _assert_stats(P, case, "bias + addend + statistics", st, o, case["stats_exact"])
    # y += conv(x)
    y = t["target"].clone()
    H.hcq_conv(d, 0, t["x"], wp, (y,), epilogues=(L.SELD_EPI_ACCUMULATE,))
    X.assert_exact(f"{name} accumulate", y, X.epilogue_reference(r["yA"], target=t["target"].cpu()))


@pytest.mark.parametrize("case", PAIR_CASES, ids=[c["name"] for c in PAIR_CASES])
def test_forward_pair_epilogues_exact(case):
    """A different epilogue per weight set: (bias + addend + statistics | accumulate + statistics) on the sets wS and
    wB, then (plain | bias + addend) on wA and wB."""
    P = _P()
    H, L = P.hip_ops, P._lib
    d = X.desc(H, case)
    t, r = _to_dev(X.inputs(case)), X.exact_oracle(case)
    name = case["name"]
    wp, wps = H.hcq_pack(d, 0, t["wA"], t["wB"]), H.hcq_pack(d, 0, t["wS"], t["wB"])
    ya, yb = _nan(X.y_shape(case)), t["target"].clone()
    sa, sb = _stats(P, case), _stats(P, case)
    H.hcq_conv(d, 0, t["x"], wps, (ya, yb), (t["biasA"], None),
               (L.SELD_EPI_ADD | L.SELD_EPI_STATS, L.SELD_EPI_ACCUMULATE | L.SELD_EPI_STATS), (t["addA"], None), (sa, sb))
    oa = X.epilogue_reference(r["yS"], t["biasA"].cpu(), t["addA"].cpu())
    ob = X.epilogue_reference(r["yB"], target=t["target"].cpu())
    X.assert_exact(f"{name} pair, set A: bias + addend + statistics", ya, oa)
    X.assert_exact(f"{name} pair, set B: accumulate + statistics", yb, ob)
    _assert_stats(P, case, "pair, set A", sa, oa, case["stats_exact"])
    _assert_stats(P, case, "pair, set B", sb, ob, False)
    ya, yb = _nan(X.y_shape(case)), _nan(X.y_shape(case))
    H.hcq_conv(d, 0, t["x"], wp, (ya, yb), (None, t["biasB"]), (0, L.SELD_EPI_ADD), (None, t["addB"]))
    X.assert_exact(f"{name} pair, set A: plain", ya, r["yA"])
    X.assert_exact(f"{name} pair, set B: bias + addend", yb, X.epilogue_reference(r["yB"], t["biasB"].cpu(), t["addB"].cpu()))


@pytest.mark.parametrize("case", FWD_CASES, ids=[c["name"] for c in FWD_CASES])
def test_conv_fwd_epilogues_exact(case):
    """The same through conv_fwd and the packed-form cache.  With statistics alone a first-layer shape runs
    hcq_first_kernel; that kernel takes no addend and does not accumulate, so the plan must fall back for those."""
    P = _P()
    H, L = P.hip_ops, P._lib
    d = X.desc(H, case)
    assert H._hcq_ok(d, 0)
    t, r = _to_dev(X.inputs(case)), X.exact_oracle(case)
    name = case["name"]
    st = _stats(P, case)
    y = H.conv_fwd(d, t["x"], t["wS"], t["biasA"], out=_nan(X.y_shape(case)), epilogue=L.SELD_EPI_STATS, stats=st)
    o = X.epilogue_reference(r["yS"], t["biasA"].cpu())
    X.assert_exact(f"{name} conv_fwd bias + statistics", y, o)
    _assert_stats(P, case, "conv_fwd bias + statistics", st, o, False)
    st = _stats(P, case)
    y = H.conv_fwd(d, t["x"], t["wS"], t["biasA"], out=_nan(X.y_shape(case)), epilogue=L.SELD_EPI_ADD | L.SELD_EPI_STATS,
                   addend=t["addA"], stats=st)
    o = X.epilogue_reference(r["yS"], t["biasA"].cpu(), t["addA"].cpu())
    X.assert_exact(f"{name} conv_fwd bias + addend + statistics", y, o)
    _assert_stats(P, case, "conv_fwd bias + addend + statistics", st, o, case["stats_exact"])
    y = H.conv_fwd(d, t["x"], t["wA"], None, out=t["target"].clone(), epilogue=L.SELD_EPI_ACCUMULATE)
    X.assert_exact(f"{name} conv_fwd accumulate", y, X.epilogue_reference(r["yA"], target=t["target"].cpu()))


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.GUARD)
def test_exact_inside_guard_bands(name):
    """The sources are views inside NaN-filled buffers with a band of one channel row plus halo on each side (a wrong
    halo mask reads a NaN -- a neighbour's memory in training -- instead of zero); every output is a view inside a
    sentinel-filled buffer, and no sentinel next to it may change (the padded slots of a mixed-tile workgroup and the
    rows a first-layer workgroup does not own must write nothing)."""
    P = _P()
    H, L = P.hip_ops, P._lib
    case = X.case(name)
    band = X.guard_band(case)
    t, r = _to_dev(X.inputs(case)), X.exact_oracle(case)
    for n in ("x", "dy", "dyB", "addA"):
        view, buf = X.guarded(t[n], band)
        assert bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[-band:]).all())
        t[n] = view
    held = []

    def new_out(shape):
        view, buf, b = X.sentinel_output(shape, band, DEV)
        held.append((buf, b))
        return view
    res = _plain_launches(P, case, t, new_out)
    _compare(case, res, r, X.assert_exact)
    if C.FWD in case["launch"]:                      # the epilogue that reads and writes more than the plain one
        d = X.desc(H, case)
        y, st = new_out(X.y_shape(case)), _stats(P, case)
        H.hcq_conv(d, 0, t["x"], H.hcq_pack(d, 0, t["wS"]), (y,), (t["biasA"],), (L.SELD_EPI_ADD | L.SELD_EPI_STATS,),
                   (t["addA"],), (st,))
        o = X.epilogue_reference(r["yS"], t["biasA"].cpu(), t["addA"].cpu())
        X.assert_exact(f"{name} bias + addend + statistics", y, o)
        _assert_stats(P, case, "bias + addend + statistics inside guard bands", st, o, case["stats_exact"])
    torch.cuda.synchronize()
    assert len(held) >= len(case["launch"])
    for i, (buf, b) in enumerate(held):
        X.assert_band_intact(f"{name} output {i}", buf, b)


# ---- D ---------------------------------------------------------------------------------------------------------------------
ENVS = {"default": {}, "deterministic": {"SELD_DETERMINISTIC": "1"}, "block_matrix": {"SELD_CONV_NO_HCQ": "1"}}


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("name", C.ROUTES)
def test_autograd_routes_exact(name, env, seld_env):
    P = _P()
    H = P.hip_ops
    for k, v in ENVS[env].items():
        seld_env.set(k, v)
    H._drop_kernel_choice_caches()
    case = X.case(name)
    d = X.desc(H, case)
    if env == "default":
        assert all(H._hcq_ok(d, m, n) for m, n in X.COMBOS) and set(case["launch"]) == set(X.COMBOS), "all four launches"
    if env == "block_matrix":
        assert not any(H._hcq_ok(d, m, n) for m, n in X.COMBOS)
    if env == "deterministic":
        assert H.deterministic()
    host = X.inputs(case)
    host["wA"], host["wB"] = [w.clone() for w in host["wA"]], [w.clone() for w in host["wB"]]
    host["wS"] = host["wA"]
    t = _to_dev(host)
    wA, wB = [w.requires_grad_(True) for w in t["wA"]], [w.requires_grad_(True) for w in t["wB"]]
    p, dl = case["padding"], case["dilation"]
    r = X.exact_oracle(case)
    for attempt in ("first weights", "after an in-place edit"):
        what = f"{name} via {env}, {attempt}: "
        xs = t["x"].clone().requires_grad_(True)
        y = H.hyper_conv(xs, wA, t["biasA"], 1, p, dl)
        (y * t["dy"]).sum().backward()
        X.assert_exact(what + "hyper_conv y", y, X.epilogue_reference(r["yA"], host["biasA"]))
        X.assert_exact(what + "hyper_conv x.grad", xs.grad, r["dx"])
        xs = t["x"].clone().requires_grad_(True)
        y = H.hyper_conv_add(xs, wA, None, t["addA"], 1, p, dl)
        (y * t["dy"]).sum().backward()
        X.assert_exact(what + "hyper_conv_add y", y, X.epilogue_reference(r["yA"], addend=host["addA"]))
        X.assert_exact(what + "hyper_conv_add x.grad", xs.grad, r["dx"])
        xs = t["x"].clone().requires_grad_(True)
        ya, yb = H.hyper_conv_pair(xs, wA, None, wB, None, 1, p, dl, t["addA"], None)
        ((ya * t["dy"]).sum() + (yb * t["dyB"]).sum()).backward()
        H.deferred_wgrads.flush()
        H.join_side_stream()
        torch.cuda.synchronize()
        X.assert_exact(what + "hyper_conv_pair y, set A", ya, X.epilogue_reference(r["yA"], addend=host["addA"]))
        X.assert_exact(what + "hyper_conv_pair y, set B", yb, r["yB"])
        X.assert_exact(what + "hyper_conv_pair x.grad", xs.grad, r["dx_pair"])
        # an in-place integer edit torch knows about: the packed-form cache must follow (still weights in {-1, 0, 1})
        with torch.no_grad():
            for w in wA + wB:
                w.copy_(-w.roll(1, 1))
                w.grad = None
        for ws in (host["wA"], host["wB"]):
            for w in ws:
                w.copy_(-w.roll(1, 1))
        r = X.oracle(case, host)
        assert all(bool((v == v.round()).all()) for v in r.values())


# ---- E ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_plain_launches_rounding(case):
    P = _P()
    host = X.inputs(case, "randn")
    r = X.oracle(case, host)
    res = _plain_launches(P, case, _to_dev(host))
    _compare(case, res, r, _check)
