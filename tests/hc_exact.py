"""Exact block-matrix convolutions (no GPU in this module): inputs, float64 oracle and exactness bound of the cases of
tests/golden/hc_exact_cases.py -- the kernels of csrc/hc_conv_fwd.hip, hc_conv_vec.hip, hc_conv_smallk.hip, hc_wgrad.hip,
hc_wgrad_row.hip and hc_conv_transpose.hip.

Why these kernels must give the float64 oracle's numbers bit for bit on these inputs.  x, dy, dyB, bias, addend and the
accumulate target are integers in [-2, 2], the weights are drawn from {-1, 0, 1}.  The kernels multiply the operands as
they are (a Hamilton block enters with its sign, hc_comp of csrc/hc_common.h; nothing is pre-combined) and accumulate on
the fp32 MFMA or in plain fp32, so
  * a forward element sums at most Cin * KH * KW products of magnitude <= 2 (hc_conv_kernel, hc_conv_vec_kernel and
    hc_conv_smallk_kernel reduce over Ktot = Cin * KH * KW; the transposed convolution's phase kernel over the same
    count at most); bias, addend and the accumulate target add at most 6;
  * a data-gradient element sums at most Cout * KH * KW such products, twice that where a pair launch adds the gradients
    of two convolutions;
  * a weight-gradient element sums, over the Hamilton blocks that hold its component and over the positions, products
    x * dy of magnitude <= 4.  The blocks per component are COUNTED from the sign tables (blocks_per_component below
    restates hc_comp and is checked against the oracle's block_table): 1 real, 4 quaternion, 8 dual quaternion (the
    primal components sit in the two diagonal quadrants).  So |dw| <= 4 * blocks * positions, and the bias gradient is
    at most 2 * positions.  An accumulating call starts from slots holding 0.25 * (component + 1) and the position
    splits fold with float atomics: every partial sum is a multiple of 0.25.
assert_exactness_bound() keeps the forward and data-gradient magnitudes below 2^24 and four times the weight-gradient
magnitude below 2^24 (a float32 holds every multiple of 0.25 below 2^22), so every value any kernel can form is a
float32 number and every float32 operation on them is exact IN ANY ORDER: the MFMA chains, the K chunks, the two sources
of a pair, the position splits and their atomics.  A dropped, doubled or misplaced tap cannot hide below a tolerance.

The BatchNorm statistics of the forward epilogue are plain sums per channel through shuffles, LDS and float atomics.
They are exact under the CONDITION of tests/hcq_exact.py -- the oracle's per-channel sum |o| and sum o^2 stay below 2^24
-- and every case that gathers statistics (`stats`) must meet it: statistics_condition() is asserted, there is no
fallback to a tolerance.  A case may list a `thin`: its statistics launches then run on a weight set with one weight in
`thin` non-zero."""
import torch
import torch.nn.functional as F

from oracle import seld_oracle as O
from tests import hcq_exact as Q
from tests import wgrad_exact as W
from tests.golden.hc_exact_cases import BY_NAME

EXACT_LIMIT = 2 ** 24
FILL_STEP = W.FILL_STEP
guarded, mismatch_report = W.guarded, W.mismatch_report
assert_exact, sentinel_output, assert_band_intact = Q.assert_exact, Q.sentinel_output, Q.assert_band_intact
assert_stats, sums_are_exact, channel_sums, epilogue_reference = Q.assert_stats, Q.sums_are_exact, Q.channel_sums, \
    Q.epilogue_reference


def case(name):
    return BY_NAME[name]


def is_tconv(c):
    return c["kind"] == "tconv"


def _two(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(e) for e in v)


def out_extent(c):
    """(H, W) of the case's output: hc_out_shape, or tconv_validate's rule for the transposed convolution."""
    k, s, p, d = _two(c["k"]), _two(c["stride"]), _two(c["padding"]), _two(c["dilation"])
    if is_tconv(c):
        op = _two(c["output_padding"])
        return tuple((c["x"][2 + i] - 1) * s[i] - 2 * p[i] + d[i] * (k[i] - 1) + op[i] + 1 for i in range(2))
    return tuple((c["x"][2 + i] + 2 * p[i] - d[i] * (k[i] - 1) - 1) // s[i] + 1 for i in range(2))


def y_shape(c):
    return (c["x"][0], c["cout"]) + out_extent(c)


def weight_shape(c):
    A, ci, co = c["algebra"], c["x"][1], c["cout"]
    return ((ci // A, co // A) if is_tconv(c) else (co // A, ci // A)) + _two(c["k"])


def taps(c):
    k = _two(c["k"])
    return k[0] * k[1]


def positions(c):
    """Positions a weight-gradient element reduces over: the output positions of a convolution, the INPUT positions of a
    transposed one (its weight gradient is the mirrored convolution's, reduced over that convolution's output)."""
    e = c["x"][2:] if is_tconv(c) else out_extent(c)
    return c["x"][0] * e[0] * e[1]


def desc(H, c):
    """The descriptor of the case (and the int32[2] output padding for a transposed convolution)."""
    if is_tconv(c):
        return H.conv_transpose_desc(tuple(c["x"]), c["cout"], c["algebra"], c["k"], c["stride"], c["padding"],
                                     c["output_padding"], c["dilation"])
    return H.make_conv_desc(tuple(c["x"]), c["cout"], c["algebra"], c["k"], c["stride"], c["padding"], c["dilation"])


def guard_band(c):
    """One full channel row of the larger tensor plus 64 + pad floats."""
    o = out_extent(c)
    return max(c["x"][2] * c["x"][3], o[0] * o[1]) + 64 + max(_two(c["padding"]))


# ---- the bound -------------------------------------------------------------------------------------------------------------
def hc_comp(algebra, pp, qq):
    """hc_comp of csrc/hc_common.h restated: (component, structural zero, negative) of Hamilton block (pp, qq)."""
    if algebra == 1:
        return 0, False, False
    neg = bool((0x284E >> (((pp & 3) << 2) | (qq & 3))) & 1)
    comp = (pp ^ qq) & 3
    zero = False
    if algebra == 8:
        hp, hq = pp >> 2, qq >> 2
        zero = hp == 0 and hq == 1
        if hp == 1 and hq == 0:
            comp += 4
    return comp, zero, neg


def blocks_per_component(algebra):
    """The most Hamilton blocks any one component occupies, counted from hc_comp."""
    count = [0] * algebra
    for pp in range(algebra):
        for qq in range(algebra):
            comp, zero, _ = hc_comp(algebra, pp, qq)
            if not zero:
                count[comp] += 1
    return max(count)


def bounds(c):
    """Largest magnitude of a forward, data-gradient (of a pair) and weight-gradient element, and of a bias gradient."""
    ci, co = c["x"][1], c["cout"]
    fwd = 2 * ci * taps(c) + 6
    dgrad = 2 * 2 * co * taps(c)
    wgrad = 4 * blocks_per_component(c["algebra"]) * positions(c) + 1
    o = out_extent(c)
    dbias = 2 * c["x"][0] * o[0] * o[1] + 1
    return fwd, dgrad, wgrad, dbias


def assert_exactness_bound(c):
    fwd, dgrad, wgrad, dbias = bounds(c)
    assert fwd < EXACT_LIMIT and dgrad < EXACT_LIMIT, (c["name"], fwd, dgrad)
    assert 4 * wgrad < EXACT_LIMIT and 4 * dbias < EXACT_LIMIT, (c["name"], wgrad, dbias)       # counted in quarters


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _weights(c, gen, kind, thin=1):
    def one():
        if kind != "int":
            return torch.randn(weight_shape(c), generator=gen) * 0.2
        w = torch.randint(-1, 2, weight_shape(c), generator=gen).float()
        if thin > 1:
            w = w * (torch.randint(0, thin, weight_shape(c), generator=gen) == 0).float()
        return w
    return [one() for _ in range(c["algebra"])]


_last_inputs = {}


def inputs(c, kind="int"):
    """dict of float32 tensors: x, dy, dyB (cotangents of the two outputs of a pair), wA, wB (component lists), biasA,
    biasB, addA, `target` (what an accumulating launch adds to) and wS, the weights of the launches that gather
    statistics (wA itself unless the case lists a `thin`).  kind 'int': integers in [-2, 2], weights in {-1, 0, 1};
    'randn': the rounding test's draw.  Seeded per case name."""
    memo = (c["name"], kind)
    if _last_inputs.get("key") == memo:
        return dict(_last_inputs["value"])
    if kind == "int":
        assert_exactness_bound(c)
    gen = torch.Generator().manual_seed(W._seed(c, None) ^ (0 if kind == "int" else 0x5A5A))
    draw = (lambda s: torch.randint(-2, 3, s, generator=gen).float()) if kind == "int" else \
        (lambda s: torch.randn(s, generator=gen))
    t = {"x": draw(tuple(c["x"]))}
    for n in ("dy", "dyB", "addA", "target"):
        t[n] = draw(y_shape(c))
    t["biasA"], t["biasB"] = draw((c["cout"],)), draw((c["cout"],))
    t["wA"], t["wB"] = _weights(c, gen, kind), _weights(c, gen, kind)
    thin = c.get("thin", 1)
    t["wS"] = _weights(c, gen, kind, thin) if kind == "int" and thin > 1 else t["wA"]
    _last_inputs["key"], _last_inputs["value"] = memo, t
    return dict(t)


# ---- oracle ----------------------------------------------------------------------------------------------------------------
def conv64(c, x, ws):
    """The case's operation in float64: the oracle's explicit Hamilton form, or its transposed form (the real block
    matrix through conv_transpose, as tests/test_gpu_tconv.py restates it)."""
    ws = [w.double() for w in ws]
    if is_tconv(c):
        return F.conv_transpose2d(x.double(), O.assemble_conv_weight(ws), None, _two(c["stride"]), _two(c["padding"]),
                                  _two(c["output_padding"]), 1, _two(c["dilation"]))
    return O.hypercomplex_conv(x.double(), ws, None, _two(c["stride"]), _two(c["padding"]), 1, _two(c["dilation"]),
                               mode="explicit")


def oracle(c, t):
    """float64, only what the case's launches (`run`, `pair`) need: yA, yB, yS (no bias), dx (dy through wA), dx_pair
    (plus dyB through wB), dwA / dwB (component lists: x against dy / dyB), dbA / dbB (bias gradients)."""
    run, pair = c["run"], c["pair"]
    res = {}
    x = t["x"].double().requires_grad_(1 in run)
    wA = [w.double().requires_grad_(2 in run) for w in t["wA"]]
    yA = conv64(c, x, wA)
    assert tuple(yA.shape) == y_shape(c), (c["name"], tuple(yA.shape), y_shape(c))
    res["yA"] = yA.detach()
    wanted = ([x] if 1 in run else []) + (wA if 2 in run else [])
    if wanted:
        g = list(torch.autograd.grad((yA * t["dy"].double()).sum(), wanted))
        if 1 in run:
            res["dx"] = g.pop(0)
        if 2 in run:
            res["dwA"], res["dbA"] = g, t["dy"].double().sum(dim=(0, 2, 3))
    if pair:
        wB = [w.double().requires_grad_(2 in pair) for w in t["wB"]]
        yB = conv64(c, x, wB)
        res["yB"] = yB.detach()
        wanted = ([x] if 1 in pair else []) + (wB if 2 in pair else [])
        if wanted:
            g = list(torch.autograd.grad((yB * t["dyB"].double()).sum(), wanted))
            if 1 in pair:
                res["dx_pair"] = res["dx"] + g.pop(0)
            if 2 in pair:
                res["dwB"], res["dbB"] = g, t["dyB"].double().sum(dim=(0, 2, 3))
    if c["stats"]:
        res["yS"] = res["yA"] if t["wS"] is t["wA"] else conv64(c, t["x"], t["wS"]).detach()
    return res


_exact_cache = {}


def exact_oracle(c):
    """oracle() of inputs(c), cached per case name and left unchanged by its users.  Integer-valued and inside the case's
    bounds -- asserted."""
    if c["name"] not in _exact_cache:
        res = oracle(c, inputs(c))
        fwd, dgrad, wgrad, dbias = bounds(c)
        lim = {"yA": fwd, "yB": fwd, "yS": fwd, "dx": dgrad, "dx_pair": dgrad, "dwA": wgrad, "dwB": wgrad, "dbA": dbias,
               "dbB": dbias}
        for n, v in res.items():
            for u in (v if isinstance(v, list) else [v]):
                assert bool((u == u.round()).all()), (c["name"], n)
                assert float(u.abs().max()) <= lim[n], (c["name"], n, float(u.abs().max()), lim[n])
        _exact_cache[c["name"]] = res
    return _exact_cache[c["name"]]


def stats_output(c):
    """The output the statistics launches gather over: conv(x, wS) + biasA + addA."""
    t, r = inputs(c), exact_oracle(c)
    return epilogue_reference(r["yS"], t["biasA"], t["addA"])


def statistics_condition(c):
    return sums_are_exact(stats_output(c)) and sums_are_exact(epilogue_reference(exact_oracle(c)["yS"], inputs(c)["biasA"]))


# ---- weight-gradient slots -------------------------------------------------------------------------------------------------
def slots(c, fill, device="cpu"):
    """Gradient slots, component i prefilled with `fill` * (i + 1)."""
    return [torch.full(weight_shape(c), fill * (i + 1), device=device) for i in range(c["algebra"])]


def expected_slots(dw64, fill):
    return [w + fill * (i + 1) for i, w in enumerate(dw64)]


def assert_slots_exact(what, got, dw64, fill=0.0):
    for i, (g, w) in enumerate(zip(got, expected_slots(dw64, fill))):
        assert_exact(f"{what} component {i}", g, w)
