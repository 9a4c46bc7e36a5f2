"""Exact depthwise convolutions (no GPU in this module): inputs, float64 oracle, exactness bound and the restated launch
plan of the cases of tests/golden/dwconv_exact_cases.py -- the kernels of csrc/dwconv.hip.

Why these kernels must give the float64 oracle's numbers bit for bit on these inputs.  x and dy are integers in [-2, 2],
the weights are drawn from {-1, 0, 1}, the bias is an integer in [-3, 3].  Every kernel is plain fp32 FMAs, wave sums and
a fixed-order fold:
  * a forward element sums KK products of magnitude <= 2 and the bias, a data-gradient element m * KK of them;
  * a weight-gradient element sums x * dy of magnitude <= 4 over the N * Ho * Wo output positions of its channel, a bias
    gradient dy over the same positions.
assert_exactness_bound() keeps m * KK * 2 + 3 below 2^24 and 4 * N * Ho * Wo below 2^22, so that the quarter-valued
prefill of an accumulating call stays representable next to the sums: every value a kernel can form is a float32 number
and every float32 operation on them is exact IN ANY ORDER.  No tolerance fallback.

plan() restates dw_plan of csrc/dwconv.hip -- rows per thread, wave layout, which of the three tile candidates fitted the
LDS budget, staged or not, the phase map of the data gradient, the tile -- in its integer arithmetic.  The kernel label
shows only (nr, div, staged); tests/test_dwconv_exact_host.py ties the rest to the library through the weight-gradient
workspace, Cdst * (KK + 1) * N * tiles * 4 bytes, which fixes TH x TW."""
import torch
import torch.nn.functional as F

from tests import hcq_exact as Q
from tests import wgrad_exact as W
from tests.golden.dwconv_exact_cases import BY_NAME

FWD_LIMIT = 2 ** 24
WGRAD_LIMIT = 2 ** 22
FILL = 0.25
DW_NC = 4
DW_LDS_FLOATS = 8192
FWD, DGRAD, WGRAD = 0, 1, 2
KERNEL = ("dwconv_fwd_kernel", "dwconv_dgrad_kernel", "dwconv_wgrad_kernel")
guarded, mismatch_report = W.guarded, W.mismatch_report
assert_exact, sentinel_output, assert_band_intact = Q.assert_exact, Q.sentinel_output, Q.assert_band_intact


def case(name):
    return BY_NAME[name]


def ndim(c):
    return len(c["x"]) - 2


def two(c, v):
    """The (h, w) pair make_conv_desc stores for a 1-D or 2-D field."""
    if ndim(c) == 1:
        return (1, int(v[0] if isinstance(v, (tuple, list)) else v))
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(e) for e in v)


def geometry(c):
    """in, k, stride, pad, dil as (h, w) pairs, as the descriptor holds them."""
    xin = (1, c["x"][2]) if ndim(c) == 1 else tuple(c["x"][2:])
    pad = two(c, c["padding"])
    if ndim(c) == 1:
        pad = (0, pad[1])
    return xin, two(c, c["k"]), two(c, c["stride"]), pad, two(c, c["dilation"])


def out_extent(c):
    xin, k, s, p, d = geometry(c)
    return tuple((xin[i] + 2 * p[i] - d[i] * (k[i] - 1) - 1) // s[i] + 1 for i in range(2))


def cout(c):
    return c["x"][1] * c["m"]


def y_shape(c):
    o = out_extent(c)
    return (c["x"][0], cout(c)) + (o[1:] if ndim(c) == 1 else o)


def weight_shape(c):
    k = geometry(c)[1]
    return (cout(c), 1) + (k[1:] if ndim(c) == 1 else k)


def taps(c):
    k = geometry(c)[1]
    return k[0] * k[1]


def desc(H, c):
    return H.make_dwconv_desc(tuple(c["x"]), cout(c), c["k"], c["stride"], c["padding"], c["dilation"])


# ---- the plan --------------------------------------------------------------------------------------------------------------
def _extent(ax, T, div):
    """dw_extent: the window along one axis for T results."""
    if div:
        return (T - 1 + (ax["k"] - 1) * ax["d"]) // ax["s"] + 2
    return (T - 1) * ax["a"] + (ax["k"] - 1) * abs(ax["e"]) + 1


def plan(c, which):
    """dw_plan: dict(nr, div, staged, WC, cand, TH, TW, tiles, rows, pitch, src_w, dst).  cand: the index of the tile
    candidate that fitted the LDS budget (0 when none did and the launch reads global memory instead)."""
    xin, k, s, p, d = geometry(c)
    o = out_extent(c)
    dg = which == DGRAD
    ax = []
    for i in range(2):
        a = dict(k=k[i], s=s[i], d=d[i])
        if dg:
            a.update(src=o[i], dst=xin[i], a=1, b=p[i], e=-d[i])
        else:
            a.update(src=xin[i], dst=o[i], a=s[i], b=-p[i], e=d[i])
        ax.append(a)
    div = dg and (s[0] > 1 or s[1] > 1)
    dh, dw = ax[0]["dst"], ax[1]["dst"]
    wc_w = 4 if dw > 512 else 2 if dw > 256 else 1
    wc_1 = wc_w if dh >= 4 else (max(wc_w, 2) if dh >= 2 else 4)
    cand = ((4 if dh >= 8 else 1, wc_w if dh >= 8 else wc_1), (1, wc_1), (1, 1))
    pick, rows, pitch = -1, 0, 0
    for i, (nr, wc) in enumerate(cand):
        r = _extent(ax[0], (4 // wc) * nr, div)
        pt = (_extent(ax[1], 64 * wc * DW_NC, div) + 3 + 3) & ~3
        if r * pt <= DW_LDS_FLOATS:
            pick, rows, pitch = i, r, pt
            break
    staged = pick >= 0
    pick = max(pick, 0)
    nr, WC = cand[pick]
    TH, TW = (4 // WC) * nr, 64 * WC * DW_NC
    tiles = ((dh + TH - 1) // TH) * ((dw + TW - 1) // TW)
    return dict(nr=nr, div=div, staged=staged, WC=WC, cand=pick, TH=TH, TW=TW, tiles=tiles, rows=rows, pitch=pitch,
                src_w=ax[1]["src"], dst=(dh, dw), dm=tuple(a["d"] % a["s"] for a in ax))


def plan_key(c, which):
    """(nr, div, staged, WC, candidate): what distinguishes one launch form from another."""
    q = plan(c, which)
    return q["nr"], q["div"], q["staged"], q["WC"], q["cand"]


def label_of(which, nr, div, staged):
    b = lambda v: "true" if v else "false"
    if which == DGRAD:
        return f"{KERNEL[which]}<{nr}, {b(div)}, {b(staged)}>"
    return f"{KERNEL[which]}<{nr}, {b(staged)}>"


def label(c, which):
    q = plan(c, which)
    return label_of(which, q["nr"], q["div"], q["staged"])


def workspace_bytes(c):
    return cout(c) * (taps(c) + 1) * c["x"][0] * plan(c, WGRAD)["tiles"] * 4


def vec_possible(c, which):
    """The 16-byte staging switch can be on: a staged launch whose source width is a multiple of 4."""
    q = plan(c, which)
    return q["staged"] and q["src_w"] % 4 == 0


def guard_band(c):
    """One full plane of the larger tensor plus 64 + pad floats."""
    xin, _, _, p, _ = geometry(c)
    o = out_extent(c)
    return max(xin[0] * xin[1], o[0] * o[1]) + 64 + max(p)


def read_mask(c):
    """bool (H, W) over the input plane: the samples some output reads through some tap."""
    xin, k, s, p, d = geometry(c)
    o = out_extent(c)
    axes = []
    for i in range(2):
        m = torch.zeros(xin[i], dtype=torch.bool)
        for q in range(o[i]):
            for t in range(k[i]):
                j = q * s[i] - p[i] + t * d[i]
                if 0 <= j < xin[i]:
                    m[j] = True
        axes.append(m)
    return axes[0][:, None] & axes[1][None, :]


# ---- the bound -------------------------------------------------------------------------------------------------------------
def bounds(c):
    o = out_extent(c)
    return c["m"] * taps(c) * 2 + 3, 4 * c["x"][0] * o[0] * o[1] + 1


def assert_exactness_bound(c):
    fwd, wgrad = bounds(c)
    assert fwd < FWD_LIMIT and wgrad < WGRAD_LIMIT, (c["name"], fwd, wgrad)


# ---- inputs and oracle -----------------------------------------------------------------------------------------------------
_last_inputs = {}


def inputs(c, kind="int"):
    """dict of float32 tensors: x, dy, w, bias.  kind 'int': x, dy integers in [-2, 2], weights in {-1, 0, 1}, bias in
    [-3, 3]; 'randn': the rounding pass's draw.  Seeded per case name."""
    memo = (c["name"], kind)
    if _last_inputs.get("key") == memo:
        return dict(_last_inputs["value"])
    gen = torch.Generator().manual_seed(W._seed(c, None) ^ (0 if kind == "int" else 0x5A5A))
    if kind == "int":
        assert_exactness_bound(c)
        t = {"x": torch.randint(-2, 3, tuple(c["x"]), generator=gen).float(),
             "dy": torch.randint(-2, 3, y_shape(c), generator=gen).float(),
             "w": torch.randint(-1, 2, weight_shape(c), generator=gen).float(),
             "bias": torch.randint(-3, 4, (cout(c),), generator=gen).float()}
    else:
        t = {"x": torch.randn(tuple(c["x"]), generator=gen), "dy": torch.randn(y_shape(c), generator=gen),
             "w": torch.randn(weight_shape(c), generator=gen) * 0.3, "bias": torch.randn((cout(c),), generator=gen)}
    _last_inputs["key"], _last_inputs["value"] = memo, t
    return dict(t)


def oracle(c, t):
    """float64 F.conv1d / F.conv2d with groups = C: y (no bias), dx, dw, db."""
    conv = F.conv1d if ndim(c) == 1 else F.conv2d
    x = t["x"].double().requires_grad_(True)
    w = t["w"].double().requires_grad_(True)
    y = conv(x, w, None, c["stride"], c["padding"], c["dilation"], c["x"][1])
    assert tuple(y.shape) == y_shape(c), (c["name"], tuple(y.shape), y_shape(c))
    dx, dw = torch.autograd.grad((y * t["dy"].double()).sum(), [x, w])
    red = (0, 2) if ndim(c) == 1 else (0, 2, 3)
    return {"y": y.detach(), "dx": dx, "dw": dw, "db": t["dy"].double().sum(dim=red)}


_exact_cache = {}


def exact_oracle(c):
    """oracle() of inputs(c), cached per case name and left unchanged by its users.  Integer-valued and inside the case's
    bounds -- asserted."""
    if c["name"] not in _exact_cache:
        res = oracle(c, inputs(c))
        fwd, wgrad = bounds(c)
        lim = {"y": fwd, "dx": fwd, "dw": wgrad, "db": wgrad}
        for n, v in res.items():
            assert bool((v == v.round()).all()), (c["name"], n)
            assert float(v.abs().max()) <= lim[n], (c["name"], n, float(v.abs().max()), lim[n])
        _exact_cache[c["name"]] = res
    return _exact_cache[c["name"]]


# ---- the search grid -------------------------------------------------------------------------------------------------------
def _grid_case(N, C, m, hw, k, s, d):
    kk, ss, dd = ((v, v) if isinstance(v, int) else v for v in (k, s, d))
    pad = tuple(dd[i] * (kk[i] - 1) // 2 for i in range(2))
    return dict(name="grid", x=(N, C) + tuple(hw), m=m, k=kk, stride=ss, padding=pad, dilation=dd)


def grid():
    """Descriptors of the plan search (2-D, every plane below 50 000 elements): extents on either side of the row
    thresholds 2 / 4 / 8 and the width thresholds 256 / 512, windows that fit the 32 KB budget with the first, second or
    third tile candidate or not at all (taps up to 15 x 15 at dilation up to 30), strides that put the data gradient on
    its phase map."""
    for hw in ((1, 8), (1, 40), (1, 264), (1, 528), (2, 40), (2, 264), (2, 528), (5, 8), (5, 264), (5, 528), (9, 40), (9, 264),
               (9, 528), (40, 40), (40, 264), (40, 528), (64, 72)):
        for k in (1, 3, 7, 15):
            for s in (1, 2, (1, 2), (2, 1), 3):
                for d in (1, 2, 30):
                    if k == 1 and d != 1:
                        continue
                    yield _grid_case(1, 2, 1, hw, k, s, d)
