"""Exact 3-D convolutions (no GPU in this module): inputs, float64 oracle, exactness bound and the restated launch plans
of the cases of tests/golden/conv3d_exact_cases.py -- the kernels of csrc/hc_conv3d.hip.

Why these kernels must give the float64 oracle's numbers bit for bit on these inputs.  x and dy are integers in [-2, 2],
the component weights are drawn from {-1, 0, 1}, the bias is an integer in [-3, 3].  c3_gemm multiplies the operands as
they are (a Hamilton block enters with its sign as a +-1 / 0 multiplier at the LDS store, hc_comp of csrc/hc_common.h)
and accumulates on v_mfma_f32_16x16x4_f32, a chain of fp32 FMAs, so
  * a forward or data-gradient element sums at most Cr * KK products of magnitude <= 2 (Cr: the channels of the streamed
    operand, KK the taps) and the bias adds at most 3;
  * a weight-gradient component element sums, over the Hamilton blocks that hold the component and over the positions,
    products x * dy of magnitude <= 4: |dw| <= 4 * blocks * N * So, blocks COUNTED from the oracle's block table (1 real,
    4 quaternion, 8 dual quaternion); the bias gradient is at most 2 * N * (positions of dy).
assert_exactness_bound() keeps the forward and data-gradient magnitudes below 2^24 and the weight-gradient and bias
magnitudes below 2^22, so that the quarter-valued prefill 0.25 * (c + 1) of an accumulating call stays representable next
to them: every value any kernel can form is a float32 number and every float32 operation on them is exact IN ANY ORDER
-- the MFMA chains, the channel blocks, the position splits, the fold.  A dropped, doubled or misplaced tap cannot hide
below a tolerance.  There is no tolerance fallback: a case that breaks the bound is a table error.

The module also restates, in the library's own integer and double arithmetic, what the host side of hc_conv3d.hip
decides and no query reports directly: the phase tables (c3_axis_phase), the tile choice (c3_cfg) and the weight-gradient
plan (c3_plan, c3_bias_plan).  tests/test_conv3d_exact_host.py holds the restatements to the built library: labels to
seld_hc_conv3d_kernel_label, plans to the workspace-byte queries."""
import torch
import torch.nn.functional as F

from oracle import seld_oracle as O
from tests import hc_exact as X2
from tests import hcq_exact as Q
from tests import wgrad_exact as W
from tests.golden.conv3d_exact_cases import BY_NAME

FWD_LIMIT = 2 ** 24
WGRAD_LIMIT = 2 ** 22
FILL_STEP = W.FILL_STEP
C3_MAXS = 16
TILES = ((12, 1), (4, 4), (4, 1), (2, 4), (1, 4))           # cand[] of c3_cfg, in its order
PREF = (1.00, 0.90, 0.60, 0.45, 0.30)
guarded, mismatch_report = W.guarded, W.mismatch_report
assert_exact, sentinel_output, assert_band_intact = Q.assert_exact, Q.sentinel_output, Q.assert_band_intact
epilogue_reference = Q.epilogue_reference
blocks_per_component = X2.blocks_per_component


def case(name):
    return BY_NAME[name]


def is_tconv(c):
    return c["kind"] == "tconv"


def three(v):
    return (int(v),) * 3 if isinstance(v, int) else tuple(int(e) for e in v)


def vol(v):
    return v[0] * v[1] * v[2]


# ---- geometry --------------------------------------------------------------------------------------------------------------
def out_extent(c):
    """(D, H, W) of the case's output: c3_conv_out, or c3_tconv_out for the transposed convolution."""
    k, s, p, d, x = three(c["k"]), three(c["stride"]), three(c["padding"]), three(c["dilation"]), c["x"][2:]
    if is_tconv(c):
        op = three(c["output_padding"])
        return tuple((x[i] - 1) * s[i] - 2 * p[i] + d[i] * (k[i] - 1) + op[i] + 1 for i in range(3))
    return tuple((x[i] + 2 * p[i] - d[i] * (k[i] - 1) - 1) // s[i] + 1 for i in range(3))


def y_shape(c):
    return (c["x"][0], c["cout"]) + out_extent(c)


def weight_shape(c):
    A, ci, co = c["algebra"], c["x"][1], c["cout"]
    return ((ci // A, co // A) if is_tconv(c) else (co // A, ci // A)) + three(c["k"])


def taps(c):
    return vol(three(c["k"]))


def desc(H, c):
    """(descriptor, int32[3] output padding or None)."""
    if is_tconv(c):
        return H.conv3d_transpose_desc(tuple(c["x"]), c["cout"], c["algebra"], c["k"], c["stride"], c["padding"],
                                       c["output_padding"], c["dilation"])
    return H.make_conv3d_desc(tuple(c["x"]), c["cout"], c["algebra"], c["k"], c["stride"], c["padding"], c["dilation"]), None


def g3(c, mirror):
    """g3_of: one launch in convolution terms, x (Ci, in) -> y (Co, out)."""
    cin, cout, xin, out = c["x"][1], c["cout"], tuple(c["x"][2:]), out_extent(c)
    return dict(A=c["algebra"], N=c["x"][0], Ci=cout if mirror else cin, Co=cin if mirror else cout,
                inp=out if mirror else xin, out=xin if mirror else out, k=three(c["k"]), s=three(c["stride"]),
                p=three(c["padding"]), d=three(c["dilation"]))


def gemm(c, which):
    """(g3, phase) of the GEMM launch of entry point `which` (0 forward, 1 data gradient): the convolution's forward and
    the transposed convolution's data gradient run hc_conv3d_fwd_kernel, the other two hc_conv3d_phase_kernel."""
    return g3(c, which == 1), (which == 1) != is_tconv(c)


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def axis_phase(s, pad, dil, K, out):
    """c3_axis_phase: per residue class r of the output index, (k0, n, c0, q) -- first tap, taps, input offset, positions."""
    kstep = s // _gcd(s, dil)
    rows = []
    for r in range(s):
        first = next((k for k in range(min(K, kstep)) if (r + pad - k * dil) % s == 0), -1)
        q = (out - r + s - 1) // s if r < out else 0
        if first < 0:
            rows.append((0, 0, 0, q))
        else:
            assert (r + pad - first * dil) % s == 0
            rows.append((first, (K - 1 - first) // kstep + 1, (r + pad - first * dil) // s, q))
    return rows


def classes(c, which):
    """Per residue class of the launch (class fastest along W, as the grid): (positions per image, taps reaching it,
    (rd, rh, rw)).  One class (the whole output) for hc_conv3d_fwd_kernel."""
    g, phase = gemm(c, which)
    if not phase:
        return [(vol(g["out"]), vol(g["k"]), (0, 0, 0))]
    ax = [axis_phase(g["s"][i], g["p"][i], g["d"][i], g["k"][i], g["out"][i]) for i in range(3)]
    res = []
    for rd in range(g["s"][0]):
        for rh in range(g["s"][1]):
            for rw in range(g["s"][2]):
                a, b, e = ax[0][rd], ax[1][rh], ax[2][rw]
                res.append((a[3] * b[3] * e[3], a[1] * b[1] * e[1], (rd, rh, rw)))
    return res


def gemm_positions(c, which):
    """P of c3_cfg: all positions of the launch's output, over the classes."""
    return c["x"][0] * sum(ps for ps, _, _ in classes(c, which))


def cfg_of(Co, P):
    """c3_cfg in the same double arithmetic: the (ct, pt) with the largest fill * use * pref, the earlier on a tie."""
    best, pick = -1.0, TILES[1]
    for (ct, pt), pref in zip(TILES, PREF):
        bc, bp = ct * 16, pt * 64
        cb = (Co + bc - 1) // bc
        wgs = ((P + bp - 1) // bp) * cb
        fill = 1.0 if wgs >= 512 else float(wgs) / 512.0
        use = float(Co) / float(cb * bc)
        score = fill * use * pref
        if score > best:
            best, pick = score, (ct, pt)
    return pick


def tile(c, which):
    g, _ = gemm(c, which)
    return cfg_of(g["Co"], gemm_positions(c, which))


def label(c, which):
    """What seld_hc_conv3d_kernel_label / seld_hc_conv3d_transpose_kernel_label answer, restated."""
    if which == 2:
        return "hc_conv3d_wgrad_kernel"
    _, phase = gemm(c, which)
    ct, pt = tile(c, which)
    return f"{'hc_conv3d_phase_kernel' if phase else 'hc_conv3d_fwd_kernel'}<{ct}, {pt}>"


def wgrad_plan(c):
    """c3_plan and c3_bias_plan of the case's weight-gradient launch (the mirrored convolution for a transposed one; the
    bias blocks always run over dy = (N, Cout, out))."""
    g = g3(c, is_tconv(c))
    KK = vol(g["k"])
    Kc = g["Ci"] * KK
    Ptot = g["N"] * vol(g["out"])
    ntn, ntm = (Kc + 63) // 64, (g["Co"] + 63) // 64
    ns = min((1024 + ntm * ntn - 1) // (ntm * ntn), (Ptot + 255) // 256, (1 << 26) // (g["Co"] * Kc))
    ns = max(ns, 1)
    split_len = ((Ptot + ns - 1) // ns + 15) // 16 * 16
    nsplit = (Ptot + split_len - 1) // split_len
    C, total = c["cout"], c["x"][0] * vol(out_extent(c))
    nb = max(min((2048 + C - 1) // C, (total + 4095) // 4096), 1)
    blen = (total + nb - 1) // nb
    nbias = (total + blen - 1) // blen
    return dict(Co=g["Co"], Ci=g["Ci"], Kc=Kc, KK=KK, Ptot=Ptot, ntm=ntm, ntn=ntn, nsplit=nsplit, split_len=split_len,
                last_split=Ptot - (nsplit - 1) * split_len, nbias=nbias, blen=blen, Wo=g["out"][2],
                bytes=(nsplit * g["Co"] * Kc + nbias * C) * 4)


def guard_band(c):
    """One full channel row of the larger tensor plus 64 + pad floats."""
    return max(vol(c["x"][2:]), vol(out_extent(c))) + 64 + max(three(c["padding"]))


def read_mask(c):
    """bool (D, H, W) over the INPUT of a convolution: the samples some output reads through some tap."""
    k, s, p, d, x, o = three(c["k"]), three(c["stride"]), three(c["padding"]), three(c["dilation"]), c["x"][2:], out_extent(c)
    axes = []
    for i in range(3):
        m = torch.zeros(x[i], dtype=torch.bool)
        for q in range(o[i]):
            for t in range(k[i]):
                j = q * s[i] - p[i] + t * d[i]
                if 0 <= j < x[i]:
                    m[j] = True
        axes.append(m)
    return axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]


# ---- the bound -------------------------------------------------------------------------------------------------------------
def bounds(c):
    """Largest magnitude of a forward, data-gradient and weight-gradient element, and of a bias gradient."""
    fwd = 2 * c["x"][1] * taps(c) + 3
    dgrad = 2 * c["cout"] * taps(c)
    pl = wgrad_plan(c)
    wgrad = 4 * blocks_per_component(c["algebra"]) * pl["Ptot"] + 2        # + the prefill 0.25 * (c + 1) <= 2
    dbias = 2 * c["x"][0] * vol(out_extent(c)) + 1
    return fwd, dgrad, wgrad, dbias


def assert_exactness_bound(c):
    fwd, dgrad, wgrad, dbias = bounds(c)
    assert fwd < FWD_LIMIT and dgrad < FWD_LIMIT, (c["name"], fwd, dgrad)
    if 2 in c["run"]:
        assert wgrad < WGRAD_LIMIT and dbias < WGRAD_LIMIT, (c["name"], wgrad, dbias)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
_last_inputs = {}


def inputs(c, kind="int"):
    """dict of float32 tensors: x, dy, ws (component list), bias.  kind 'int': x, dy integers in [-2, 2], weights dense in
    {-1, 0, 1}, bias in [-3, 3]; 'randn': the rounding pass's draw.  Seeded per case name."""
    memo = (c["name"], kind)
    if _last_inputs.get("key") == memo:
        return dict(_last_inputs["value"])
    if kind == "int":
        assert_exactness_bound(c)
    gen = torch.Generator().manual_seed(W._seed(c, None) ^ (0 if kind == "int" else 0x5A5A))
    if kind == "int":
        t = {"x": torch.randint(-2, 3, tuple(c["x"]), generator=gen).float(),
             "dy": torch.randint(-2, 3, y_shape(c), generator=gen).float(),
             "ws": [torch.randint(-1, 2, weight_shape(c), generator=gen).float() for _ in range(c["algebra"])],
             "bias": torch.randint(-3, 4, (c["cout"],), generator=gen).float()}
    else:
        t = {"x": torch.randn(tuple(c["x"]), generator=gen), "dy": torch.randn(y_shape(c), generator=gen),
             "ws": [torch.randn(weight_shape(c), generator=gen) * 0.2 for _ in range(c["algebra"])],
             "bias": torch.randn((c["cout"],), generator=gen)}
    _last_inputs["key"], _last_inputs["value"] = memo, t
    return dict(t)


# ---- oracle ----------------------------------------------------------------------------------------------------------------
def conv64(c, x, ws):
    """The case's operation in float64 on the assembled real block matrix (as tests/test_gpu_conv3d.py's
    test_large_shapes_against_float64), no bias."""
    M = O.assemble_conv_weight([w.double() for w in ws])
    s, p, d = three(c["stride"]), three(c["padding"]), three(c["dilation"])
    if is_tconv(c):
        return F.conv_transpose3d(x.double(), M, None, s, p, three(c["output_padding"]), 1, d)
    return F.conv3d(x.double(), M, None, s, p, d)


def oracle(c, t):
    """float64, only what the case's launches (`run`) need: y (no bias), dx, dw (component list), db."""
    run = c["run"]
    res = {}
    x = t["x"].double().requires_grad_(1 in run)
    ws = [w.double().requires_grad_(2 in run) for w in t["ws"]]
    y = conv64(c, x, ws)
    assert tuple(y.shape) == y_shape(c), (c["name"], tuple(y.shape), y_shape(c))
    if 0 in run:
        res["y"] = y.detach()
    wanted = ([x] if 1 in run else []) + (ws if 2 in run else [])
    if wanted:
        g = list(torch.autograd.grad((y * t["dy"].double()).sum(), wanted))
        if 1 in run:
            res["dx"] = g.pop(0)
        if 2 in run:
            res["dw"], res["db"] = g, t["dy"].double().sum(dim=(0, 2, 3, 4))
    return res


_exact_cache = {}


def exact_oracle(c):
    """oracle() of inputs(c), cached per case name and left unchanged by its users.  Integer-valued and inside the case's
    bounds -- asserted."""
    if c["name"] not in _exact_cache:
        res = oracle(c, inputs(c))
        fwd, dgrad, wgrad, dbias = bounds(c)
        lim = {"y": fwd, "dx": dgrad, "dw": wgrad, "db": dbias}
        for n, v in res.items():
            for u in (v if isinstance(v, list) else [v]):
                assert bool((u == u.round()).all()), (c["name"], n)
                assert float(u.abs().max()) <= lim[n], (c["name"], n, float(u.abs().max()), lim[n])
        _exact_cache[c["name"]] = res
    return _exact_cache[c["name"]]


# ---- weight-gradient slots -------------------------------------------------------------------------------------------------
def expected_slots(dw64, fill):
    return [w + fill * (i + 1) for i, w in enumerate(dw64)]


def assert_slots_exact(what, got, dw64, fill=0.0):
    for i, (g, w) in enumerate(zip(got, expected_slots(dw64, fill))):
        assert_exact(f"{what} component {i}", g, w)
