"""Exact forward passes and data gradients of the fast-product convolution (no GPU in this module): inputs, oracle,
exactness bound and statistics condition of the cases of tests/golden/hcq_exact_cases.py.

Why the kernels of csrc/hcq_conv.hip must give the float64 oracle's numbers bit for bit on these inputs.  x, dy, dyB,
bias, addend and the accumulate target are integers in [-2, 2], the weights are drawn from {-1, 0, 1}.  Then
  * a weight form F_m(w) = +-w_a +- w_b (hcq_pack_kernel; the conjugate of the data gradient only flips signs) is an
    integer with |F| <= 2, an input form G_m(x) = +-x_a +- x_b (hcq_xforms) one with |G| <= 4: a product is an integer of
    magnitude <= 8;
  * each of the 8 accumulators of an output element sums  ranges * IB * taps * nsrc  such products (ranges: 2 for the half
    of a dual quaternion that both K ranges feed, IB: block channels of the source, nsrc: 2 for the data gradient of a
    pair), i.e. an integer of magnitude <= 8 * terms(case);
  * hcq_recombine adds four halves and one whole accumulator: every intermediate is a multiple of 0.5 of magnitude
    <= 3 * 8 * terms, and bias, addend and the accumulate target add at most 6.
A float32 holds every multiple of 0.5 below 2^23.  assert_exactness_bound() keeps 24 * terms + 6 below 2^20, so every
value is a float32 number and every float32 operation on them is exact IN ANY ORDER: the MFMA chains, the order of the
chunks, ranges and sources, the association of the recombination.  A dropped, doubled or misplaced term cannot hide below
a tolerance.

The BatchNorm statistics of the epilogue are plain sums -- sum(o) and sum(o * o) per channel, through shuffles, LDS and
float atomics into replicas.  They are exact under a CONDITION, not a tolerance: the oracle's per-channel sum |o| and
sum o^2 stay below 2^24 (every partial sum of integers is then an integer a float32 holds).  stats_condition() computes
it from the oracle; where it holds the statistics must match exactly, where it does not today's rtol=1e-4, atol=2e-3
apply.  In the cases that list a `thin` the launches that gather statistics run on a third weight set wS with one weight
in `thin` non-zero, which keeps the outputs small enough; every other launch keeps the dense sets wA and wB (in a
thinned set most taps are zero, and a dropped tap that is zero shows nowhere)."""
import ctypes
import re

import torch

from oracle import seld_oracle as O
from tests import wgrad_exact as W
from tests.golden.hcq_exact_cases import BY_NAME

COMBOS = ((0, 1), (0, 2), (1, 1), (1, 2))             # (mode, npair): mode 0 forward, 1 data gradient
EXACT_LIMIT = 2 ** 20
STATS_LIMIT = 2 ** 24
STATS_RTOL, STATS_ATOL = 1e-4, 2e-3

positions, weight_shape, y_shape, desc = W.positions, W.weight_shape, W.y_shape, W.desc
guarded, guard_band, mismatch_report = W.guarded, W.guard_band, W.mismatch_report


def case(name):
    return BY_NAME[name]


def terms(c):
    """Products one accumulator can sum, the larger of the two directions: ranges * IB * taps * nsrc."""
    A = c["algebra"]
    taps = 1
    for e in c["k"]:
        taps *= e
    ranges = 2 if A == 8 else 1
    return max(ranges * (c["x"][1] // A) * taps * 1, ranges * (c["cout"] // A) * taps * 2)


def assert_exactness_bound(c):
    assert 3 * 8 * terms(c) + 6 < EXACT_LIMIT, (c["name"], terms(c))
    assert positions(c) % 64 == 0 and c["x"][-1] % 64 == 0, c["name"]


def launch_key(P, d, mode, npair):
    """(label, slot kind) of the launch the built library plans for (desc, mode, npair); None where it takes none."""
    lib = P._lib.lib()
    if lib.seld_hcq_pack_floats(ctypes.byref(d), mode, npair) == 0:
        return None
    buf = ctypes.create_string_buffer(96)
    shape = (ctypes.c_int32 * 6)()
    if lib.seld_hcq_kernel_label(ctypes.byref(d), mode, npair, buf, 96) != 0:
        return None
    if lib.seld_hcq_launch_shape(ctypes.byref(d), mode, npair, shape) != 0:
        return None
    return buf.value.decode(), int(shape[4])


def tile_program(label):
    """'first' for hcq_first_kernel, else (NT1, NT2, NR, MX) of an hcq_conv_kernel label."""
    if label.startswith("hcq_first_kernel<"):
        return "first"
    a = re.fullmatch(r"hcq_conv_kernel<(.*)>", label).group(1).split(", ")
    return int(a[3]), int(a[4]), int(a[5]), a[7] == "true"


TILE_PROGRAMS = {(1, 2, 2, False): "three-tile", (1, 1, 2, True): "mixed", (1, 1, 2, False): "two-tile dual quaternion",
                 (2, 0, 1, False): "two quaternion tiles", (1, 0, 1, False): "one quaternion tile", "first": "hcq_first_kernel"}


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _weights(c, gen, kind, thin=1):
    if kind == "int":

        def one():
            w = torch.randint(-1, 2, weight_shape(c), generator=gen).float()
            if thin > 1:
                w = w * (torch.randint(0, thin, weight_shape(c), generator=gen) == 0).float()
            return w
    else:
        one = lambda: torch.randn(weight_shape(c), generator=gen) * 0.2
    return [one() for _ in range(c["algebra"])]


_last_inputs = {}


def inputs(c, kind="int", seed=None):
    """dict of float32 tensors: x, dy, dyB (cotangents of the two outputs of a pair), wA, wB (component lists), biasA,
    biasB, addA, addB, `target` (what an accumulating launch adds to) and wS, the weights of the launches that gather
    statistics (wA itself unless the case lists a `thin`).  kind 'int': integers in [-2, 2], weights in {-1, 0, 1};
    'randn': the rounding test's draw."""
    memo = (c["name"], c.get("thin", 1), kind, seed)
    if _last_inputs.get("key") == memo:                     # (the oracle and the test that follows ask for the same draw)
        return dict(_last_inputs["value"])
    if kind == "int":
        assert_exactness_bound(c)
    gen = torch.Generator().manual_seed(W._seed(c, seed) ^ (0 if kind == "int" else 0x5A5A))
    draw = (lambda s: torch.randint(-2, 3, s, generator=gen).float()) if kind == "int" else \
        (lambda s: torch.randn(s, generator=gen))
    t = {"x": draw(tuple(c["x"]))}
    for n in ("dy", "dyB", "addA", "addB", "target"):
        t[n] = draw(y_shape(c))
    t["biasA"], t["biasB"] = draw((c["cout"],)), draw((c["cout"],))
    t["wA"], t["wB"] = _weights(c, gen, kind), _weights(c, gen, kind)
    t["wS"] = _weights(c, gen, kind, c.get("thin", 1)) if kind == "int" and c.get("thin", 1) > 1 else t["wA"]
    _last_inputs["key"], _last_inputs["value"] = memo, t
    return dict(t)


# ---- oracle ---------------------------------------------------------------------------------------------------------------
def conv64(c, x, ws):
    return O.hypercomplex_conv(x.double(), [w.double() for w in ws], None, c["stride"], c["padding"], 1, c["dilation"],
                               mode="explicit")


def oracle(c, t):
    """float64: yA, yB, yS (no bias), dx (of dy through wA) and dx_pair (dy through wA plus dyB through wB)."""
    x = t["x"].double().requires_grad_(True)
    yA, yB = conv64(c, x, t["wA"]), conv64(c, x, t["wB"])
    assert tuple(yA.shape) == y_shape(c), (c["name"], tuple(yA.shape))
    dxA, = torch.autograd.grad((yA * t["dy"].double()).sum(), x)
    dxB, = torch.autograd.grad((yB * t["dyB"].double()).sum(), x)
    yS = yA.detach() if t["wS"] is t["wA"] else conv64(c, t["x"], t["wS"])
    return {"yA": yA.detach(), "yB": yB.detach(), "yS": yS, "dx": dxA, "dx_pair": dxA + dxB}


_exact_cache = {}


def exact_oracle(c):
    """oracle() of inputs(c), cached per case name and left unchanged by its users.  Integer-valued and inside the
    exactness bound -- asserted -- and kept as int16, which holds every case's bound (the whole list stays cached for
    the session: a quarter of the float64 tensors' memory)."""
    if c["name"] not in _exact_cache:
        res = oracle(c, inputs(c))
        assert 3 * 8 * terms(c) < 2 ** 15, c["name"]
        for n, v in res.items():
            assert bool((v == v.round()).all()), (c["name"], n)
            assert float(v.abs().max()) <= 3 * 8 * terms(c), (c["name"], n)
            res[n] = v.to(torch.int16)
        _exact_cache[c["name"]] = res
    return _exact_cache[c["name"]]


def epilogue_reference(y, bias=None, addend=None, target=None):
    """What a forward launch with this epilogue must leave (float64 from exact float32 integers)."""
    o = y.double()
    if bias is not None:
        o = o + bias.double().view(1, -1, *([1] * (y.dim() - 2)))
    if addend is not None:
        o = o + addend.double()
    if target is not None:
        o = o + target.double()
    return o


# ---- statistics -----------------------------------------------------------------------------------------------------------
def channel_sums(o):
    red = tuple(i for i in range(o.dim()) if i != 1)
    o = o.double()
    return o.sum(dim=red), (o * o).sum(dim=red)


def sums_are_exact(o):
    """The condition: per-channel sum |o| and sum o^2 below 2^24 (and o integer-valued)."""
    red = tuple(i for i in range(o.dim()) if i != 1)
    o = o.double()
    return bool((o == o.round()).all()) and float(o.abs().sum(dim=red).max()) < STATS_LIMIT and \
        float((o * o).sum(dim=red).max()) < STATS_LIMIT


def stats_output(c):
    """The output the statistics launches of the tests gather over: conv(x, wS) + biasA + addA."""
    t, r = inputs(c), exact_oracle(c)
    return epilogue_reference(r["yS"], t["biasA"], t["addA"])


def stats_condition(c):
    return sums_are_exact(stats_output(c))


def assert_stats(what, replicas, o, nrep):
    """replicas: the device's statistics buffer (nrep rows of [sum | sum of squares]); o: the float64 output they were
    gathered over.  Exact where the condition holds, else rtol / atol of tests/test_gpu_conv.py.  Returns whether the
    exact comparison applied."""
    C = o.shape[1]
    got = replicas.detach().cpu().double().view(nrep, 2 * C).sum(0)
    s1, s2 = channel_sums(o)
    exact = sums_are_exact(o)
    for name, g, w in (("sum", got[:C], s1), ("sum of squares", got[C:], s2)):
        if exact:
            assert torch.equal(g, w), mismatch_report(f"{what} {name} (exact)", g, w)
        else:
            assert torch.allclose(g, w, rtol=STATS_RTOL, atol=STATS_ATOL), f"{what} {name}: {float((g - w).abs().max())}"
    return exact


# ---- comparison -----------------------------------------------------------------------------------------------------------
def assert_exact(what, got, want):
    g, w = got.detach().cpu(), want.detach().cpu()
    assert g.shape == w.shape, (what, tuple(g.shape), tuple(w.shape))
    assert torch.equal(g.double(), w.double()), mismatch_report(what, g, w)


def sentinel_output(shape, band, device, sentinel=-7777.25):
    """An output view in the middle of a buffer filled with `sentinel` (no result is a quarter): (view, buffer, band)."""
    band = (band + 127) // 128 * 128
    n = 1
    for e in shape:
        n *= e
    buf = torch.full((2 * band + n,), sentinel, device=device, dtype=torch.float32)
    return buf[band:band + n].view(shape), buf, band


def assert_band_intact(what, buf, band, sentinel=-7777.25):
    head, tail = buf[:band], buf[buf.numel() - band:]
    bad = int((head != sentinel).sum()) + int((tail != sentinel).sum())
    assert bad == 0, f"{what}: {bad} floats next to the output were written " \
                     f"(before: {(head != sentinel).nonzero().flatten()[:4].tolist()}, " \
                     f"after: {(tail != sentinel).nonzero().flatten()[:4].tolist()})"
