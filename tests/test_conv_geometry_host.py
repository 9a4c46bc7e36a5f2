"""Geometry of the 1-D / 2-D hypercomplex convolution, host side (no GPU): the reference fixture against the oracle in
both of its modes, what the case table must contain (so that a later edit cannot thin it), the output shapes the library
answers against torch's, and the requests that must raise rather than launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import seld_oracle as O
from tests.golden.conv_geometry_cases import (FIXTURE_CASES, GPU_CASES, fixture_cotangent, fixture_inputs, geometry,
                                              out_extent, remainder, touched, untouched_mask)
from tests.helpers import pkg

SPECIALISED_TAPS = {(1,), (3,), (1, 1), (1, 3), (3, 3)}


@pytest.mark.parametrize("mode", ["assembled", "explicit"])
@pytest.mark.parametrize("case", FIXTURE_CASES, ids=[c["name"] for c in FIXTURE_CASES])
def test_fixture_matches_oracle(golden, case, mode):
    g = golden("conv_geometry")
    name = case["name"]
    x, ws, bias = fixture_inputs(case, torch.float64)
    for t in [x] + ws + ([bias] if bias is not None else []):
        t.requires_grad_(True)
    y = O.hypercomplex_conv(x, ws, bias, case["stride"], case["padding"], 1, case["dilation"], mode=mode)
    assert tuple(y.shape[2:]) == out_extent(case)
    (y * fixture_cotangent(y.shape, torch.float64)).sum().backward()
    pairs = [("y", y.detach()), ("dx", x.grad)] + [(f"dw{i}", w.grad) for i, w in enumerate(ws)]
    if bias is not None:
        pairs.append(("dbias", bias.grad))
    else:
        assert name + ".dbias" not in g
    assert f"{name}.dw{len(ws)}" not in g
    for key, got in pairs:
        ref = g[f"{name}.{key}"]
        assert ref.shape == tuple(got.shape), key
        err = np.abs(got.numpy() - ref).max()
        assert err <= 2e-6 * max(np.abs(ref).max(), 1.0), (key, err)
    # the reference itself leaves the samples no output reads without a gradient
    dead = untouched_mask(case)
    assert float(np.abs(g[name + ".dx"][..., dead.numpy()]).max(initial=0.0)) == 0.0


def test_fixture_holds_only_the_table(golden):
    import json
    g = dict(golden("conv_geometry"))
    meta = json.loads(str(g.pop("meta")))
    assert "reference" in meta
    names = {k.split(".")[0] for k in g}
    assert names == {c["name"] for c in FIXTURE_CASES}
    assert all(v.dtype == np.float32 for v in g.values())


# ---- what the table must contain ---------------------------------------------------------------------------------------
def _ck(c):
    k = 1
    for e in c["k"]:
        k *= e
    return (c["x"][1] // c["algebra"]) * k


def _extent(g, a):
    return g["d"][a] * (g["k"][a] - 1) + 1


def _is_same(c):
    return out_extent(c) == geometry(c)["inp"]


def test_case_table_covers_the_issue():
    names = [c["name"] for c in GPU_CASES]
    assert len(set(names)) == len(names)
    assert all(c in GPU_CASES for c in FIXTURE_CASES)
    G = {c["name"]: geometry(c) for c in GPU_CASES}
    geo = lambda c: G[c["name"]]
    dq = [c for c in GPU_CASES if c["algebra"] == 8]
    dq1 = [c for c in dq if geo(c)["nd"] == 1]
    dq2 = [c for c in dq if geo(c)["nd"] == 2]
    by_algebra = {A: [c for c in GPU_CASES if c["algebra"] == A] for A in (1, 4, 8)}

    # ---- stride
    for s in (2, 3):
        assert any(geo(c)["s"] == (s,) and geo(c)["p"][0] > 0 for c in dq1), f"1-D stride {s} with padding"
    assert {(2, 2), (2, 1), (1, 2), (3, 2)} <= {geo(c)["s"] for c in dq2}
    assert any(geo(c)["k"] == (1,) and geo(c)["s"] == (2,) for c in dq1), "k = 1, s = 2"
    assert any(geo(c)["k"] == (2,) and geo(c)["s"] == (3,) and geo(c)["d"] == (1,) for c in dq1), "k = 2, s = 3"
    assert any(any(s > 1 and d > 1 for s, d in zip(geo(c)["s"], geo(c)["d"])) for c in dq), "stride with dilation"
    for group, what in ((dq1, "1-D"), (dq2, "2-D")):
        # a remainder, and one that reaches past the padding: the last input sample of that axis is read by no output
        assert any(any(r != 0 and not t[-1] for r, t in zip(remainder(c), touched(c))) for c in group), what + " remainder"
    assert any(max(geo(c)["s"]) > 1 and _ck(c) % 4 == 0 and _ck(c) >= 16 and geo(c)["k"] in SPECIALISED_TAPS
               for c in dq), "strided FAST forward"
    assert any(geo(c)["k"] == (3, 3) and geo(c)["s"] == (2, 1) and out_extent(c)[1] % 32 == 0 for c in dq2), \
        "row-chunk weight gradient with sh = 2"

    # ---- tap shapes
    assert {(2,), (4,), (5,), (7,)} <= {geo(c)["k"] for c in dq1}
    assert {(3, 1), (1, 5), (5, 5), (2, 3), (1, 2)} <= {geo(c)["k"] for c in dq2}

    # ---- padding
    pad_items = {
        "valid k = 3 on 32-aligned rows": lambda c, g: g["k"][-1] == 3 and set(g["p"]) == {0} and set(g["s"]) == {1}
        and out_extent(c)[-1] % 32 == 0,
        "output larger than the input": lambda c, g: any(2 * p > d * (k - 1) and s == 1 and o > i for p, d, k, s, o, i in
                                                         zip(g["p"], g["d"], g["k"], g["s"], out_extent(c), g["inp"])),
        "(p, 0)": lambda c, g: g["nd"] == 2 and g["p"][0] > 0 and g["p"][1] == 0,
        "(0, p)": lambda c, g: g["nd"] == 2 and g["p"][0] == 0 and g["p"][1] > 0,
        "padding >= kernel extent": lambda c, g: any(g["p"][a] >= _extent(g, a) for a in range(g["nd"])),
    }
    for what, pred in pad_items.items():
        assert any(pred(c, geo(c)) for c in dq), what
    assert any(geo(c)["nd"] == 2 and len({p for p in geo(c)["p"] if p > 0}) == 2 for c in dq), "two different paddings"

    # ---- the stride, tap and padding items for the quaternion and the real algebra
    for A in (4, 1):
        cs = by_algebra[A]
        assert any(max(geo(c)["s"]) > 1 and max(geo(c)["p"]) > 0 for c in cs), (A, "stride")
        assert any(geo(c)["nd"] == 2 and len(set(geo(c)["s"])) == 2 for c in cs), (A, "per-axis stride")
        assert any(geo(c)["k"] not in SPECIALISED_TAPS for c in cs), (A, "taps")
        assert any(any(pred(c, geo(c)) for pred in pad_items.values()) for c in cs), (A, "padding")
        assert any(geo(c)["nd"] == 1 for c in cs) and any(geo(c)["nd"] == 2 for c in cs), (A, "ranks")

    # ---- dilation
    assert any(geo(c)["k"] == (3, 3) and geo(c)["d"] == (2, 1) and geo(c)["s"] == (1, 1) and _is_same(c)
               and geo(c)["inp"][1] % 64 == 0 and (c["x"][1] // 8) % 16 == 0 and (c["cout"] // 8) % 16 == 0
               for c in dq2), "dil_h = 2 on an otherwise hcq-eligible 3x3"
    assert any(geo(c)["d"] == (2, 3) and geo(c)["k"] == (3, 3) for c in dq2)
    assert any(geo(c)["k"] == (5,) and geo(c)["d"][0] > 1 for c in dq1)

    # ---- gate edges: the benchmark's layers with one property moved
    edges = [c for c in GPU_CASES if c["edge"]]
    for c in edges:
        g = geo(c)
        assert c["algebra"] == 8 and set(g["s"]) == {1} and _is_same(c), c["name"]
        assert g["k"] in {(3,), (1, 3), (3, 3)} and set(g["d"]) == {1}, c["name"]
        assert c["x"][1] in (192, 384) or c["cout"] in (192, 384), c["name"]
    ow = lambda c: out_extent(c)[-1]
    edge_items = {
        "W = 520 or 72": lambda c: geo(c)["inp"][-1] in (520, 72),
        "odd outW": lambda c: ow(c) % 2 == 1,
        "outW < 32": lambda c: ow(c) < 32,
        "outW % 4 == 0, % 32 != 0": lambda c: ow(c) % 4 == 0 and ow(c) % 32 != 0 and ow(c) >= 32,
        "short K": lambda c: _ck(c) < 16 and _ck(c) % 4 != 0,
        "block channels that fill no tile": lambda c: (c["cout"] // 8) % 8 != 0,
        "N = 1": lambda c: c["x"][0] == 1,
        "2-D with H = 1": lambda c: geo(c)["nd"] == 2 and geo(c)["inp"][0] == 1,
        "3x3": lambda c: geo(c)["k"] == (3, 3),
    }
    for what, pred in edge_items.items():
        assert any(pred(c) for c in edges), what

    # ---- the fixture carries every algebra and both ranks on its own
    assert {(c["algebra"], geometry(c)["nd"]) for c in FIXTURE_CASES} == {(A, nd) for A in (1, 4, 8) for nd in (1, 2)}
    assert any(not c["bias"] for c in FIXTURE_CASES) and any(c["bias"] for c in FIXTURE_CASES)


# ---- the library's answers that need no device ---------------------------------------------------------------------------
def _desc(H, c, **over):
    kw = dict(c, **over)
    return H.make_conv_desc(tuple(kw["x"]), kw["cout"], kw["algebra"], kw["k"], kw["stride"], kw["padding"], kw["dilation"])


@pytest.mark.parametrize("case", GPU_CASES, ids=[c["name"] for c in GPU_CASES])
def test_output_shape_equals_torch(case):
    H = pkg().hip_ops
    g = geometry(case)
    x = torch.empty(case["x"], device="meta")
    w = torch.empty((case["cout"], case["x"][1]) + tuple(case["k"]), device="meta")
    fn = F.conv1d if g["nd"] == 1 else F.conv2d
    want = tuple(fn(x, w, None, case["stride"], case["padding"], case["dilation"], 1).shape[2:])
    got = H.conv_out_shape(_desc(H, case))
    assert (got[1],) == want if g["nd"] == 1 else tuple(got) == want
    assert want == out_extent(case)
    if g["nd"] == 1:
        assert got[0] == 1


# the dilated kernel is longer than the padded input: (x shape, k, stride, padding, dilation)
TOO_LONG = [
    ((1, 8, 8), (5,), 1, 0, 3),                  # extent 13 on 8 samples
    ((1, 8, 4), (3,), 2, 0, 2),                  # extent 5 on 4 samples, stride 2: in + 2p - d(k-1) - 1 = -1
    ((1, 8, 8), (5,), 2, 2, 3),                  # extent 13 on 8 + 4, stride 2
    ((1, 8, 10), (4,), 7, 1, 5),                 # extent 16 on 12, stride 7
    ((1, 8, 3, 9), (3, 3), (4, 1), 0, (2, 1)),   # H: extent 5 on 3 rows, stride 4
    ((1, 8, 9, 2), (1, 3), (1, 3), 0, 1),        # W: extent 3 on 2 columns, stride 3
]


@pytest.mark.parametrize("shape,k,s,p,d", TOO_LONG)
def test_kernel_longer_than_the_padded_input_raises(shape, k, s, p, d):
    P = pkg()
    H, L = P.hip_ops, P._lib
    fn = F.conv1d if len(shape) == 3 else F.conv2d
    with pytest.raises(RuntimeError):                       # torch refuses the same request
        fn(torch.zeros(shape), torch.zeros((8, 8) + k), None, s, p, d, 1)
    for A in (1, 4, 8):
        desc = H.make_conv_desc(shape, 8, A, k, s, p, d)
        out = (ctypes.c_int32 * 2)()
        assert L.lib().seld_hc_conv_out_shape(ctypes.byref(desc), out) == -1        # SELD_EINVAL
        with pytest.raises(L.SeldHipError):
            H.conv_out_shape(desc)
        # every entry point answers the same without touching its (absent) operands
        assert L.lib().seld_hc_conv_pair_supported(ctypes.byref(desc), 0) == 0
        if A > 1:
            assert H.hcq_pack_floats(desc, 0) == 0 and H.hcq_pack_floats(desc, 1) == 0


def test_groups_raise():
    P = pkg()
    H, L = P.hip_ops, P._lib
    Q, DQ = P.quaternion, P.dual_quaternion
    desc = H.make_conv_desc((1, 8, 16), 8, 4, (3,), 1, 1, 1, groups=2)
    with pytest.raises(L.SeldHipError):
        H.conv_out_shape(desc)
    m = Q.quaternion_layers.QuaternionConv(8, 8, 3, 1, padding=1, groups=2, seed=1, operation="convolution1d")
    with pytest.raises(L.SeldHipError, match="groups"):
        m(torch.zeros(1, 8, 16))
    m = DQ.dual_quaternion_layers.DualQuaternionConv(16, 16, 3, 1, padding=1, groups=2, seed=1)
    with pytest.raises(L.SeldHipError, match="groups"):
        m(torch.zeros(1, 16, 4, 4))
