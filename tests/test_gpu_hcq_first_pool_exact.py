"""The pooling first-layer convolution (csrc/hcq_first.hip: hcq_first_pool_kernel behind seld_hcq_first_pool and
seld_hcq_first_pool_bn) on the MI355X against the float64 oracle, EXACTLY.  Inputs as in tests/hcq_exact.py: x and bias
integers in [-2, 2], weights in {-1, 0, 1}, so every float32 operation of the convolution is exact in any order and y,
the window value and its row must hold the oracle's numbers bit for bit.  The BatchNorm inputs keep that: gamma in
{-2 .. 2}, mean and beta integers in [-2, 2], invstd in {0.5, 1, 2} -- a = gamma * invstd is a multiple of 0.5 of magnitude
<= 4, b = beta - mean * a one of magnitude <= 10, and a * v + b a float32 number whether or not it is contracted into an
fma.  drop_p = 0.5 scales by exactly 2.

Shapes: the smallest that reach each of the eight (IBC, tile program) instantiations -- the label is asserted, a shape
that falls to another kernel fails -- plus one shape per algebra with two row blocks per image and two column tiles
(interior halos).  The three-tile program needs one channel tile of 24 block channels, i.e. at least 512 position tiles.

  1  seld_hcq_first_pool with y and statistics: y, the statistics (exactly: the condition of tests/hcq_exact.py is
     asserted, not branched on), the window value and its row -- the FIRST row at which sign(gamma) * y is largest, row 0
     for gamma == 0; integer inputs make ties frequent -- all inside sentinel-guarded buffers
  2  the same call without y: the same window values and rows
  3  seld_hcq_first_pool_bn, drop_p = 0: out = relu(a raw + b), the rows, and pool_raw written for gamma == 0 only
  4  seld_hcq_first_pool_bn, drop_p = 0.5: out of 3 times the mask of tests/philox_ref.py, with and without a step state"""
import ctypes

import pytest
import torch

from tests import hcq_exact as X
from tests import philox_ref as R
from tests import pool_window_ref as PW
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POOL = 8                                            # rows of a pooling window = rows a workgroup walks
IDX_SENTINEL = 0xEE                                 # no row of a window


def _case(name, algebra, x, cout, label):
    """The case of tests/golden/hcq_exact_cases.py with this name (same x and Cout: its oracle is shared with
    test_gpu_hcq_exact.py), else a local one."""
    c = X.BY_NAME.get(name) or dict(name=name, algebra=algebra, x=tuple(x), cout=cout, k=(3, 3), stride=1, padding=1,
                                    dilation=1, launch={}, thin=1)
    assert c["x"] == tuple(x) and c["cout"] == cout and c["algebra"] == algebra and c["k"] == (3, 3), name
    return dict(c, pool_label=f"hcq_first_pool_kernel<{label}, {POOL}>")


CASES = [
    _case("q_3x3_ib1_ob16_d1_n1_h8_w64", 4, (1, 4, 8, 64), 64, "1, 1, 0, 1"),
    _case("q_3x3_ib2_ob16_d1_n1_h8_w64", 4, (1, 8, 8, 64), 64, "2, 1, 0, 1"),
    _case("q_3x3_ib1_ob32_d1_n1_h8_w64", 4, (1, 4, 8, 64), 128, "1, 2, 0, 1"),
    _case("q_3x3_ib2_ob32_d1_n1_h8_w64", 4, (1, 8, 8, 64), 128, "2, 2, 0, 1"),
    _case("dq_3x3_ib1_ob16_d1_n1_h8_w64", 8, (1, 8, 8, 64), 128, "1, 1, 1, 2"),
    _case("dq_3x3_ib2_ob16_d1_n1_h8_w64", 8, (1, 16, 8, 64), 128, "2, 1, 1, 2"),
    _case("dq_3x3_ib1_ob24_d1_n2_h16_w1024", 8, (2, 8, 16, 1024), 192, "1, 1, 2, 2"),
    _case("dq_3x3_ib2_ob24_d1_n2_h16_w1024", 8, (2, 16, 16, 1024), 192, "2, 1, 2, 2"),
    # two row blocks per image, two column tiles
    _case("q_3x3_ib2_ob16_d1_n2_h16_w128", 4, (2, 8, 16, 128), 64, "2, 1, 0, 1"),
    _case("dq_3x3_ib1_ob16_d1_n2_h16_w128", 8, (2, 8, 16, 128), 128, "1, 1, 1, 2"),
]
IDS = [c["name"] for c in CASES]
DROPOUT = ["q_3x3_ib1_ob16_d1_n1_h8_w64", "dq_3x3_ib2_ob24_d1_n2_h16_w1024"]       # one quaternion, one three-tile
assert len(set(IDS)) == len(IDS) and len({c["pool_label"] for c in CASES[:8]}) == 8 and all(n in IDS for n in DROPOUT)


# ---- host reference (float64, once per case, left unchanged) -----------------------------------------------------------------
def _bn_inputs(case):
    """gamma in {-2 .. 2} with a positive, a negative and a zero channel in every group of 8 (their places move with the
    group); mean, beta integers in [-2, 2]; invstd in {0.5, 1, 2}."""
    return PW.bn_inputs(case["cout"], torch.Generator().manual_seed(X.W._seed(case, None) ^ 0x9001))


_refs = {}


def _ref(case):
    if case["name"] not in _refs:
        X.assert_exactness_bound(case)
        t = X.inputs(case)
        assert t["wS"] is t["wA"], "the dense weight set gathers the statistics"
        y = X.exact_oracle(case)["yA"] if case["name"] in X.BY_NAME else X.conv64(case, t["x"], t["wA"])
        o = X.epilogue_reference(y, t["biasA"])                              # float64 (N, C, H, W)
        assert bool((o == o.round()).all())
        b = _bn_inputs(case)
        raw, idx, ties = PW.window_rows(o, b["gamma"], POOL)
        z = PW.bn_relu(raw, b["gamma"], b["beta"], b["mean"], b["invstd"])
        _refs[case["name"]] = dict(b, o=o, raw=raw, idx=idx.to(torch.uint8), z=z, ties=ties)
    return _refs[case["name"]]


# ---- device side ------------------------------------------------------------------------------------------------------------
def _setup(case):
    """(library, desc, device inputs, packed forms of mode 2) -- with the label the case names, or the test fails."""
    P = pkg()
    H, L = P.hip_ops, P._lib
    lib = L.lib()
    d = X.desc(H, case)
    buf = ctypes.create_string_buffer(96)
    assert lib.seld_hcq_kernel_label(ctypes.byref(d), 2, 1, buf, 96) == 0, case["name"]
    assert buf.value.decode() == case["pool_label"], case["name"]
    t = X.inputs(case)
    dev = {"x": t["x"].to(DEV), "bias": t["biasA"].to(DEV), "w": [w.to(DEV) for w in t["wA"]]}
    n = int(lib.seld_hcq_pack_floats(ctypes.byref(d), 2, 1))
    assert n > 0
    dev["wp"] = torch.empty(n, device=DEV)
    L.check(lib.seld_hcq_pack(ctypes.byref(d), 2, 1, L.ptr_array8(dev["w"]), None, L.ptr(dev["wp"]), L.current_stream()),
            "seld_hcq_pack")
    return P, d, dev


def _pooled_shape(case):
    N, _, H, Wd = case["x"]
    return (N, case["cout"], H // POOL, Wd)


class _Outputs:
    """Float outputs inside sentinel-filled buffers (X.sentinel_output), the rows inside a buffer of IDX_SENTINEL bytes."""

    def __init__(self, case):
        self.band = X.guard_band(case)
        self.held = []
        self.idx_bufs = []

    def floats(self, shape):
        view, buf, band = X.sentinel_output(shape, self.band, DEV)
        self.held.append((buf, band))
        return view

    def rows(self, shape):
        band = (self.band + 127) // 128 * 128
        n = shape[0] * shape[1] * shape[2] * shape[3]
        buf = torch.full((2 * band + n,), IDX_SENTINEL, device=DEV, dtype=torch.uint8)
        self.idx_bufs.append((buf, band))
        return buf[band:band + n].view(shape)

    def assert_intact(self, what):
        torch.cuda.synchronize()
        for i, (buf, band) in enumerate(self.held):
            X.assert_band_intact(f"{what} float output {i}", buf, band)
        for i, (buf, band) in enumerate(self.idx_bufs):
            bad = int((buf[:band] != IDX_SENTINEL).sum()) + int((buf[buf.numel() - band:] != IDX_SENTINEL).sum())
            assert bad == 0, f"{what} rows {i}: {bad} bytes next to the output were written"


def _pool(P, d, dev, gamma, want_stats, y, stats, raw, idx):
    L = P._lib
    L.check(L.lib().seld_hcq_first_pool(ctypes.byref(d), L.ptr(dev["x"]), L.ptr(dev["wp"]), L.ptr(dev["bias"]), L.ptr(gamma),
                                        int(want_stats), L.ptr(y), L.ptr(stats), L.ptr(raw), L.ptr(idx), L.current_stream()),
            "seld_hcq_first_pool")


def _pool_bn(P, d, dev, b, drop_p, seed, offset, state, raw, idx, out):
    L = P._lib
    L.check(L.lib().seld_hcq_first_pool_bn(ctypes.byref(d), L.ptr(dev["x"]), L.ptr(dev["wp"]), L.ptr(dev["bias"]),
                                           L.ptr(b["gamma"]), L.ptr(b["beta"]), L.ptr(b["mean"]), L.ptr(b["invstd"]),
                                           float(drop_p), int(seed), int(offset), L.ptr(state), L.ptr(raw), L.ptr(idx),
                                           L.ptr(out), L.current_stream()), "seld_hcq_first_pool_bn")


def _bn_dev(r):
    return {k: r[k].to(DEV) for k in ("gamma", "beta", "mean", "invstd")}


def _assert_rows(what, got, want):
    g, w = got.cpu(), want
    assert g.shape == w.shape and torch.equal(g, w), X.mismatch_report(what, g, w)


# ---- 1, 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pool_conv_exact(case):
    P, d, dev = _setup(case)
    r = _ref(case)
    name = case["name"]
    assert r["ties"] > 0, "integer inputs: windows with several maximal rows"
    assert X.sums_are_exact(r["o"]), "the statistics of every shape here can be exact"
    gamma = r["gamma"].to(DEV)
    nrep = P.hip_ops.STATS_REPLICAS
    out = _Outputs(case)
    y, raw, idx = out.floats(X.y_shape(case)), out.floats(_pooled_shape(case)), out.rows(_pooled_shape(case))
    stats = torch.zeros(nrep * 2 * case["cout"], device=DEV)
    _pool(P, d, dev, gamma, 1, y, stats, raw, idx)
    X.assert_exact(f"{name} y", y, r["o"])
    assert X.assert_stats(f"{name} statistics", stats, r["o"], nrep), "compared exactly"
    X.assert_exact(f"{name} window value", raw, r["raw"])
    _assert_rows(f"{name} window row", idx, r["idx"])
    # without y: the same bits
    raw2, idx2 = out.floats(_pooled_shape(case)), out.rows(_pooled_shape(case))
    _pool(P, d, dev, gamma, 0, None, None, raw2, idx2)
    torch.cuda.synchronize()
    assert torch.equal(raw2.view(torch.int32), raw.view(torch.int32)), f"{name}: window values without y differ"
    assert torch.equal(idx2, idx), f"{name}: window rows without y differ"
    out.assert_intact(name)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pool_bn_exact(case):
    P, d, dev = _setup(case)
    r = _ref(case)
    name = case["name"]
    outs = _Outputs(case)
    raw, idx, z = outs.floats(_pooled_shape(case)), outs.rows(_pooled_shape(case)), outs.floats(_pooled_shape(case))
    sentinel = float(raw.flatten()[0])
    _pool_bn(P, d, dev, _bn_dev(r), 0.0, 0, 0, None, raw, idx, z)
    X.assert_exact(f"{name} relu(a raw + b)", z, r["z"])
    _assert_rows(f"{name} window row", idx, r["idx"])
    zero = (r["gamma"] == 0).view(1, -1, 1, 1)
    assert bool(zero.any()) and not bool(zero.all())
    X.assert_exact(f"{name} pool_raw (window value where gamma == 0, untouched elsewhere)", raw,
                   torch.where(zero, r["raw"], torch.full_like(r["raw"], sentinel)))
    outs.assert_intact(name)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_state", [False, True], ids=["offset", "offset+state"])
@pytest.mark.parametrize("name", DROPOUT)
def test_pool_bn_dropout_exact(name, with_state):
    case = CASES[IDS.index(name)]
    P, d, dev = _setup(case)
    r = _ref(case)
    seed, offset, base = 0x5E1D2024, 977, 123457
    state = torch.tensor([base, 0], dtype=torch.int64, device=DEV) if with_state else None
    outs = _Outputs(case)
    raw, idx, z = outs.floats(_pooled_shape(case)), outs.rows(_pooled_shape(case)), outs.floats(_pooled_shape(case))
    _pool_bn(P, d, dev, _bn_dev(r), 0.5, seed, offset, state, raw, idx, z)
    assert float(R.scale_of(0.5)) == 2.0
    mask = torch.from_numpy(R.factors(seed, offset + (base if with_state else 0), r["z"].numel(), 0.5)).view(r["z"].shape)
    assert 0.4 < float((mask == 0).double().mean()) < 0.6
    X.assert_exact(f"{name} dropout of relu(a raw + b)", z, r["z"] * mask.double())
    _assert_rows(f"{name} window row", idx, r["idx"])
    outs.assert_intact(name)
