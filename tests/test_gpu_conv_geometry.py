"""Geometry of the 1-D / 2-D hypercomplex convolution on the MI355X (csrc/hc_conv_fwd.hip, hc_wgrad.hip, hc_wgrad_row.hip
and the fast families in front of them): stride, tap shapes, padding, dilation and the shapes one step outside a fast
kernel's gate, against the float64 oracle and the reference fixture; elements a kernel must write, add to or leave at
exactly zero; which kernels the table reaches; the neighbouring entry points on the generic kernels; the layers.
Tolerance: test_gpu_conv.py's 1e-4 of max|ref| throughout."""
import ctypes
import re

import pytest
import torch

from oracle import seld_oracle as O
from tests.golden.conv_geometry_cases import (FIXTURE_CASES, GPU_CASES, fixture_cotangent, fixture_inputs, geometry,
                                              random_inputs, untouched_mask, weight_shape)
from tests.helpers import pkg
from tests.test_gpu_conv import REL, _close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDS = [c["name"] for c in GPU_CASES]
BY_NAME = {c["name"]: c for c in GPU_CASES}


def _mods():
    P = pkg()
    return P, P._lib, P.hip_ops


def _desc(H, c):
    return H.make_conv_desc(tuple(c["x"]), c["cout"], c["algebra"], c["k"], c["stride"], c["padding"], c["dilation"])


def _check(what, got, ref):
    """_close, with the figure on record first (pytest shows it for a failing test, -s for every test)."""
    g = got.detach().double().cpu()
    r = (ref.detach() if torch.is_tensor(ref) else torch.as_tensor(ref)).double().cpu()
    if tuple(g.shape) == tuple(r.shape):
        err, scale = float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)
        print(f"{what}: max err {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e} (bound {REL:.0e})")
    _close(got, ref)


_oracle_cache = {}


def _oracle(case):
    """float64 oracle (mode='explicit': one real convolution per Hamilton block) of a case's seeded random inputs:
    (x, ws, bias, cot) in float32 and (y, dx, [dw], dbias) in float64."""
    name = case["name"]
    if name not in _oracle_cache:
        x, ws, bias, cot = random_inputs(case)
        x64 = x.double().requires_grad_(True)
        w64 = [w.double().requires_grad_(True) for w in ws]
        b64 = bias.double().requires_grad_(True) if bias is not None else None
        yr = O.hypercomplex_conv(x64, w64, b64, case["stride"], case["padding"], 1, case["dilation"], mode="explicit")
        assert tuple(yr.shape) == tuple(cot.shape)
        (yr * cot.double()).sum().backward()
        _oracle_cache[name] = ((x, ws, bias, cot),
                               (yr.detach(), x64.grad, [w.grad for w in w64], b64.grad if b64 is not None else None))
    return _oracle_cache[name]


def _run(H, case, x, ws, bias, cot):
    xd = x.to(DEV).requires_grad_(True)
    wd = [w.to(DEV).requires_grad_(True) for w in ws]
    bd = bias.to(DEV).requires_grad_(True) if bias is not None else None
    y = H.hyper_conv(xd, wd, bd, case["stride"], case["padding"], case["dilation"])
    (y * cot.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xd.grad, [w.grad for w in wd], bd.grad if bd is not None else None


def _assert_dead_zero(case, dx):
    """Input samples no (output position, tap) reads have the gradient 0.0 exactly, not merely a small one."""
    dead = untouched_mask(case).to(dx.device)
    if bool(dead.any()):
        assert float(dx[..., dead].abs().max()) == 0.0, "dx is not exactly 0.0 where no output reads x"
    return int(dead.sum())


# ---- main comparison ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GPU_CASES, ids=IDS)
def test_geometry_vs_oracle(case):
    _, _, H = _mods()
    (x, ws, bias, cot), (yr, dxr, dwr, dbr) = _oracle(case)
    y, dx, dws, db = _run(H, case, x, ws, bias, cot)
    for t in [y, dx] + dws + ([db] if db is not None else []):
        assert not bool(torch.isnan(t).any())
    _check("y", y, yr)
    _check("dx", dx, dxr)
    for i, (a, b) in enumerate(zip(dws, dwr)):
        _check(f"dw{i}", a, b)
    if db is not None:
        _check("dbias", db, dbr)
    _assert_dead_zero(case, dx)


def test_some_case_has_untouched_samples_per_rank():
    for nd in (1, 2):
        assert any(bool(untouched_mask(c)[..., -1].any()) for c in GPU_CASES if geometry(c)["nd"] == nd)


@pytest.mark.parametrize("case", FIXTURE_CASES, ids=[c["name"] for c in FIXTURE_CASES])
def test_fixture_forward_backward(golden, case):
    _, _, H = _mods()
    g = golden("conv_geometry")
    n = case["name"]
    x, ws, bias = fixture_inputs(case)
    yshape = g[n + ".y"].shape
    y, dx, dws, db = _run(H, case, x, ws, bias, fixture_cotangent(yshape))
    _check("y", y, g[n + ".y"])
    _check("dx", dx, g[n + ".dx"])
    for i, w in enumerate(dws):
        _check(f"dw{i}", w, g[f"{n}.dw{i}"])
    if db is not None:
        _check("dbias", db, g[n + ".dbias"])
    _assert_dead_zero(case, dx)


# ---- unwritten and untouched elements ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GPU_CASES, ids=IDS)
def test_prefilled_output_and_gradient_slots(case):
    """The forward kernel writes every element of a NaN-filled output; the accumulating weight-gradient entry ADDS to
    non-zero slots; the data gradient (written into torch.empty memory) holds no NaN and exact zeros where it must."""
    _, _, H = _mods()
    (x, ws, bias, cot), (yr, dxr, dwr, dbr) = _oracle(case)
    desc = _desc(H, case)
    xd, wd, cd = x.to(DEV), [w.to(DEV) for w in ws], cot.to(DEV)
    bd = bias.to(DEV) if bias is not None else None
    y = torch.full(tuple(yr.shape), float("nan"), device=DEV)
    assert H.conv_fwd(desc, xd, wd, bd, out=y) is y
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y).any()), "an output element was not written"
    _check("y into a NaN-filled buffer", y, yr)
    slots = [torch.full(weight_shape(case), 0.5 + 0.25 * c, device=DEV) for c in range(case["algebra"])]
    bslot = torch.full((case["cout"],), -0.75, device=DEV) if bias is not None else None
    H.conv_bwd_weight(desc, xd, cd, weight_shape(case), bias is not None, into=slots, bias_into=bslot)
    torch.cuda.synchronize()
    for c, (a, b) in enumerate(zip(slots, dwr)):
        _check(f"dw{c} added to {0.5 + 0.25 * c}", a.double().cpu() - (0.5 + 0.25 * c), b)
    if bslot is not None:
        _check("dbias added to -0.75", bslot.double().cpu() + 0.75, dbr)
    dx = H.conv_bwd_data(desc, cd, wd, tuple(case["x"]))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dx).any())
    _check("dx", dx, dxr)
    _assert_dead_zero(case, dx)


# ---- kernel census -------------------------------------------------------------------------------------------------------
def _labels(H, case):
    """The kernel symbols hyper_conv's forward, data gradient and weight gradient launch for a case."""
    d = _desc(H, case)
    out = []
    for which in (0, 1):
        out.append(H.hcq_label(d, which) if H._hcq_ok(d, which) else H._label(d, which))
    if not case["bias"] and H._hcq_wgrad_ok(d):
        out.append(H._hcq_wgrad_label(d))
    else:
        out.append(H._label(d, 2))
    return out


def test_kernel_census():
    """Label grammar (seld_hc_conv_kernel_label, hc_wgrad_label): hc_conv_kernel<CT, PT, KH, KW, MODE, FAST> with
    KH = KW = 0 the generic-tap instantiation; hc_wgrad_kernel / hc_wgrad32_kernel<WRW, RT, CTL, KH, KW>;
    hc_wgrad_row_kernel<WRW, RT, CTL, KH, KW, FUSED>."""
    _, _, H = _mods()
    census = {}
    lab = {}
    for c in GPU_CASES:
        lab[c["name"]] = _labels(H, c)
        for which, l in enumerate(lab[c["name"]]):
            census.setdefault(l.split("<")[0] + ("", " as data gradient", "")[which], []).append(f"{c['name']}: {l}")
    for fam in sorted(census):
        print(fam)
        for line in census[fam]:
            print("   ", line)
    G = {c["name"]: geometry(c) for c in GPU_CASES}
    strided = [n for n in lab if max(G[n]["s"]) > 1]
    sh2 = [n for n in lab if G[n]["nd"] == 2 and G[n]["s"][0] > 1]
    fwd = lambda n: lab[n][0]
    dgr = lambda n: lab[n][1]
    wgr = lambda n: lab[n][2]
    assert any(re.fullmatch(r"hc_conv_kernel<\d+, \d+, 0, 0, 0, 0>", fwd(n)) for n in lab)
    assert any(re.fullmatch(r"hc_conv_kernel<\d+, \d+, (1, 1|1, 3|3, 3), 0, 1>", fwd(n)) for n in strided)
    assert any(re.fullmatch(r"hc_conv_kernel<\d+, \d+, 3, 3, 0, 1>", fwd(n)) for n in sh2)
    assert any(re.fullmatch(r"hc_conv_kernel<\d+, \d+, \d+, \d+, 1, 0>", dgr(n)) for n in strided)
    assert all(re.fullmatch(r"hc_conv_kernel<\d+, \d+, 0, 0, 1, 0>", dgr(n)) for n in strided)    # no fast strided dgrad
    assert any(re.fullmatch(r"hc_wgrad_kernel<\d+, \d+, \d+, 0, 0>", wgr(n)) for n in lab)
    assert any(wgr(n).startswith("hc_wgrad32_kernel<") for n in sh2)
    assert any(re.fullmatch(r"hc_wgrad32_kernel<\d+, \d+, \d+, 0, 0>", wgr(n)) for n in lab)
    row = [n for n in lab if wgr(n).startswith("hc_wgrad_row_kernel<")]
    assert any(n in sh2 for n in row), "row-chunk weight gradient with sh > 1"
    assert any(set(G[n]["p"]) == {0} and G[n]["k"] == (3, 3) for n in row), "row-chunk weight gradient with pad 0"
    assert any(G[n]["nd"] == 2 and G[n]["d"][0] == 2 for n in row), "row-chunk weight gradient with dil_h = 2"
    # one step outside a gate: never a fast-product kernel
    for c in GPU_CASES:
        d = _desc(H, c)
        if c["edge"] or max(G[c["name"]]["s"]) > 1 or (G[c["name"]]["nd"] == 2 and G[c["name"]]["d"][0] != 1):
            assert not H._hcq_ok(d, 0) and not H._hcq_ok(d, 1) and not H._hcq_ok(d, 0, 2) and not H._hcq_ok(d, 1, 2), c["name"]
            assert not H._hcq_wgrad_ok(d), c["name"]
            assert not any(l.startswith("hcq_") for l in lab[c["name"]]), (c["name"], lab[c["name"]])
            assert H.wgrad_group_family(d) == -1, c["name"]
        # strided shapes stay off the stride-1 staging kernels too
        if max(G[c["name"]]["s"]) > 1:
            assert not any(l.startswith(("hc_conv_vec_kernel<", "hc_conv_smallk_kernel<")) for l in lab[c["name"]][:2])


# ---- neighbouring entry points on the generic kernels ------------------------------------------------------------------------
NEIGHBOURS = ["dq1d_k5_s3_p2_d2", "dq2d_k31_s21_p10", "dq2d_fast_row_s21", "q1d_k5_s2_p2", "dq1d_k7_s2_p3"]


def _stats_close(H, stats_rep, ref):
    cout = ref.shape[1]
    stats = stats_rep.view(H.STATS_REPLICAS, 2 * cout).sum(0).double().cpu()
    red = tuple(i for i in range(ref.dim()) if i != 1)
    assert torch.allclose(stats[:cout], ref.sum(dim=red), rtol=1e-4, atol=1e-3)
    assert torch.allclose(stats[cout:], (ref * ref).sum(dim=red), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("name", NEIGHBOURS)
def test_add_and_epilogues(name):
    _, L, H = _mods()
    case = BY_NAME[name]
    assert not H._hcq_ok(_desc(H, case), 0)
    (x, ws, bias, cot), (yr, dxr, dwr, dbr) = _oracle(case)
    gen = torch.Generator().manual_seed(21)
    addend = torch.randn(tuple(yr.shape), generator=gen)
    ref2 = yr + addend.double()
    # hyper_conv_add through autograd
    xd = x.to(DEV).requires_grad_(True)
    wd = [w.to(DEV).requires_grad_(True) for w in ws]
    bd = bias.to(DEV).requires_grad_(True)
    ad = addend.to(DEV).requires_grad_(True)
    y = H.hyper_conv_add(xd, wd, bd, ad, case["stride"], case["padding"], case["dilation"])
    (y * cot.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _check("conv + addend", y, ref2)
    _check("dx", xd.grad, dxr)
    for i, (a, b) in enumerate(zip(wd, dwr)):
        _check(f"dw{i}", a.grad, b)
    _check("dbias", bd.grad, dbr)
    _check("d addend", ad.grad, cot)
    # the fused epilogues
    desc = _desc(H, case)
    wdd = [w.detach() for w in wd]
    stats_rep = H.new_stats(case["cout"], DEV)
    y2 = H.conv_fwd(desc, xd.detach(), wdd, bd.detach(), epilogue=L.SELD_EPI_ADD | L.SELD_EPI_STATS, addend=ad.detach(),
                    stats=stats_rep)
    torch.cuda.synchronize()
    _check("ADD | STATS output", y2, ref2)
    _stats_close(H, stats_rep, ref2)
    acc = ad.detach().clone()
    H.conv_fwd(desc, xd.detach(), wdd, bd.detach(), out=acc, epilogue=L.SELD_EPI_ACCUMULATE)
    torch.cuda.synchronize()
    _check("ACCUMULATE", acc, ref2)


@pytest.mark.parametrize("name", NEIGHBOURS)
def test_pair_falls_back_to_two_calls(name):
    """hyper_conv_pair on shapes no pair data-gradient kernel takes (and, but for the row-chunk case, no pair weight
    gradient either): the outputs, the summed data gradient and both sets of weight gradients equal the two single
    calls'; set A also against the oracle."""
    _, _, H = _mods()
    case = BY_NAME[name]
    desc = _desc(H, case)
    assert not H._pair_ok(desc, 1) and not H._hcq_ok(desc, 0, 2)
    assert H._pair_ok(desc, 2) == H._label(desc, 2).startswith("hc_wgrad_row_kernel<")
    (x, ws, bias, cot), (yr, dxr, dwr, dbr) = _oracle(case)
    gen = torch.Generator().manual_seed(99)
    wsB = [torch.randn(weight_shape(case), generator=gen) * 0.2 for _ in ws]
    biasB = torch.randn(case["cout"], generator=gen)
    cotB = torch.randn(tuple(yr.shape), generator=gen)
    s, p, d = case["stride"], case["padding"], case["dilation"]

    def run(pair):
        xs = x.to(DEV).requires_grad_(True)
        wl = [[w.to(DEV).requires_grad_(True) for w in wset] for wset in (ws, wsB)]
        bl = [b.to(DEV).requires_grad_(True) for b in (bias, biasB)]
        if pair:
            ya, yb = H.hyper_conv_pair(xs, wl[0], bl[0], wl[1], bl[1], s, p, d)
        else:
            ya, yb = H.hyper_conv(xs, wl[0], bl[0], s, p, d), H.hyper_conv(xs, wl[1], bl[1], s, p, d)
        ((ya * cot.to(DEV)).sum() + (yb * cotB.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        return [ya.detach(), yb.detach(), xs.grad] + [w.grad for w in wl[0] + wl[1]] + [b.grad for b in bl]

    got, ref = run(True), run(False)
    for i, (a, b) in enumerate(zip(got, ref)):
        _check(f"pair vs two calls [{i}]", a, b)
    A = case["algebra"]
    _check("yA", got[0], yr)
    for i in range(A):
        _check(f"dwA{i}", got[3 + i], dwr[i])
    _check("dbiasA", got[3 + 2 * A], dbr)
    _assert_dead_zero(case, got[2])
    if H._pair_ok(desc, 2):
        # the pair weight-gradient entry point itself (autograd takes it only with FlatAdam's gradient slots)
        P, L, _ = _mods()
        xd, ca, cb = x.to(DEV), cot.to(DEV), cotB.to(DEV)
        dwa = [torch.zeros(weight_shape(case), device=DEV) for _ in range(A)]
        dwb = [torch.zeros(weight_shape(case), device=DEV) for _ in range(A)]
        dba, dbb = torch.zeros(case["cout"], device=DEV), torch.zeros(case["cout"], device=DEV)
        L.check(L.lib().seld_hc_conv_pair_bwd_weight_acc(ctypes.byref(desc), L.ptr(xd), L.ptr(ca), L.ptr(cb),
                                                         L.ptr_array8(dwa), L.ptr_array8(dwb), L.ptr(dba), L.ptr(dbb),
                                                         L.current_stream()), "pair wgrad")
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(dwa + dwb + [dba, dbb], ref[3:])):
            _check(f"pair weight-gradient entry [{i}]", a, b)


@pytest.mark.parametrize("name", NEIGHBOURS)
def test_deterministic_mode(name, seld_env):
    _, _, H = _mods()
    case = BY_NAME[name]
    (x, ws, bias, cot), (yr, dxr, dwr, dbr) = _oracle(case)
    default = _run(H, case, x, ws, bias, cot)
    seld_env.set("SELD_DETERMINISTIC", "1")
    assert H.deterministic()
    one = _run(H, case, x, ws, bias, cot)
    two = _run(H, case, x, ws, bias, cot)
    flat = lambda r: [r[0], r[1]] + r[2] + [r[3]]
    for a, b in zip(flat(one), flat(two)):
        assert torch.equal(a, b), "SELD_DETERMINISTIC=1: two runs differ"
    for i, (a, b) in enumerate(zip(flat(one), flat(default))):
        _check(f"deterministic vs default [{i}]", a, b)
    for i, (a, b) in enumerate(zip(flat(one), [yr, dxr] + dwr + [dbr])):
        _check(f"deterministic vs oracle [{i}]", a, b)
    _assert_dead_zero(case, one[1])


# ---- layer plumbing -----------------------------------------------------------------------------------------------------
LAYERS = [
    # operation, x shape per 8 channels of width, kernel_size, stride, padding, dilatation
    ("convolution1d", (3, 37), 5, 2, 2, 1),
    ("convolution1d", (2, 41), 5, 3, 4, 2),
    ("convolution2d", (2, 11, 14), (3, 1), (2, 1), (1, 0), 1),
    ("convolution2d", (2, 13, 12), 5, 2, 2, 1),
]


@pytest.mark.parametrize("algebra", [4, 8])
@pytest.mark.parametrize("operation,xs,k,s,p,d", LAYERS)
def test_layers(algebra, operation, xs, k, s, p, d):
    P, _, _ = _mods()
    cin, cout = 2 * algebra, 3 * algebra
    if algebra == 4:
        m = P.quaternion.quaternion_layers.QuaternionConv(cin, cout, k, s, dilatation=d, padding=p, seed=3,
                                                          operation=operation)
        names = ("r_weight", "i_weight", "j_weight", "k_weight")
    else:
        m = P.dual_quaternion.dual_quaternion_layers.DualQuaternionConv(cin, cout, k, s, dilatation=d, padding=p, seed=3,
                                                                        operation=operation)
        names = ("r_weight", "i_weight", "j_weight", "k_weight", "r_weight_2", "i_weight_2", "j_weight_2", "k_weight_2")
    kk = (k,) if operation == "convolution1d" else ((k, k) if isinstance(k, int) else k)
    assert tuple(m.r_weight.shape) == (cout // algebra, cin // algebra) + kk
    gen = torch.Generator().manual_seed(8)
    with torch.no_grad():
        m.bias.copy_(torch.randn(cout, generator=gen))
    x = torch.randn((xs[0], cin) + tuple(xs[1:]), generator=gen)
    w64 = [getattr(m, n).detach().double().requires_grad_(True) for n in names]
    b64 = m.bias.detach().double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    yr = O.hypercomplex_conv(x64, w64, b64, s, p, 1, d, mode="explicit")
    cot = torch.randn(tuple(yr.shape), generator=gen)
    (yr * cot.double()).sum().backward()
    m = m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    (y * cot.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _check("y", y, yr)
    _check("dx", xd.grad, x64.grad)
    for n, w in zip(names, w64):
        _check("d" + n, getattr(m, n).grad, w.grad)
    _check("dbias", m.bias.grad, b64.grad)


# ---- requests that must raise rather than launch -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k,s,p,d", [((1, 8, 8), (5,), 1, 0, 3), ((1, 8, 4), (3,), 2, 0, 2),
                                           ((1, 8, 3, 9), (3, 3), (4, 1), 0, (2, 1))])
def test_kernel_longer_than_the_padded_input_raises_on_the_device(shape, k, s, p, d):
    P, L, H = _mods()
    x = torch.ones(shape, device=DEV)
    ws = [torch.ones((1, 1) + k, device=DEV) for _ in range(8)]
    with pytest.raises(L.SeldHipError):
        H.hyper_conv(x, ws, None, s, p, d)
    with pytest.raises(L.SeldHipError):
        H.hyper_conv_add(x, ws, None, x, s, p, d)
    with pytest.raises(L.SeldHipError):
        H.hyper_conv_pair(x, ws, None, ws, None, s, p, d)
    op = "convolution1d" if len(shape) == 3 else "convolution2d"
    m = P.dual_quaternion.dual_quaternion_layers.DualQuaternionConv(8, 8, k[0] if len(k) == 1 else k, s, dilatation=d,
                                                                    padding=p, seed=1, operation=op).to(DEV)
    with pytest.raises(L.SeldHipError):
        m(x)
    desc = H.make_conv_desc(shape, 8, 8, k, s, p, d)
    y = torch.full((64,), 7.0, device=DEV)
    rc = L.lib().seld_hc_conv_fwd_ex(ctypes.byref(desc), L.ptr(x), L.ptr_array8(ws), None, L.ptr(y), 0, None, None,
                                     L.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((y == 7.0).all())            # SELD_EINVAL, nothing written
