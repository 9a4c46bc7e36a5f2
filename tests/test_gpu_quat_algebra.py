"""Element-wise quaternion algebra on the MI355X (csrc/quat_algebra.hip) through the public functions of
quaternion_ops / dual_quaternion_ops: the reference fixture, a shape sweep and a full-size case against the float64
restatement, refused inputs, run-to-run identity, graph replay and two algebraic identities.

Every comparison is against a float64 result (the reference's, from the fixture, or the restatement's), bound
max |got - ref| <= 1e-5 * max |ref| per tensor: the project's bound for point-wise fp32 results."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.golden.quat_algebra_cases import CASE_IDS, QUAT_ALGEBRA_CASES, closed_form, quat_cotangent, quat_inputs
from tests.helpers import pkg
from tests.test_quat_algebra_host import MODULE_OPS, module_of, refused_meta, restated

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4            # include/seld_hip.h
TOL = 1e-5


def _err(got, ref, what):
    """max |got - ref| / max |ref| after the shapes are checked; no NaN on either side."""
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all() and torch.isfinite(ref).all(), what
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _run(fn, args, kwargs, cot=None):
    """fn forward + backward on the device: [y, d(args[0]), d(args[1])...] and the cotangent used."""
    dargs = [a.to(DEV).requires_grad_(True) for a in args]
    y = fn(*dargs, **kwargs)
    y.backward(cot(y.shape).to(DEV) if callable(cot) else cot.to(DEV))
    return [y] + [a.grad for a in dargs]


def _reference(op, args, kwargs, cot):
    rargs = [a.double().requires_grad_(True) for a in args]
    y = restated(op, rargs, kwargs)
    y.backward(cot.double())
    return [y.detach()] + [a.grad for a in rargs]


def _check(mod, op, args, kwargs, label):
    """One op against the float64 restatement on the same float32 inputs; returns the relative errors."""
    ref_y = restated(op, [a.double() for a in args], kwargs)
    cot = closed_form(tuple(ref_y.shape), 0.77)
    got = _run(getattr(mod, op), args, kwargs, cot)
    ref = _reference(op, args, kwargs, cot)
    errs = [_err(g, r, (label, k)) for k, (g, r) in enumerate(zip(got, ref))]
    assert max(errs) <= TOL, (label, errs)
    return errs


@pytest.mark.parametrize("case", QUAT_ALGEBRA_CASES, ids=CASE_IDS)
def test_fixture_through_public_functions(golden, case):
    g = golden("quat_algebra")
    L = pkg()._lib
    name = case["name"]
    fn = getattr(module_of(case), case["op"])
    kind = refused_meta(g).get(name)
    if kind is not None:
        with pytest.raises(RuntimeError if kind == "RuntimeError" else L.SeldHipError):
            fn(*[a.to(DEV) for a in quat_inputs(case)], **case["kwargs"])
        return
    got = _run(fn, quat_inputs(case), case["kwargs"], lambda shape: quat_cotangent(case, shape))
    keys = ["y", "dx", "dq1"][:len(got)]
    errs = {k: _err(t, g[f"{name}.{k}"], (name, k)) for k, t in zip(keys, got)}
    print(f"{name}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert max(errs.values()) <= TOL, errs


SWEEP_SHAPES = [
    (1, 4), (5, 4), (3, 36), (64, 128), (2100, 16), (1030, 64), (4099, 8), (300, 1028),
    (4, 7, 12), (2, 9, 64), (600, 3, 16), (1, 5, 8), (70, 33, 20),
    (2, 4, 3, 5), (3, 16, 4, 8), (1, 8, 1, 1), (40, 8, 6, 6), (2, 12, 3, 700),
    (2, 8, 2, 3, 4), (1, 4, 3, 3, 3), (3, 20, 2, 5, 6),
]


def _accepted(m, op, rank):
    if m == "Q":
        return rank in (2, 3) and not (op == "hamilton_product" and rank == 3)
    if op == "get_normalized":
        return rank in (2, 3)
    return not (op == "hamilton_product" and rank == 3)


def test_sweep_against_float64():
    p = pkg()
    mods = {"Q": p.quaternion.quaternion_ops, "D": p.dual_quaternion.dual_quaternion_ops}
    worst, count = {}, 0
    for (m, ops), (k, shape) in itertools.product(MODULE_OPS.items(), enumerate(SWEEP_SHAPES)):
        for op in ops:
            if not _accepted(m, op, len(shape)):
                continue
            variants = [{"vector_form": True}, {"vector_form": False}] if op == "get_modulus" else [{}]
            if op == "get_normalized":
                variants = [{}, {"eps": 0.05}]
            for kw in variants:
                args = [closed_form(shape, 0.3 + k + 2.1 * i) for i in range(2 if op == "hamilton_product" else 1)]
                errs = _check(mods[m], op, args, kw, (m, op, shape, kw))
                worst[op] = max([worst.get(op, 0.0)] + errs)
                count += 1
    print(f"quat algebra sweep: {count} calls, worst relative error per op " +
          " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_input_forms():
    """Non-contiguous inputs, a contiguous view that is not 16-byte aligned, inputs that only broadcast, and every
    `channel` of q_normalize."""
    D = pkg().dual_quaternion.dual_quaternion_ops
    base = closed_form((12, 40, 6), 0.4)
    _check(D, "q_normalize", [base.transpose(0, 2)], {}, "transposed 3-D")
    _check(D, "get_modulus", [base.transpose(1, 2)[:, :4]], {}, "sliced 3-D")
    flat = closed_form((8 * 64 + 3,), 1.4)

    def misaligned(args, kwargs, fn):
        dargs = [a.to(DEV)[3:].view(8, 64).requires_grad_(True) for a in args]
        assert all(a.data_ptr() % 16 == 12 and a.is_contiguous() for a in dargs)
        return fn(*dargs, **kwargs), dargs
    for op, kw in [("get_modulus", {"vector_form": True}), ("get_modulus", {}), ("get_normalized", {}),
                   ("q_normalize", {}), ("quaternion_exp", {}), ("hamilton_product", {})]:
        args = [flat, flat.flip(0)][:2 if op == "hamilton_product" else 1]
        y, dargs = misaligned(args, kw, getattr(D, op))
        cot = closed_form(tuple(y.shape), 0.9)
        y.backward(cot.to(DEV))
        ref = _reference(op, [a[3:].view(8, 64) for a in args], kw, cot)
        errs = [_err(t, r, (op, "misaligned")) for t, r in zip([y] + [a.grad for a in dargs], ref)]
        assert max(errs) <= TOL, (op, errs)
    # inputs that only broadcast are expanded: q1 one row, and a 4-D q1 with singleton spatial extents
    q0, q1 = closed_form((6, 24), 0.2), closed_form((1, 24), 1.2)
    got = _run(D.hamilton_product, [q0, q1], {}, closed_form((6, 24), 2.2))
    ref = _reference("hamilton_product", [q0, q1.expand(6, 24)], {}, closed_form((6, 24), 2.2))
    assert _err(got[0], ref[0], "broadcast y") <= TOL and _err(got[1], ref[1], "broadcast dq0") <= TOL
    assert _err(got[2], ref[2].sum(0, keepdim=True), "broadcast dq1") <= TOL
    x4 = closed_form((2, 8, 3, 5), 0.6)
    for shape, channels in [((5, 12), (0, 1, -1, -2)), ((3, 5, 12), (0, 1, 2, -1, -3)), ((2, 8, 3, 5), (0, 1, 2, 3, -1)),
                            ((2, 4, 2, 3, 4), (1, 4, -4))]:
        for ch in channels:
            _check(D, "q_normalize", [closed_form(shape, 0.1 * ch + 1.0)], {"channel": ch}, (shape, ch))
    with pytest.raises(IndexError):
        D.q_normalize(x4.to(DEV), channel=4)


def test_zero_quaternions_give_finite_values_and_gradients():
    """Forward values at q = 0 are the reference's; q_normalize's gradient there is 100 dy; the other gradients take the
    factor 0 where the reference's autograd divides 0 by 0, so nothing is NaN."""
    D = pkg().dual_quaternion.dual_quaternion_ops
    x = closed_form((6, 16), 0.3)
    x.view(6, 4, 4)[1::2, :, 1] = 0.0                              # quaternion 1 of rows 1, 3, 5
    x.view(6, 4, 4)[2, 1:, 3] = 0.0                                # quaternion 3 of row 2: i = j = k = 0, r kept
    cot = closed_form((6, 16), 1.9)
    cv = cot.view(6, 4, 4)
    for op, kw in [("get_modulus", {"vector_form": True}), ("get_modulus", {}), ("get_normalized", {}),
                   ("q_normalize", {}), ("quaternion_exp", {})]:
        got = _run(getattr(D, op), [x], kw, closed_form(tuple(restated(op, [x], kw).shape), 1.9))
        y64 = restated(op, [x.double()], kw)
        assert _err(got[0], y64, op) <= TOL
        assert torch.isfinite(got[1]).all(), op
        dx = got[1].cpu().view(6, 4, 4)
        if op == "q_normalize":
            assert _err(dx[1::2, :, 1], 100.0 * cv[1::2, :, 1], "q_normalize at 0") <= TOL
        if op == "get_modulus" and kw.get("vector_form"):
            assert (dx[1::2, :, 1] == 0).all()
        if op == "quaternion_exp":
            n = torch.tensor(1e-4, dtype=torch.float64)
            e = x.double().view(6, 4, 4)[2, 0, 3].exp()
            want = torch.stack([e * n.cos() * cv[2, 0, 3].double()] + [e * n.sin() / n * cv[2, c, 3].double()
                                                                        for c in (1, 2, 3)])
            assert _err(dx[2, :, 3], want, "quaternion_exp at v = 0") <= TOL
    y = D.quaternion_exp(torch.zeros(2, 8, device=DEV)).cpu()
    assert torch.equal(y[:, 2:], torch.zeros(2, 6)) and _err(y[:, :2], torch.full((2, 2), np.cos(1e-4)), "exp(0)") <= TOL
    assert torch.equal(D.q_normalize(torch.zeros(2, 8, device=DEV)).cpu(), torch.zeros(2, 8))


def _all_ops(D, x2, x3, q1):
    outs = []
    for x in (x2, x3):
        for fn, kw in [(D.get_modulus, {"vector_form": True}), (D.get_modulus, {}), (D.get_normalized, {}),
                       (D.q_normalize, {}), (D.quaternion_exp, {})]:
            y = fn(x, **kw)
            outs += [y, torch.autograd.grad(y, x, torch.cos(y))[0]]
    y = D.hamilton_product(x2, q1)
    return outs + [y] + list(torch.autograd.grad(y, (x2, q1), torch.cos(y)))


def test_two_runs_are_bit_identical(seld_env):
    D = pkg().dual_quaternion.dual_quaternion_ops
    x2 = closed_form((5000, 64), 0.3).to(DEV).requires_grad_(True)
    x3 = closed_form((700, 5, 24), 0.8).to(DEV).requires_grad_(True)
    q1 = closed_form((5000, 64), 1.3).to(DEV).requires_grad_(True)
    a = _all_ops(D, x2, x3, q1)
    b = _all_ops(D, x2, x3, q1)
    seld_env.set("SELD_DETERMINISTIC", "1")
    c = _all_ops(D, x2, x3, q1)
    seld_env.unset("SELD_DETERMINISTIC")
    for k, (ta, tb, tc) in enumerate(zip(a, b, c)):
        assert torch.equal(ta, tb), k
        assert torch.equal(ta, tc), k


def test_graph_capture_and_replay():
    """Every op, forward and backward, captured in a graph and replayed on new inputs equals the eager result: nothing
    on the path synchronises with the host, and the reduction workspaces come from the graph's pool."""
    D = pkg().dual_quaternion.dual_quaternion_ops
    x2 = closed_form((1200, 32), 0.3).to(DEV).requires_grad_(True)
    x3 = closed_form((300, 6, 16), 0.8).to(DEV).requires_grad_(True)
    q1 = closed_form((1200, 32), 1.3).to(DEV).requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _all_ops(D, x2, x3, q1)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = _all_ops(D, x2, x3, q1)
    with torch.no_grad():
        for t in (x2, x3, q1):
            t.mul_(0.7).add_(0.05)
    g.replay()
    torch.cuda.synchronize()
    eager = _all_ops(D, x2, x3, q1)
    for k, (a, b) in enumerate(zip(static, eager)):
        assert torch.equal(a, b), k


def test_refused_inputs_launch_nothing(golden):
    from torch.profiler import ProfilerActivity, profile
    L = pkg()._lib
    lib = L.lib()
    meta = refused_meta(golden("quat_algebra"))
    calls = []
    for case in QUAT_ALGEBRA_CASES:
        if case["name"] in meta:
            kind = RuntimeError if meta[case["name"]] == "RuntimeError" else L.SeldHipError
            calls.append((getattr(module_of(case), case["op"]), [a.to(DEV) for a in quat_inputs(case)], case["kwargs"],
                          kind))
    D = pkg().dual_quaternion.dual_quaternion_ops
    calls.append((D.hamilton_product, [torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, 1, 1, device=DEV)], {},
                  L.SeldHipError))
    calls.append((D.hamilton_product, [torch.zeros(4, 8, device=DEV), torch.zeros(3, 8, device=DEV)], {}, RuntimeError))
    calls.append((D.quaternion_exp, [torch.zeros(4, 8, device=DEV, dtype=torch.float64)], {}, L.SeldHipError))
    x = torch.zeros(1 << 12, device=DEV)
    y = torch.full((1 << 12,), 7.0, device=DEV)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for fn, args, kw, kind in calls:
            with pytest.raises(kind):
                fn(*args, **kw)
        st = L.current_stream()
        for dims, want in [((8, 1, 10, 1), EINVAL), ((8, 3, 6, 5), EINVAL), ((0, 1, 8, 1), EINVAL),
                           ((2 ** 16, 1, 2 ** 16, 2), EUNSUPPORTED)]:
            s = L.QuatShape(*dims)
            b = ctypes.byref(s)
            rcs = [lib.seld_quat_modulus_fwd(b, L.ptr(x), L.ptr(y), st),
                   lib.seld_quat_modulus_sum_fwd(b, L.ptr(x), L.ptr(y), L.ptr(y), 1 << 14, st),
                   lib.seld_quat_normalized_bwd(b, L.ptr(x), L.ptr(x), L.ptr(x), 1e-4, L.ptr(y), L.ptr(y), 1 << 14, st),
                   lib.seld_quat_normalize_fwd(b, 1, L.ptr(x), L.ptr(y), st),
                   lib.seld_quat_exp_bwd(b, 1, L.ptr(x), L.ptr(x), L.ptr(y), st),
                   lib.seld_quat_hamilton_bwd(b, L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(y), L.ptr(y), st)]
            assert rcs == [want] * len(rcs), (dims, rcs)
        ok = L.QuatShape(8, 1, 16, 1)
        assert lib.seld_quat_modulus_sum_fwd(ctypes.byref(ok), L.ptr(x), L.ptr(y), L.ptr(y), 16, st) == EWORKSPACE
        assert lib.seld_quat_normalize_fwd(ctypes.byref(ok), 5, L.ptr(x), L.ptr(y), st) == EINVAL
        torch.cuda.synchronize()
    launched = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    assert not launched, launched
    assert bool((y == 7.0).all()), "output written by a refused call"


def test_algebraic_identities():
    """q (x) (conj(q) / |q|^2) is the identity quaternion, and q_normalize gives unit modulus once |q|^2 >= 25 makes
    its 1e-4 inside the root smaller than the bound (relative effect 1e-4 / (2 |q|^2) <= 2e-6)."""
    D = pkg().dual_quaternion.dual_quaternion_ops
    Q = pkg().quaternion.quaternion_ops
    for mod, shape in [(Q, (37, 44)), (D, (37, 44)), (D, (3, 12, 5, 7)), (D, (2, 8, 2, 3, 3))]:
        x = closed_form(shape, 0.5)
        axis = 1
        n = shape[axis] // 4
        x.narrow(axis, 0, n).copy_(5.0 + x.narrow(axis, 0, n) ** 2)
        x64 = x.double()
        sq = sum(c * c for c in x64.chunk(4, axis))
        conj = torch.cat([x64.narrow(axis, 0, n), -x64.narrow(axis, n, 3 * n)], axis) / torch.cat([sq] * 4, axis)
        y = mod.hamilton_product(x.to(DEV), conj.float().to(DEV))
        one = torch.cat([torch.ones_like(sq), torch.zeros_like(sq), torch.zeros_like(sq), torch.zeros_like(sq)], axis)
        e1 = _err(y, one, ("identity", shape))
        e2 = _err(D.get_modulus(D.q_normalize(x.to(DEV)), vector_form=True), torch.ones_like(sq), ("unit", shape))
        print(f"identities {shape}: product {e1:.2e} unit modulus {e2:.2e}")
        assert e1 <= TOL and e2 <= TOL, (shape, e1, e2)


def test_full_size_against_float64():
    """(32, 192, 8, 512), 50 MB per tensor, through the dual-quaternion functions (get_normalized takes rank 2 and 3
    only, as in the reference)."""
    D = pkg().dual_quaternion.dual_quaternion_ops
    shape = (32, 192, 8, 512)
    x, q1 = closed_form(shape, 0.3), closed_form(shape, 1.7)
    for op, kw in [("get_modulus", {"vector_form": True}), ("get_modulus", {}), ("q_normalize", {}),
                   ("quaternion_exp", {}), ("hamilton_product", {})]:
        errs = _check(D, op, [x, q1][:2 if op == "hamilton_product" else 1], kw, ("full size", op))
        print(f"full size {shape} {op} {kw}: " + " ".join(f"{e:.2e}" for e in errs))
        torch.cuda.empty_cache()
    with pytest.raises(pkg()._lib.SeldHipError):
        D.get_normalized(x.to(DEV))
