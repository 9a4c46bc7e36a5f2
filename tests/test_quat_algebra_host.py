"""Element-wise quaternion algebra without a GPU: the fixture (tests/golden/quat_algebra.npz, made by the reference's
quaternion_ops / dual_quaternion_ops) against a float64 restatement of the formulas, the public names and their
signatures, which inputs are refused before the device is touched, and the C ABI (symbols, workspace, refusals)."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests.golden.quat_algebra_cases import CASE_IDS, QUAT_ALGEBRA_CASES, quat_cotangent, quat_inputs
from tests.helpers import pkg

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4            # include/seld_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["seld_quat_modulus_fwd", "seld_quat_modulus_bwd", "seld_quat_reduce_workspace", "seld_quat_modulus_sum_fwd",
         "seld_quat_modulus_sum_bwd", "seld_quat_normalized_fwd", "seld_quat_normalized_bwd", "seld_quat_normalize_fwd",
         "seld_quat_normalize_bwd", "seld_quat_exp_fwd", "seld_quat_exp_bwd", "seld_quat_hamilton_fwd",
         "seld_quat_hamilton_bwd"]
# name -> (parameter, default) list, as in the reference's two modules
SIGNATURES = {
    "get_modulus": [("input", inspect.Parameter.empty), ("vector_form", False)],
    "get_normalized": [("input", inspect.Parameter.empty), ("eps", 0.0001)],
    "hamilton_product": [("q0", inspect.Parameter.empty), ("q1", inspect.Parameter.empty)],
    "q_normalize": [("input", inspect.Parameter.empty), ("channel", 1)],
    "quaternion_exp": [("input", inspect.Parameter.empty)],
}
MODULE_OPS = {"Q": ["get_modulus", "get_normalized", "hamilton_product"],
              "D": ["get_modulus", "get_normalized", "hamilton_product", "q_normalize", "quaternion_exp"]}
# what each module refuses: rank (the Q module takes 2 and 3 only; get_normalized has no branch past rank 3; the product
# concatenates on dim 1 and so cannot take rank 3) or a component axis that 4 does not divide
REFUSED = {"q_ham_3d", "q_modv_4d", "q_mods_5d", "q_norm_4d", "q_ham_4d", "q_mods_2d_bad", "q_norm_3d_bad",
           "q_ham_2d_bad", "d_ham_3d", "d_norm_4d", "d_norm_5d", "d_unit_2d_bad", "d_mods_4d_bad", "d_exp_3d_bad"}


def module_of(case):
    p = pkg()
    return p.quaternion.quaternion_ops if case["module"] == "Q" else p.dual_quaternion.dual_quaternion_ops


def refused_meta(g):
    return json.loads(str(g["meta"]))["refused"]


def _quats(x):
    """x as (R, S, 4, M): dim 0, the middle extent of a 3-D input (else 1), component, everything else."""
    s = x.shape
    if x.dim() == 2:
        return x.reshape(s[0], 1, 4, s[1] // 4)
    if x.dim() == 3:
        return x.reshape(s[0], s[1], 4, s[2] // 4)
    return x.reshape(s[0], 1, 4, -1)


def _small_shape(x):
    """The input's shape with the component axis divided by 4."""
    s = list(x.shape)
    s[-1 if x.dim() < 4 else 1] //= 4
    return s


def _on_channel(y, x, channel):
    """y (laid out like x): its four components concatenated on `channel`."""
    axis = x.dim() - 1 if x.dim() < 4 else 1
    return torch.cat(torch.chunk(y, 4, dim=axis), dim=channel)


def restated(op, args, kwargs):
    """The five functions in terms of the (R, S, 4, M) view, any float dtype, differentiable."""
    x = args[0]
    v = _quats(x)
    sq = (v * v).sum(2)                                           # |q|^2, (R, S, M)
    if op == "get_modulus":
        if kwargs.get("vector_form", False):
            return sq.sqrt().reshape(_small_shape(x))
        return sq.sum(0).sqrt().reshape(_small_shape(x)[1:])
    if op == "get_normalized":
        d = sq.sum(0).sqrt() + kwargs.get("eps", 0.0001)          # (S, M)
        return (v / d[None, :, None, :]).reshape(x.shape)
    if op == "q_normalize":
        y = (v / (sq + 1e-4).sqrt()[:, :, None, :]).reshape(x.shape)
        return _on_channel(y, x, kwargs.get("channel", 1))
    if op == "quaternion_exp":
        r, u = v[:, :, 0], v[:, :, 1:]
        n = (u * u).sum(2).sqrt() + 1e-4
        y = torch.cat([(r.exp() * n.cos())[:, :, None], (r.exp() * n.sin() / n)[:, :, None] * u], 2).reshape(x.shape)
        return _on_channel(y, x, 1)
    if op == "hamilton_product":
        a, b = v.unbind(2), _quats(args[1]).unbind(2)
        y = torch.stack([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                         a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                         a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], 2)
        return y.reshape(x.shape)
    raise KeyError(op)


def restated_with_grads(case, dtype=torch.float64, args=None, cot=None):
    """y, dx (and dq1) of the restatement for the case's closed-form inputs and cotangent (or the given ones)."""
    args = [a.detach().to(dtype).requires_grad_(True) for a in (args or quat_inputs(case, dtype))]
    y = restated(case["op"], args, case["kwargs"])
    cot = quat_cotangent(case, y.shape, dtype) if cot is None else cot.to(dtype)
    (y * cot).sum().backward()
    return [y.detach()] + [a.grad for a in args]


def test_refused_cases_are_the_documented_ones(golden):
    g = golden("quat_algebra")
    meta = refused_meta(g)
    assert set(meta) == REFUSED
    assert {n for n, t in meta.items() if t != "RuntimeError"} == {"d_norm_4d", "d_norm_5d"}
    for c in QUAT_ALGEBRA_CASES:
        assert (c["name"] + ".y" in g) != (c["name"] in meta), c["name"]


@pytest.mark.parametrize("case", [c for c in QUAT_ALGEBRA_CASES if c["name"] not in REFUSED],
                         ids=[n for n in CASE_IDS if n not in REFUSED])
def test_fixture_agrees_with_float64_restatement(golden, case):
    g = golden("quat_algebra")
    got = restated_with_grads(case)
    keys = ["y", "dx", "dq1"][:len(got)]
    assert ("dq1" in keys) == (case["op"] == "hamilton_product")
    for what, t in zip(keys, got):
        ref = g[f"{case['name']}.{what}"].astype(np.float64)
        assert np.isfinite(ref).all(), what
        assert tuple(t.shape) == ref.shape, (what, t.shape, ref.shape)
        err = np.abs(t.numpy() - ref).max()
        assert err <= 2e-6 * max(np.abs(ref).max(), 1e-30), (what, err)


def test_fixture_tells_the_three_regularisations_apart():
    """1e-4 inside the root (q_normalize), outside it (quaternion_exp), eps added to the summed root (get_normalized):
    with each constant moved, the restatement leaves the fixture's bound by a wide margin."""
    for name in ("d_unit_2d", "d_unit_3d", "d_unit_4d", "d_exp_2d", "d_exp_3d", "d_exp_5d"):
        x = quat_inputs(next(c for c in QUAT_ALGEBRA_CASES if c["name"] == name), torch.float64)[0]
        v = _quats(x)
        sq = (v * v).sum(2)
        inside = v / (sq + 1e-4).sqrt()[:, :, None, :]
        outside = v / (sq.sqrt() + 1e-4)[:, :, None, :]
        assert sq.sqrt().min().item() < 0.2, name
        assert (inside - outside).abs().max().item() > 1e-3 * inside.abs().max().item(), name


def test_public_names_and_signatures():
    p = pkg()
    mods = {"Q": p.quaternion.quaternion_ops, "D": p.dual_quaternion.dual_quaternion_ops}
    for m, ops in MODULE_OPS.items():
        for name in ops:
            sig = inspect.signature(getattr(mods[m], name))
            assert [(k, v.default) for k, v in sig.parameters.items()] == SIGNATURES[name], (m, name, sig)
    for name in ("q_normalize", "quaternion_exp"):
        assert not hasattr(mods["Q"], name), name            # the reference's quaternion_ops has neither


@pytest.mark.parametrize("case", QUAT_ALGEBRA_CASES, ids=CASE_IDS)
def test_host_tensors_and_refused_inputs_raise(golden, case):
    """The package has no CPU path: an accepted case raises SeldHipError for a host tensor; a refused case raises its
    listed type (SeldHipError where the reference dies with UnboundLocalError) before the device matters."""
    L = pkg()._lib
    fn = getattr(module_of(case), case["op"])
    kind = refused_meta(golden("quat_algebra")).get(case["name"])
    want = L.SeldHipError if kind in (None, "UnboundLocalError") else RuntimeError
    with pytest.raises(want) as e:
        fn(*quat_inputs(case), **case["kwargs"])
    if kind == "UnboundLocalError":
        assert "rank %d" % len(case["shape"]) in str(e.value)
    if kind is None:
        assert "no CPU path" in str(e.value)


def test_header_declares_and_library_exports_entry_points():
    with open(os.path.join(ROOT, "include", "seld_hip.h")) as f:
        header = f.read()
    lib = pkg()._lib.lib()
    for name in NAMES:
        assert f"{name}(" in header, name
        assert hasattr(lib, name), name


def _all_calls(lib, s, ws=None, ws_bytes=0, p=None):
    b = ctypes.byref(s)
    e = 1e-4
    return [lib.seld_quat_modulus_fwd(b, p, p, None),
            lib.seld_quat_modulus_bwd(b, p, p, p, None),
            lib.seld_quat_modulus_sum_fwd(b, p, p, ws, ws_bytes, None),
            lib.seld_quat_modulus_sum_bwd(b, p, p, p, p, None),
            lib.seld_quat_normalized_fwd(b, p, p, e, p, None),
            lib.seld_quat_normalized_bwd(b, p, p, p, e, p, ws, ws_bytes, None),
            lib.seld_quat_normalize_fwd(b, 1, p, p, None),
            lib.seld_quat_normalize_bwd(b, 1, p, p, p, None),
            lib.seld_quat_exp_fwd(b, 0, p, p, None),
            lib.seld_quat_exp_bwd(b, 0, p, p, p, None),
            lib.seld_quat_hamilton_fwd(b, p, p, p, None),
            lib.seld_quat_hamilton_bwd(b, p, p, p, p, p, None)]


def test_refused_extents_without_gpu():
    """Host-side argument checking: every entry point refuses before it touches the device."""
    L = pkg()._lib
    lib = L.lib()
    p = ctypes.c_void_p(64)
    ok = L.QuatShape(8, 3, 16, 5)
    assert lib.seld_quat_reduce_workspace(ctypes.byref(ok)) >= 4 * 2 * 3 * 4 * 5
    for dims in [(8, 1, 10, 1), (8, 3, 6, 5), (8, 1, 0, 1), (0, 1, 8, 1), (8, 0, 8, 1), (8, 1, 8, 0), (8, 1, -4, 1)]:
        bad = L.QuatShape(*dims)
        assert set(_all_calls(lib, bad, p, 1 << 20, p)) == {EINVAL}, dims
        assert lib.seld_quat_reduce_workspace(ctypes.byref(bad)) == 0, dims
    big = L.QuatShape(2 ** 16, 1, 2 ** 16, 2)                      # 2^31 quaternions
    assert set(_all_calls(lib, big, p, 1 << 20, p)) == {EUNSUPPORTED}
    assert lib.seld_quat_reduce_workspace(ctypes.byref(big)) == 0
    # a valid shape: missing buffers, an unknown layout, then too small a workspace (checked before any launch)
    assert set(_all_calls(lib, ok)) == {EINVAL}
    assert lib.seld_quat_normalize_fwd(ctypes.byref(ok), 2, p, p, None) == EINVAL
    assert lib.seld_quat_exp_bwd(ctypes.byref(ok), -1, p, p, p, None) == EINVAL
    assert lib.seld_quat_modulus_sum_fwd(ctypes.byref(ok), p, p, None, 0, None) == EWORKSPACE
    assert lib.seld_quat_modulus_sum_fwd(ctypes.byref(ok), p, p, p, 64, None) == EWORKSPACE
    assert lib.seld_quat_normalized_bwd(ctypes.byref(ok), p, p, p, 1e-4, p, p, 64, None) == EWORKSPACE


def test_workspace_holds_every_partial_and_the_folded_row():
    """The sum over dim 0 is split into slices of dim 0; the workspace is one row of (mid * M) floats per slice plus the
    folded row, and grows with dim 0 once one slice no longer covers it."""
    L = pkg()._lib
    lib = L.lib()

    def ws(*dims):
        return lib.seld_quat_reduce_workspace(ctypes.byref(L.QuatShape(*dims)))
    for dims in [(1, 1, 4, 1), (7, 1, 20, 1), (3, 5, 12, 1), (32, 1, 192, 4096), (16384, 1, 768, 1), (2100, 1, 4, 1)]:
        row = 4 * dims[1] * (dims[2] // 4) * dims[3]
        n = ws(*dims)
        assert n >= 2 * row and n % row == 0, dims
    assert ws(2100, 1, 4, 1) > ws(7, 1, 4, 1)                       # the long fixture cases use more than one partial
    assert ws(600, 2, 8, 1) > ws(3, 2, 8, 1)
    assert ws(32, 1, 192, 4096) <= 50 * 2 ** 20 // 4                # the full-size shape: at most a quarter of the tensor
