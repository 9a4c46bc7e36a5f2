"""Quaternion rotation ops, host side (no GPU): the reference-generated fixture against the rotation weight restated from
its formula + torch conv / conv_transpose / matmul in float64, the reference's signatures and state-dict keys, and the
requests that must raise."""
import inspect
import json

import numpy as np
import pytest
import torch

from oracle.seld_oracle import closed_form_input
from tests.golden.rotation_cases import (LAYER_CASES, all_variants, rotation_cotangent, rotation_inputs,
                                         rotation_matrix, rotation_reference64)
from tests.helpers import pkg

VARIANTS = all_variants()


def _check(got, ref, what, tol=2e-6):
    assert ref.shape == tuple(got.shape), (what, ref.shape, tuple(got.shape))
    err = np.abs(got.detach().numpy() - ref).max()
    assert err <= tol * max(np.abs(ref).max(), 1.0), (what, err)


@pytest.mark.parametrize("case,name,qformat,bias", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_fixture_matches_restatement(golden, case, name, qformat, bias):
    g = golden("rotation")
    x, ws, b = rotation_inputs(case, qformat, bias, torch.float64)
    leaves = [x] + ws + ([b] if b is not None else [])
    for t in leaves:
        t.requires_grad_(True)
    y = rotation_reference64(case, x, ws, b, qformat)
    (y * rotation_cotangent(y.shape, torch.float64)).sum().backward()
    _check(y, g[name + ".y"], "y")
    _check(x.grad, g[name + ".dx"], "dx")
    for c, w in zip("rijk", ws):
        _check(w.grad, g[f"{name}.d{c}"], "d" + c)
    if b is not None:
        _check(b.grad, g[name + ".dbias"], "dbias")
    else:
        assert name + ".dbias" not in g


def test_case_table_covers_the_issue():
    kinds = {(c["kind"], len(c["w"])) for c, *_ in VARIANTS}
    assert {("conv", 3), ("conv", 4), ("tconv", 3), ("tconv", 4), ("linear", 2)} <= kinds
    assert any(c["kind"] == "conv" and c["dilation"] > 1 and c["padding"] > 0 for c, *_ in VARIANTS)
    assert any(c["kind"] == "conv" and c["stride"] > 1 for c, *_ in VARIANTS)
    assert any(c["kind"] == "tconv" and c["output_padding"] > 0 for c, *_ in VARIANTS)
    assert {len(c["x"]) for c, *_ in VARIANTS if c["kind"] == "linear"} == {1, 2}      # 2-D and 3-D input
    assert {(q, b) for _, _, q, b in VARIANTS} == {(False, False), (False, True), (True, False), (True, True)}


def test_rotation_matrix_layout():
    """The block structure of the restatement: E at block (m, c), or (m+1, c+1) behind zero row / column 0, and the
    constant 1 on the diagonal blocks only."""
    ws = [torch.zeros(2, 3, 2, dtype=torch.float64) for _ in range(4)]
    K = rotation_matrix(ws, False)
    assert torch.equal(K, torch.eye(3, dtype=torch.float64).repeat_interleave(2, 0).repeat_interleave(3, 1)
                       [:, :, None].expand(6, 9, 2))
    Kq = rotation_matrix(ws, True)
    assert Kq.shape == (8, 12, 2)
    assert not Kq[:2].any() and not Kq[:, :3].any()
    assert torch.equal(Kq[2:, 3:], K)


REFERENCE_SIGNATURES = {
    "quaternion_conv_rotation": ["input", "r_weight", "i_weight", "j_weight", "k_weight", "bias", "stride", "padding",
                                 "groups", "dilatation", "quaternion_format"],
    "quaternion_transpose_conv_rotation": ["input", "r_weight", "i_weight", "j_weight", "k_weight", "bias", "stride",
                                           "padding", "output_padding", "groups", "dilatation", "quaternion_format"],
    "quaternion_linear_rotation": ["input", "r_weight", "i_weight", "j_weight", "k_weight", "bias",
                                   "quaternion_format"],
}


@pytest.mark.parametrize("fn", sorted(REFERENCE_SIGNATURES))
def test_functional_signatures_match_reference(fn):
    """Parameter names and order of quaternion_ops.py:174-388, so that the reference's positional calls work."""
    params = inspect.signature(getattr(pkg().quaternion.quaternion_ops, fn)).parameters
    assert list(params) == REFERENCE_SIGNATURES[fn]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params.values())
    if fn == "quaternion_linear_rotation":
        assert params["bias"].default is None and params["quaternion_format"].default is False


def _our_layer(c):
    np.random.seed(c["np_seed"])
    return getattr(pkg().quaternion.quaternion_layers, c["cls"])(**c["kwargs"])


@pytest.mark.parametrize("c", LAYER_CASES, ids=[c["name"] for c in LAYER_CASES])
def test_rotation_layers_keep_reference_state(golden, c):
    g = golden("rotation")
    m = _our_layer(c)
    sd = m.state_dict()
    assert list(sd.keys()) == json.loads(str(g["layer_keys"]))[c["name"]]
    for k, v in sd.items():
        ref = g[f"{c['name']}.{k}"]
        assert tuple(v.shape) == ref.shape, k
        # the seeded initialisation draws as the reference's
        assert np.abs(v.numpy() - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), k


@pytest.mark.parametrize("c", LAYER_CASES, ids=[c["name"] for c in LAYER_CASES])
def test_layer_fixture_matches_restatement(golden, c):
    g = golden("rotation")
    name = c["name"]
    kw = c["kwargs"]
    ws = [torch.from_numpy(g[f"{name}.{p}_weight"]).double().requires_grad_(True) for p in "rijk"]
    b = torch.from_numpy(g[name + ".bias"]).double().requires_grad_(True) if kw["bias"] else None
    x = closed_form_input(c["x"], torch.float64).requires_grad_(True)
    if c["cls"] == "QuaternionLinearAutograd":
        case = dict(kind="linear")
    elif c["cls"] == "QuaternionConv":
        case = dict(kind="conv", stride=kw["stride"], padding=kw["padding"], dilation=1)
    else:
        case = dict(kind="tconv", stride=kw["stride"], padding=kw["padding"], output_padding=kw["output_padding"],
                    dilation=1)
    y = rotation_reference64(case, x, ws, b, kw["quaternion_format"])
    (y * rotation_cotangent(y.shape, torch.float64)).sum().backward()
    _check(y, g[name + ".y"], "y")
    _check(x.grad, g[name + ".dx"], "dx")
    for p, w in zip("rijk", ws):
        _check(w.grad, g[f"{name}.grad.{p}_weight"], p)
    if b is not None:
        _check(b.grad, g[name + ".grad.bias"], "bias")


def test_requests_raise():
    P = pkg()
    L, H, Q = P._lib, P.hip_ops, P.quaternion.quaternion_ops
    Ql = P.quaternion.quaternion_layers
    ws = [torch.zeros(2, 2, 3) for _ in range(4)]
    x = torch.zeros(1, 6, 8)
    # CPU tensors: the package has no host path
    with pytest.raises(L.SeldHipError, match="HIP device"):
        Q.quaternion_conv_rotation(x, *ws, None, 1, 1, 1, 1, False)
    with pytest.raises(L.SeldHipError, match="HIP device"):
        Q.quaternion_transpose_conv_rotation(x, *ws, None, 1, 1, 0, 1, 1, False)
    with pytest.raises(L.SeldHipError, match="HIP device"):
        Q.quaternion_linear_rotation(torch.zeros(3, 6), *[torch.zeros(2, 2) for _ in range(4)])
    with pytest.raises(L.SeldHipError):
        Ql.QuaternionConv(8, 8, 3, 1, rotation=True, seed=1, operation="convolution1d")(torch.zeros(1, 6, 8))
    with pytest.raises(L.SeldHipError):
        Ql.QuaternionLinearAutograd(8, 8, rotation=True, seed=1)(torch.zeros(3, 6))
    # the validation ahead of the kernels: channel counts and bias size, as the reference's torch calls would
    with pytest.raises(L.SeldHipError, match="bias"):          # the reference layers' default: 4*O elements, 3*O needed
        H.hyper_conv_rotation(x, ws, torch.zeros(8), 1, 1, 1, False)
    with pytest.raises(L.SeldHipError, match="bias"):
        H.hyper_conv_transpose_rotation(x, ws, torch.zeros(8), 1, 1, 0, 1, False)
    with pytest.raises(L.SeldHipError, match="bias"):
        H.hyper_linear_rotation(torch.zeros(3, 6), [torch.zeros(2, 2) for _ in range(4)], torch.zeros(8), False)
    with pytest.raises(L.SeldHipError, match="channels"):      # quaternion_format wants 4*I input channels
        H.hyper_conv_rotation(x, ws, None, 1, 1, 1, True)
    with pytest.raises(L.SeldHipError, match="differ"):
        H.hyper_conv_rotation(x, ws[:3] + [torch.zeros(2, 2, 2)], None, 1, 1, 1, False)
