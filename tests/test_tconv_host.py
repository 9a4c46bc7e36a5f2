"""Quaternion transposed convolution, host side (no GPU): the fixture against the oracle's Hamilton matrix +
F.conv_transposeNd in float64, the layer's parameter layout, and the requests that must raise."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.seld_oracle import assemble_conv_weight
from tests.golden.tconv_cases import LAYER_CASE, TCONV_CASES, tconv_cotangent, tconv_inputs
from tests.helpers import pkg


def _tconv64(x, ws, bias, case):
    fn = F.conv_transpose1d if x.dim() == 3 else F.conv_transpose2d
    return fn(x, assemble_conv_weight(ws), bias, case["stride"], case["padding"], case["output_padding"], 1,
              case["dilation"])


@pytest.mark.parametrize("case", TCONV_CASES, ids=[c["name"] for c in TCONV_CASES])
def test_fixture_matches_oracle(golden, case):
    g = golden("tconv")
    name = case["name"]
    x, ws, bias = tconv_inputs(case, torch.float64)
    x.requires_grad_(True)
    for w in ws:
        w.requires_grad_(True)
    if bias is not None:
        bias.requires_grad_(True)
    y = _tconv64(x, ws, bias, case)
    (y * tconv_cotangent(y.shape, torch.float64)).sum().backward()
    pairs = [("y", y.detach()), ("du", x.grad)] + [(f"dw{i}", w.grad) for i, w in enumerate(ws)]
    if bias is not None:
        pairs.append(("dbias", bias.grad))
    else:
        assert name + ".dbias" not in g
    for key, got in pairs:
        ref = g[f"{name}.{key}"]
        assert ref.shape == tuple(got.shape), key
        err = np.abs(got.numpy() - ref).max()
        assert err <= 2e-6 * max(np.abs(ref).max(), 1.0), (key, err)


def test_case_table_covers_the_issue():
    strides = {c["stride"] if isinstance(c["stride"], int) else tuple(c["stride"]) for c in TCONV_CASES}
    assert {1, 2, 3, (2, 1)} <= strides
    assert any(len(c["x"]) == 3 for c in TCONV_CASES) and any(len(c["x"]) == 4 for c in TCONV_CASES)
    ks = {c["k"] for c in TCONV_CASES}
    assert {(1, 1), (2, 2), (3,), (4,), (3, 1)} <= ks
    # output_padding >= stride (allowed because dilation > stride)
    assert any(c["stride"] == 1 and c["output_padding"] >= 1 and c["dilation"] > 1 for c in TCONV_CASES)


def test_layer_parameters_match_reference_layout(golden):
    g = golden("tconv")
    Q = pkg().quaternion.quaternion_layers
    c = LAYER_CASE
    np.random.seed(c["np_seed"])
    m = Q.QuaternionTransposeConv(c["in_channels"], c["out_channels"], c["kernel_size"], c["stride"],
                                  dilatation=c["dilatation"], padding=c["padding"], output_padding=c["output_padding"],
                                  seed=c["seed"])
    sd = m.state_dict()
    assert list(sd.keys()) == json.loads(str(g["layer_keys"]))
    for k, v in sd.items():
        ref = g["layer." + k]
        assert tuple(v.shape) == ref.shape, k
        # the seeded initialisation draws as the reference's
        assert np.abs(v.numpy() - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), k
    assert tuple(m.r_weight.shape) == (c["in_channels"] // 4, c["out_channels"] // 4, 3, 3)


def test_requests_without_a_kernel_raise():
    P = pkg()
    L = P._lib
    Q = P.quaternion.quaternion_layers
    x = torch.zeros(1, 8, 4, 4)
    m = Q.QuaternionTransposeConv(8, 8, 3, 2, rotation=True, seed=1)
    with pytest.raises(L.SeldHipError):
        m(x)
    m = Q.QuaternionTransposeConv(8, 8, 3, 2, groups=2, seed=1)
    with pytest.raises(L.SeldHipError):
        m(x)
    ws = [torch.zeros(2, 2, 3, 3, 3) for _ in range(4)]
    with pytest.raises(L.SeldHipError):
        P.quaternion.quaternion_ops.quaternion_transpose_conv(torch.zeros(1, 8, 4, 4, 4), *ws, None, 2, 0, 0, 1, 1)
    with pytest.raises(L.SeldHipError):
        P.quaternion.quaternion_ops.quaternion_transpose_conv_rotation(x)
