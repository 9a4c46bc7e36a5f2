"""Depthwise convolution and the depthwise-separable layers, host side (no GPU): the reference fixture against a float64
restatement, the layers' state-dict keys and default initialisation, and the C ABI (output extents, refused
descriptors)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden.depthwise_cases import (DEPTHWISE_CASES, PARAMS, STATS, depthwise_cotangent, depthwise_input)
from tests.helpers import pkg

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4            # include/seld_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["seld_dwconv_out_shape", "seld_dwconv_fwd", "seld_dwconv_bwd_data", "seld_dwconv_bwd_weight_workspace",
         "seld_dwconv_bwd_weight_acc", "seld_dwconv_kernel_label"]
IDS = [c["name"] for c in DEPTHWISE_CASES]


def _t(a):
    return torch.from_numpy(np.asarray(a)).double()


def restated(case, sd, x, training, running=None):
    """DepthwiseSeparableConv{1D,2D}.forward in float64 from a state dict: depthwise conv (groups = C), 1 x 1 conv,
    batch_norm, relu.  `running`: (mean, var) tensors updated in place in training mode."""
    conv = F.conv2d if case["cls"] == "2D" else F.conv1d
    _, _, _, stride, padding = case["args"]
    C = x.shape[1]
    y = conv(x, sd["depthwise.weight"], sd["depthwise.bias"], stride, padding, 1, C)
    y = conv(y, sd["pointwise.weight"], sd["pointwise.bias"])
    mean, var = running if running is not None else (sd["bn.running_mean"].clone(), sd["bn.running_var"].clone())
    y = F.batch_norm(y, mean, var, sd["bn.weight"], sd["bn.bias"], training, 0.1, 1e-5)
    return F.relu(y)


def _close(got, ref, tol, what):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= tol * max(ref.abs().max().item(), 1e-30), (what, err)


@pytest.mark.parametrize("case", DEPTHWISE_CASES, ids=IDS)
def test_fixture_agrees_with_float64_restatement(golden, case):
    g = golden("depthwise")
    name = case["name"]
    sd = {k: _t(g[f"{name}.init.{k}"]).requires_grad_(k in PARAMS) for k in PARAMS + STATS}
    x = depthwise_input(case, torch.float64).requires_grad_(True)
    mean, var = sd["bn.running_mean"].detach().clone(), sd["bn.running_var"].detach().clone()
    y = restated(case, sd, x, True, (mean, var))
    (y * depthwise_cotangent(y.shape, torch.float64)).sum().backward()
    _close(y, g[name + ".y"], 1e-6, "y")
    _close(x.grad, g[name + ".dx"], 1e-6, "dx")
    for k in PARAMS:
        _close(sd[k].grad, g[f"{name}.grad.{k}"], 1e-6, k)
    _close(mean, g[name + ".train.bn.running_mean"], 1e-6, "running_mean")
    _close(var, g[name + ".train.bn.running_var"], 1e-6, "running_var")
    assert int(g[name + ".train.bn.num_batches_tracked"]) == 1
    with torch.no_grad():
        ye = restated(case, dict(sd, **{"bn.running_mean": mean, "bn.running_var": var}), x, False)
    _close(ye, g[name + ".y_eval"], 1e-6, "y_eval")


@pytest.mark.parametrize("case", DEPTHWISE_CASES, ids=IDS)
def test_layer_keys_and_initialisation_match_reference(golden, case):
    g = golden("depthwise")
    DL = pkg().dual_quaternion.dual_quaternion_layers
    torch.manual_seed(case["seed"])
    layer = getattr(DL, "DepthwiseSeparableConv" + case["cls"])(*case["args"])
    sd = layer.state_dict()
    assert list(sd.keys()) == json.loads(str(g["layer_keys"]))[case["name"]]
    for k, v in sd.items():
        ref = g[f"{case['name']}.init.{k}"]
        assert tuple(v.shape) == ref.shape, k
        assert np.array_equal(v.numpy().astype(np.float32), ref), k
    M = pkg().model
    assert M.DepthwiseSeparableConv2D is DL.DepthwiseSeparableConv2D
    assert M.DepthwiseSeparableConv1D is DL.DepthwiseSeparableConv1D


def test_header_declares_and_library_exports_entry_points():
    with open(os.path.join(ROOT, "include", "seld_hip.h")) as f:
        header = f.read()
    lib = pkg()._lib.lib()
    for name in NAMES:
        assert f"{name}(" in header, name
        assert hasattr(lib, name), name


def _out(desc):
    out = (ctypes.c_int32 * 2)()
    rc = pkg()._lib.lib().seld_dwconv_out_shape(ctypes.byref(desc), out)
    return rc, tuple(out)


@pytest.mark.parametrize("x,cout,k,s,p,d", [
    ((2, 8, 9, 11), 8, 3, 1, 1, 1),
    ((1, 3, 10, 7), 6, (2, 5), (2, 1), (0, 2), (1, 2)),
    ((2, 4, 6, 5), 12, (3, 1), 3, (2, 0), 2),
    ((1, 5, 4, 4), 5, 4, 1, 0, 1),
    ((2, 6, 19), 6, 5, 2, 2, 1),
    ((1, 4, 7), 8, 2, 3, 1, 3),
])
def test_out_shape_matches_pytorch(x, cout, k, s, p, d):
    H = pkg().hip_ops
    desc = H.make_dwconv_desc(x, cout, k, s, p, d)
    rc, o = _out(desc)
    C = x[1]
    conv = F.conv2d if len(x) == 4 else F.conv1d
    kk = (k,) * (len(x) - 2) if isinstance(k, int) else k
    ref = conv(torch.zeros(x), torch.zeros((cout, 1) + tuple(kk)), None, s, p, d, C).shape[2:]
    assert rc == 0
    assert (o if len(x) == 4 else (o[1],)) == tuple(ref)


def test_refused_descriptors_without_gpu():
    """Host-side argument checking: every entry point refuses before it touches the device."""
    L, H = pkg()._lib, pkg().hip_ops
    lib = L.lib()

    def calls(desc):
        buf = ctypes.create_string_buffer(64)
        return [lib.seld_dwconv_out_shape(ctypes.byref(desc), (ctypes.c_int32 * 2)()),
                lib.seld_dwconv_fwd(ctypes.byref(desc), None, None, None, None, None),
                lib.seld_dwconv_bwd_data(ctypes.byref(desc), None, None, None, None),
                lib.seld_dwconv_bwd_weight_acc(ctypes.byref(desc), None, None, None, None, None, 0, None),
                lib.seld_dwconv_kernel_label(ctypes.byref(desc), 0, buf, 64)]

    ok = H.make_dwconv_desc((2, 8, 16, 16), 16, 3, 1, 1, 1)
    assert lib.seld_dwconv_bwd_weight_workspace(ctypes.byref(ok)) > 0
    bad = []
    d = H.make_dwconv_desc((2, 8, 16, 16), 16, 3, 1, 1, 1)
    d.groups = 4                                                   # groups != Cin
    bad.append((d, EINVAL))
    d = H.make_dwconv_desc((2, 8, 16, 16), 12, 3, 1, 1, 1)         # Cout not a multiple of Cin
    bad.append((d, EINVAL))
    d = H.make_dwconv_desc((2, 8, 16, 16), 32, 3, 1, 1, 1)
    d.algebra = 4                                                  # not real-valued
    bad.append((d, EINVAL))
    bad.append((H.make_dwconv_desc((2, 8, 16, 16), 8, 3, 0, 1, 1), EINVAL))       # stride 0
    bad.append((H.make_dwconv_desc((0, 8, 16, 16), 8, 3, 1, 1, 1), EINVAL))       # no batch
    bad.append((H.make_dwconv_desc((2, 8, 2, 16), 8, 5, 1, 0, 1), EINVAL))        # empty output
    bad.append((H.make_dwconv_desc((2, 8, 32, 32), 8, 16, 1, 0, 1), EUNSUPPORTED))  # kh * kw = 256
    bad.append((H.make_dwconv_desc((1, 64, 2048, 2048), 64, 1, 1, 0, 1), EUNSUPPORTED))  # image >= 2^28
    for desc, want in bad:
        assert set(calls(desc)) == {want}, (want, calls(desc))
        assert lib.seld_dwconv_bwd_weight_workspace(ctypes.byref(desc)) == 0
    # a valid descriptor: missing buffers, then too small a workspace (checked before any launch)
    assert lib.seld_dwconv_fwd(ctypes.byref(ok), None, None, None, None, None) == EINVAL
    assert lib.seld_dwconv_bwd_data(ctypes.byref(ok), None, None, None, None) == EINVAL
    p = ctypes.c_void_p(16)
    assert lib.seld_dwconv_bwd_weight_acc(ctypes.byref(ok), p, p, p, None, None, 0, None) == EWORKSPACE
    # the hypercomplex convolution entry points still refuse groups != 1
    assert lib.seld_hc_conv_fwd(ctypes.byref(ok), None, None, None, None, None) == EUNSUPPORTED


def test_kernel_labels():
    H = pkg().hip_ops
    d = H.make_dwconv_desc((32, 64, 128, 512), 64, 3, 1, 1, 1)
    assert H.dwconv_label(d, 0).startswith("dwconv_fwd_kernel<")
    assert H.dwconv_label(d, 1).startswith("dwconv_dgrad_kernel<")
    assert H.dwconv_label(d, 2).startswith("dwconv_wgrad_kernel<")
    d = H.make_dwconv_desc((2, 8, 32, 32), 8, 3, 2, 1, 1)
    assert ", true, " in H.dwconv_label(d, 1)               # stride 2: the phase form of the input gradient


def test_conv_modules_refuse_other_groups_without_gpu():
    L, hnn = pkg()._lib, pkg().hip_nn
    with pytest.raises(L.SeldHipError):
        hnn.Conv2d(8, 8, 3, groups=2)(torch.zeros(1, 8, 6, 6))
    with pytest.raises(L.SeldHipError):
        hnn.Conv1d(8, 8, 3, groups=8, padding="same")(torch.zeros(1, 8, 6))
