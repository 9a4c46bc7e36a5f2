"""3-D convolution and transposed convolution, host side (no GPU): the C ABI and the built library, output extents,
refused descriptors, the reference fixture against a float64 restatement, the case table, and the seeded layers'
parameters."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.seld_oracle import assemble_conv_weight, hypercomplex_conv
from tests.golden.conv3d_cases import (CONV3D_CASES, LAYER3D_CASES, ROT3D_CASES, conv3d_cotangent, conv3d_inputs,
                                       rot3d_inputs, rot3d_variants)
from tests.golden.rotation_cases import rotation_matrix
from tests.helpers import pkg

EINVAL, EUNSUPPORTED = -1, -4            # include/seld_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["out_shape", "fwd", "bwd_data", "bwd_weight_workspace", "bwd_weight_acc", "kernel_label"]
NAMES = [f"seld_hc_conv3d_{e}" for e in ENTRY] + [f"seld_hc_conv3d_transpose_{e}" for e in ENTRY]


def test_header_declares_and_library_exports_entry_points():
    with open(os.path.join(ROOT, "include", "seld_hip.h")) as f:
        header = f.read()
    assert "typedef struct seld_conv3d_desc" in header
    lib = pkg()._lib.lib()
    for name in NAMES:
        assert f"{name}(" in header, name
        assert hasattr(lib, name), name


def _out(desc, out_pad=None):
    L = pkg()._lib
    out = (ctypes.c_int32 * 3)()
    if out_pad is None:
        rc = L.lib().seld_hc_conv3d_out_shape(ctypes.byref(desc), out)
    else:
        rc = L.lib().seld_hc_conv3d_transpose_out_shape(ctypes.byref(desc), out_pad, out)
    return rc, tuple(out)


@pytest.mark.parametrize("x,k,s,p,d", [
    ((2, 8, 5, 6, 7), 3, 1, 1, 1),
    ((1, 8, 9, 10, 11), (1, 3, 5), (1, 2, 3), (0, 1, 2), 1),
    ((1, 16, 7, 8, 9), (3, 2, 3), 2, (2, 0, 1), (2, 1, 3)),
    ((3, 4, 16, 5, 4), (4, 1, 2), (3, 1, 2), 0, 1),
])
def test_out_shape_matches_pytorch(x, k, s, p, d):
    H = pkg().hip_ops
    desc = H.make_conv3d_desc(x, 8, 4, k, s, p, d)
    rc, o = _out(desc)
    w = torch.zeros((8, x[1]) + tuple(desc.k))
    assert rc == 0 and o == tuple(F.conv3d(torch.zeros(x), w, None, s, p, d).shape[2:])
    for op in [(0, 0, 0), tuple(max(0, min(a, b) - 1) for a, b in zip(desc.stride, desc.dil))]:
        desc_t, opa = H.conv3d_transpose_desc(x, 8, 4, k, s, p, op, d)
        rc, o = _out(desc_t, opa)
        wt = torch.zeros((x[1], 8) + tuple(desc.k))
        assert rc == 0 and o == tuple(F.conv_transpose3d(torch.zeros(x), wt, None, s, p, op, 1, d).shape[2:])


def test_refused_descriptors_without_gpu():
    """Host-side argument checking: every entry point refuses before it touches the device."""
    L = pkg()._lib
    H = pkg().hip_ops
    lib = L.lib()
    three = (ctypes.c_int32 * 3)

    def calls(desc, op):
        rcs = [lib.seld_hc_conv3d_fwd(ctypes.byref(desc), None, None, None, None, None),
               lib.seld_hc_conv3d_bwd_data(ctypes.byref(desc), None, None, None, None),
               lib.seld_hc_conv3d_bwd_weight_acc(ctypes.byref(desc), None, None, None, None, None, 0, None),
               lib.seld_hc_conv3d_transpose_fwd(ctypes.byref(desc), op, None, None, None, None, None),
               lib.seld_hc_conv3d_transpose_bwd_data(ctypes.byref(desc), op, None, None, None, None),
               lib.seld_hc_conv3d_transpose_bwd_weight_acc(ctypes.byref(desc), op, None, None, None, None, None, 0, None)]
        assert lib.seld_hc_conv3d_bwd_weight_workspace(ctypes.byref(desc)) == 0 or rcs[2] == 0
        return rcs

    ok = H.make_conv3d_desc((1, 8, 4, 4, 4), 8, 4, 3, 1, 1, 1)
    assert lib.seld_hc_conv3d_bwd_weight_workspace(ctypes.byref(ok)) > 0
    # channels not a multiple of the algebra
    bad = H.make_conv3d_desc((1, 6, 4, 4, 4), 8, 4, 3, 1, 1, 1)
    assert set(calls(bad, three(0, 0, 0))) == {EINVAL}
    # stride beyond the phase tables
    bad = H.make_conv3d_desc((1, 8, 40, 4, 4), 8, 4, 1, (17, 1, 1), 0, 1)
    assert set(calls(bad, three(0, 0, 0))) == {EUNSUPPORTED}
    # groups
    bad = H.make_conv3d_desc((1, 8, 4, 4, 4), 8, 4, 3, 1, 1, 1, groups=2)
    assert set(calls(bad, three(0, 0, 0))) == {EUNSUPPORTED}
    # kernel larger than the padded input (convolution only)
    bad = H.make_conv3d_desc((1, 8, 2, 4, 4), 8, 4, (5, 1, 1), 1, 0, 1)
    assert lib.seld_hc_conv3d_fwd(ctypes.byref(bad), None, None, None, None, None) == EINVAL
    # output_padding >= stride and >= dilation (transposed only)
    desc, _ = H.conv3d_transpose_desc((1, 8, 4, 4, 4), 8, 4, 3, 2, 1, 0, 1)
    assert lib.seld_hc_conv3d_transpose_fwd(ctypes.byref(desc), three(0, 2, 0), None, None, None, None, None) == EINVAL
    assert lib.seld_hc_conv3d_transpose_out_shape(ctypes.byref(desc), three(0, 2, 0), three()) == EINVAL
    # dual quaternion: no transposed form in the reference
    desc, op = H.conv3d_transpose_desc((1, 8, 4, 4, 4), 8, 8, 3, 2, 1, 0, 1)
    assert lib.seld_hc_conv3d_transpose_fwd(ctypes.byref(desc), op, None, None, None, None, None) == EUNSUPPORTED
    # an input image beyond 32-bit addressing
    bad = H.make_conv3d_desc((1, 64, 256, 256, 64), 64, 4, 1, 1, 0, 1)
    assert lib.seld_hc_conv3d_fwd(ctypes.byref(bad), None, None, None, None, None) == EUNSUPPORTED
    # a valid descriptor without buffers
    assert lib.seld_hc_conv3d_fwd(ctypes.byref(ok), None, None, None, None, None) == EINVAL
    assert lib.seld_hc_conv3d_bwd_weight_acc(ctypes.byref(ok), None, None, None, None, None, 0, None) == EINVAL


def test_kernel_labels():
    H = pkg().hip_ops
    d = H.make_conv3d_desc((2, 64, 8, 16, 16), 64, 4, 3, 1, 1, 1)
    assert H.conv3d_label(d, None, 0).startswith("hc_conv3d_fwd_kernel<")
    assert H.conv3d_label(d, None, 1).startswith("hc_conv3d_phase_kernel<")
    assert H.conv3d_label(d, None, 2) == "hc_conv3d_wgrad_kernel"
    d, op = H.conv3d_transpose_desc((2, 64, 8, 16, 16), 64, 4, 4, 2, 1, 0, 1)
    assert H.conv3d_label(d, op, 0).startswith("hc_conv3d_phase_kernel<")
    assert H.conv3d_label(d, op, 1).startswith("hc_conv3d_fwd_kernel<")
    assert H.conv3d_label(d, op, 2) == "hc_conv3d_wgrad_kernel"


def conv3d_reference64(case, x, ws, bias):
    if case["kind"] == "tconv":
        return F.conv_transpose3d(x, assemble_conv_weight(ws), bias, case["stride"], case["padding"],
                                  case["output_padding"], 1, case["dilation"])
    return hypercomplex_conv(x, ws, bias, case["stride"], case["padding"], 1, case["dilation"])


def rot3d_reference64(case, x, ws, bias, qformat):
    K = rotation_matrix(ws, qformat)
    if case["kind"] == "conv":
        return F.conv3d(x, K, bias, case["stride"], case["padding"], case["dilation"])
    return F.conv_transpose3d(x, K, bias, case["stride"], case["padding"], case["output_padding"], 1, case["dilation"])


def _check(g, name, y, x, named):
    (y * conv3d_cotangent(y.shape, torch.float64)).sum().backward()
    for key, got in [("y", y.detach()), ("dx", x.grad)] + [(k, t.grad) for k, t in named]:
        ref = g[f"{name}.{key}"]
        assert ref.shape == tuple(got.shape), key
        err = np.abs(got.numpy() - ref).max()
        assert err <= 2e-6 * max(np.abs(ref).max(), 1.0), (key, err)


@pytest.mark.parametrize("case", CONV3D_CASES, ids=[c["name"] for c in CONV3D_CASES])
def test_fixture_matches_oracle(golden, case):
    g = golden("conv3d")
    x, ws, bias = conv3d_inputs(case, torch.float64)
    for t in [x] + ws + ([bias] if bias is not None else []):
        t.requires_grad_(True)
    named = [(f"dw{i}", w) for i, w in enumerate(ws)] + ([("dbias", bias)] if bias is not None else [])
    if bias is None:
        assert case["name"] + ".dbias" not in g
    _check(g, case["name"], conv3d_reference64(case, x, ws, bias), x, named)


@pytest.mark.parametrize("case,name,qformat", rot3d_variants(), ids=[v[1] for v in rot3d_variants()])
def test_rotation_fixture_matches_oracle(golden, case, name, qformat):
    g = golden("conv3d")
    x, ws, bias = rot3d_inputs(case, qformat, torch.float64)
    for t in [x] + ws + [bias]:
        t.requires_grad_(True)
    named = [(f"d{c}", w) for c, w in zip("rijk", ws)] + [("dbias", bias)]
    _check(g, name, rot3d_reference64(case, x, ws, bias, qformat), x, named)


def _tup(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3


def test_case_table_covers_the_issue():
    conv = [c for c in CONV3D_CASES if c["kind"] == "conv"]
    for A in (4, 8):
        ks = {tuple(c["k"]) for c in conv if c["algebra"] == A}
        assert (3, 3, 3) in ks and any(len(set(k)) > 1 for k in ks), A        # cubic 'same' and anisotropic kernels
        assert any(tuple(c["k"]) == (3, 3, 3) and c["padding"] == 1 and c["stride"] == 1 for c in conv
                   if c["algebra"] == A)
    assert {(1, 3, 3), (3, 1, 3)} <= {tuple(c["k"]) for c in conv}
    assert any(1 < max(_tup(c["stride"])) and min(_tup(c["stride"])) == 1 for c in conv)      # stride on some axes
    assert any(sorted(_tup(c["dilation"]))[-2:] == [1, 2] for c in conv)                     # dilation on one axis
    assert any(any(e % 2 for e in c["x"][2:]) for c in CONV3D_CASES)                          # odd extents
    assert {True, False} == {c["bias"] for c in conv}
    tconv = [c for c in CONV3D_CASES if c["kind"] == "tconv"]
    assert any(sum(1 for e in _tup(c["output_padding"]) if e) == 1 for c in tconv)         # output_padding on one axis
    assert {c["kind"] for c in ROT3D_CASES} == {"conv", "tconv"}
    assert {q for _, _, q in rot3d_variants()} == {False, True}
    assert {"QuaternionConv", "DualQuaternionConv", "QuaternionTransposeConv"} <= {c["cls"] for c in LAYER3D_CASES}
    assert any(c["kwargs"].get("rotation") for c in LAYER3D_CASES)
    assert all(c["kwargs"]["operation"] == "convolution3d" for c in LAYER3D_CASES)


def _seeded_layer(c):
    P = pkg()
    mod = P.dual_quaternion.dual_quaternion_layers if c["cls"].startswith("Dual") else P.quaternion.quaternion_layers
    np.random.seed(c["np_seed"])
    return getattr(mod, c["cls"])(**c["kwargs"])


@pytest.mark.parametrize("c", LAYER3D_CASES, ids=[c["name"] for c in LAYER3D_CASES])
def test_seeded_layers_reproduce_reference_state_dicts(golden, c):
    g = golden("conv3d")
    sd = _seeded_layer(c).state_dict()
    assert list(sd.keys()) == json.loads(str(g["layer_keys"]))[c["name"]]
    for k, v in sd.items():
        ref = g[f"{c['name']}.{k}"]
        assert tuple(v.shape) == ref.shape, k
        assert np.abs(v.numpy() - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), k


def test_cpu_input_raises():
    P = pkg()
    L = P._lib
    Q = P.quaternion.quaternion_layers
    m = Q.QuaternionConv(8, 8, 3, 1, padding=1, seed=1, operation='convolution3d')
    with pytest.raises(L.SeldHipError, match="HIP device tensor"):
        m(torch.zeros(1, 8, 4, 4, 4))
