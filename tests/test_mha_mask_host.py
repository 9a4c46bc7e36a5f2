"""Masked / cross-length attention without a GPU: the fixture (tests/golden/mha_mask.npz, made by the reference's
MultiHeadAttention) against a float64 restatement of its formula, and the C ABI's workspace query and refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle.seld_oracle import closed_form_fill_
from tests.golden.mha_mask_cases import (MHA_MASK_CASES, mha_core_reference, mha_mask, mha_mask_cotangent,
                                         mha_mask_inputs)
from tests.helpers import pkg

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4            # include/seld_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restated_module(c, v, k, q, mask):
    """MultiHeadAttention.forward (model.py:25-51) in float64 with the closed-form weights, separate v, k, q."""
    E = c["E"]
    ws = [("values.weight", torch.empty(E, E, 1, dtype=torch.float64)),
          ("keys.weight", torch.empty(E, E, 1, dtype=torch.float64)),
          ("queries.weight", torch.empty(E, E, 1, dtype=torch.float64)),
          ("fc_out.weight", torch.empty(E, E, dtype=torch.float64)),
          ("fc_out.bias", torch.empty(E, dtype=torch.float64))]
    closed_form_fill_(ws, amp=0.6)
    p = {n: t.requires_grad_(True) for n, t in ws}

    def proj(x, w):                      # (N, T, E) -> (N, E, T) through the 1x1 convolution
        return torch.einsum("oi,nti->not", w[..., 0], x)
    out = mha_core_reference(proj(q, p["queries.weight"]), proj(k, p["keys.weight"]), proj(v, p["values.weight"]),
                             c["heads"], mask)
    y = out.transpose(1, 2) @ p["fc_out.weight"].t() + p["fc_out.bias"]
    return y, p


@pytest.mark.parametrize("case", MHA_MASK_CASES, ids=[c["name"] for c in MHA_MASK_CASES])
def test_fixture_agrees_with_float64_restatement(golden, case):
    g = golden("mha_mask")
    n = case["name"]
    v, k, q = (t.requires_grad_(True) for t in mha_mask_inputs(case, torch.float64))
    y, p = _restated_module(case, v, k, q, mha_mask(case))
    (y * mha_mask_cotangent(y.shape, torch.float64)).sum().backward()
    pairs = [("y", y), ("dv", v.grad), ("dk", k.grad), ("dq", q.grad), ("dwv", p["values.weight"].grad),
             ("dwk", p["keys.weight"].grad), ("dwq", p["queries.weight"].grad), ("dwo", p["fc_out.weight"].grad),
             ("dbo", p["fc_out.bias"].grad)]
    for what, t in pairs:
        ref = g[f"{n}.{what}"].astype(np.float64)
        got = t.detach().numpy()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        assert np.abs(got - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-6), what
        assert np.isfinite(ref).all(), what


def test_fixture_covers_the_numerical_corners():
    """The float-mask case has a fully masked query row and a fully masked (sample, head): there the reference attends
    uniformly to every key, so that row's attention output is the mean of the projected values."""
    c = next(c for c in MHA_MASK_CASES if c["mask"] == "float_full")
    m = mha_mask(c)
    assert (m[0, 1, 4] == 0).all() and (m[1, 2] == 0).all() and ((m != 0) & (m != 1)).any()
    q = torch.randn(1, c["E"], 5, dtype=torch.float64)
    kv = torch.randn(1, c["E"], 7, dtype=torch.float64)
    out = mha_core_reference(q, kv, kv, c["heads"], torch.zeros(5, 7))
    assert torch.allclose(out, kv.mean(2, keepdim=True).expand_as(out))


def test_header_declares_and_library_exports_entry_points():
    with open(os.path.join(ROOT, "include", "seld_hip.h")) as f:
        hdr = f.read()
    lib = pkg()._lib.lib()
    for name in ("seld_mha_fwd_ex", "seld_mha_bwd_ex_workspace", "seld_mha_bwd_ex"):
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name


def test_workspace_query():
    lib = pkg()._lib.lib()
    assert lib.seld_mha_bwd_ex_workspace(3, 40, 8) == 3 * 8 * 40 * 4
    assert lib.seld_mha_bwd_ex_workspace(0, 40, 8) == 0
    assert lib.seld_mha_bwd_ex_workspace(3, -1, 8) == 0


def test_refused_descriptors_without_gpu():
    """Every refusal returns before any launch, so these run on a machine without a GPU.  The pointers are never
    dereferenced: the descriptor checks come first."""
    lib = pkg()._lib.lib()
    P = ctypes.c_void_p(0x1000)          # stands in for a device pointer; never read
    ok = (ctypes.c_int64 * 4)(0, 0, 0, 1)
    neg = (ctypes.c_int64 * 4)(0, 0, -1, 1)

    def fwd(q=P, N=2, Tq=16, Tk=16, H=2, hd=16, keep=None, strides=None, out=P):
        return lib.seld_mha_fwd_ex(q, P, P, N, Tq, Tk, H, hd, keep, strides, out, P, None)

    def bwd(hd=16, keep=None, strides=None, ws=None, nbytes=0, Tk=16):
        return lib.seld_mha_bwd_ex(P, P, P, P, P, P, 2, 16, Tk, 2, hd, keep, strides, P, P, P, ws, nbytes, None)
    assert fwd(q=None) == EINVAL
    assert fwd(out=None) == EINVAL
    assert fwd(N=0) == EINVAL
    assert fwd(Tq=0) == EINVAL
    assert fwd(Tk=-3) == EINVAL
    assert fwd(hd=0) == EINVAL
    assert fwd(keep=P, strides=None) == EINVAL        # a mask needs its strides
    assert fwd(keep=P, strides=neg) == EINVAL
    assert fwd(hd=65) == EUNSUPPORTED
    assert fwd(hd=65, keep=P, strides=ok) == EUNSUPPORTED
    assert bwd(hd=65) == EUNSUPPORTED
    assert bwd(keep=P, strides=neg) == EINVAL
    assert bwd(ws=None, nbytes=1 << 20) == EWORKSPACE
    assert bwd(ws=P, nbytes=2 * 2 * 16 * 4 - 1) == EWORKSPACE
    assert bwd(Tk=0, ws=P, nbytes=1 << 20) == EINVAL
