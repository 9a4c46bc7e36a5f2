"""Masked and cross-length attention on the GPU (seld_mha_fwd_ex / seld_mha_bwd_ex, hip_ops.mha_core_ex,
MultiHeadAttention.forward with a mask): the module against the reference's fixture, the core against a float64 host
restatement on both dispatch sides (fp32-MFMA: hd in {16, 32, 48, 64} with Tq, Tk % 16 == 0; VALU otherwise)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import seld_oracle as O
from tests.golden.mha_mask_cases import (MHA_MASK_CASES, mha_core_reference, mha_mask, mha_mask_cotangent,
                                         mha_mask_inputs)
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(got, ref, rel, what=""):
    got = got.detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("case", MHA_MASK_CASES, ids=[c["name"] for c in MHA_MASK_CASES])
def test_module_matches_fixture(case, golden):
    g = golden("mha_mask")
    M = pkg().model
    n = case["name"]
    mha = M.MultiHeadAttention(case["E"], case["heads"])
    O.closed_form_fill_(list(mha.state_dict().items()), amp=0.6)
    mha = mha.to(DEV)
    v, k, q = (t.to(DEV).requires_grad_(True) for t in mha_mask_inputs(case))
    mask = mha_mask(case)
    y = mha(v, k, q, None if mask is None else mask.to(DEV))
    (y * mha_mask_cotangent(y.shape).to(DEV)).sum().backward()
    _close(y, g[n + ".y"], 2e-4, "y")
    for what, t in (("dv", v.grad), ("dk", k.grad), ("dq", q.grad), ("dwv", mha.values.weight.grad[..., 0]),
                    ("dwk", mha.keys.weight.grad[..., 0]), ("dwq", mha.queries.weight.grad[..., 0]),
                    ("dwo", mha.fc_out.weight.grad), ("dbo", mha.fc_out.bias.grad)):
        ref = g[f"{n}.{what}"]
        _close(t.reshape(ref.shape), ref, 5e-4, what)


def _sweep_mask(kind, N, H, Tq, Tk, gen):
    if kind is None:
        return None
    if kind == "key_padding":
        m = torch.ones(N, 1, 1, Tk, dtype=torch.bool)
        m[-1, ..., max(1, Tk - 9):] = False
        return m
    if kind == "causal":
        return torch.tril(torch.ones(Tq, Tk, dtype=torch.bool), diagonal=Tk - Tq)
    # random per (sample, head), with a fully masked row and a row whose only kept key is the last one
    m = torch.rand(N, H, Tq, Tk, generator=gen) > 0.3
    m[0, 0, 0] = False
    m[0, -1, Tq - 1] = False
    m[0, -1, Tq - 1, Tk - 1] = True
    return m


SWEEP = [  # (N, H, hd, Tq, Tk, mask)
    (2, 3, 2, 33, 33, "random"), (2, 4, 6, 20, 45, "key_padding"), (1, 2, 6, 70, 70, "causal"),
    (2, 2, 16, 32, 32, "random"), (2, 2, 16, 48, 80, "key_padding"), (1, 2, 16, 40, 24, "random"),
    (2, 8, 48, 256, 256, "random"), (1, 2, 48, 64, 160, "causal"), (1, 2, 48, 50, 130, "random"),
    (1, 4, 64, 128, 128, "random"), (1, 2, 64, 144, 96, "key_padding"), (1, 2, 64, 33, 17, "causal"),
    (1, 2, 48, 96, 96, None), (1, 2, 6, 37, 70, None), (1, 2, 32, 80, 144, "random"),
]


@pytest.mark.parametrize("N,H_,hd,Tq,Tk,kind", SWEEP)
def test_core_vs_float64(N, H_, hd, Tq, Tk, kind):
    """Both dispatch sides against the float64 host reference; a key far above the rest in a later tile forces the
    online-softmax rescale (guide rule 26), fully masked rows must give the mean of v and zero dq."""
    Hm = pkg().hip_ops
    gen = torch.Generator().manual_seed(N * 1000 + hd * 10 + Tq + Tk)
    E = H_ * hd
    q, k, v = torch.randn(N, E, Tq, generator=gen), torch.randn(N, E, Tk, generator=gen), torch.randn(N, E, Tk, generator=gen)
    k[:, :, min(Tk - 1, Tk // 2 + 7)] *= 6.0
    mask = _sweep_mask(kind, N, H_, Tq, Tk, gen)
    cot = torch.randn(N, E, Tq, generator=gen)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    out = Hm.mha_core_ex(qd, kd, vd, H_, None if mask is None else mask.to(DEV))
    (out * cot.to(DEV)).sum().backward()
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    o = mha_core_reference(q64, k64, v64, H_, mask)
    (o * cot.double()).sum().backward()
    _close(out, o, 2e-4, "out")
    _close(qd.grad, q64.grad, 5e-4, "dq")
    _close(kd.grad, k64.grad, 5e-4, "dk")
    _close(vd.grad, v64.grad, 5e-4, "dv")
    if kind == "random":
        mean_v = v[0].view(H_, hd, Tk)[0].mean(1)
        _close(out[0].view(H_, hd, Tq)[0, :, 0], mean_v, 1e-5, "fully masked row")
        assert float(qd.grad[0].view(H_, hd, Tq)[0, :, 0].abs().max()) == 0.0


@pytest.mark.parametrize("hd,T", [(16, 64), (48, 256), (64, 96)])
def test_mfma_matches_valu_on_masked_inputs(hd, T, seld_env):
    Hm = pkg().hip_ops
    gen = torch.Generator().manual_seed(hd + T)
    N, H_ = 2, 2
    q, k, v = (torch.randn(N, H_ * hd, T, generator=gen).to(DEV) for _ in range(3))
    mask = _sweep_mask("random", N, H_, T, T, gen).to(DEV)
    cot = torch.randn(N, H_ * hd, T, generator=gen).to(DEV)

    def run():
        ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = Hm.mha_core_ex(*ts, H_, mask)
        out.backward(cot)
        return [out.detach()] + [t.grad for t in ts]
    seld_env.unset("SELD_MHA_NO_MFMA")
    a = run()
    seld_env.set("SELD_MHA_NO_MFMA", "1")
    b = run()
    for what, x, y in zip(("out", "dq", "dk", "dv"), a, b):
        _close(x, y, 2e-5, what)


@pytest.mark.parametrize("hd,T", [(6, 40), (48, 256)])
def test_all_ones_mask_matches_unmasked_path(hd, T):
    Hm = pkg().hip_ops
    gen = torch.Generator().manual_seed(7)
    N, H_ = 2, 4
    q, k, v = (torch.randn(N, H_ * hd, T, generator=gen).to(DEV) for _ in range(3))
    cot = torch.randn(N, H_ * hd, T, generator=gen).to(DEV)
    res = []
    for masked in (False, True):
        ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = Hm.mha_core_ex(*ts, H_, torch.ones(T, T, device=DEV)) if masked else Hm.mha_core(*ts, H_)
        out.backward(cot)
        res.append([out.detach()] + [t.grad for t in ts])
    for what, x, y in zip(("out", "dq", "dk", "dv"), *res):
        _close(x, y, 1e-6, what)


def test_full_clip_key_padding():
    """Batched full-clip inference (T = 2400, hd = 48): clip 1 is 1500 frames padded to 2400 and masked by a key-padding
    mask.  Its first 1500 outputs equal the clip run alone, and no energy tensor is ever materialised."""
    Hm = pkg().hip_ops
    gen = torch.Generator().manual_seed(11)
    N, H_, hd, T, Ts = 2, 8, 48, 2400, 1500
    E = H_ * hd
    q, k, v = (torch.randn(N, E, T, generator=gen).to(DEV) for _ in range(3))
    mask = torch.ones(N, 1, 1, T, dtype=torch.bool)
    mask[1, ..., Ts:] = False
    mask = mask.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = Hm.mha_core_ex(*ts, H_, mask)
    cot = torch.ones_like(out)
    cot[1, :, Ts:] = 0.0             # the padded queries' outputs are not used
    out.backward(cot)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    energy = N * H_ * T * T * 4
    assert peak < energy / 4, (peak, energy)
    alone = [t[1:2, :, :Ts].clone().requires_grad_(True) for t in (q, k, v)]
    oa = Hm.mha_core_ex(*alone, H_)
    oa.backward(torch.ones_like(oa))
    _close(out[1:2, :, :Ts], oa, 1e-5, "short clip out")
    _close(ts[1].grad[1:2, :, :Ts], alone[1].grad, 1e-5, "short clip dk")
    _close(ts[2].grad[1:2, :, :Ts], alone[2].grad, 1e-5, "short clip dv")
    assert float(ts[2].grad[1, :, Ts:].abs().max()) == 0.0       # padded keys receive nothing


@pytest.mark.parametrize("hd,T", [(6, 50), (48, 128)])
def test_bitwise_repeatable(hd, T):
    Hm = pkg().hip_ops
    gen = torch.Generator().manual_seed(3)
    N, H_ = 2, 4
    q, k, v = (torch.randn(N, H_ * hd, T, generator=gen).to(DEV) for _ in range(3))
    mask = _sweep_mask("random", N, H_, T, T, gen).to(DEV)
    cot = torch.randn(N, H_ * hd, T, generator=gen).to(DEV)
    runs = []
    for _ in range(2):
        ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = Hm.mha_core_ex(*ts, H_, mask)
        out.backward(cot)
        runs.append([out.detach()] + [t.grad for t in ts])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_graph_capture_and_replay():
    """A masked forward + backward (float mask: the `mask != 0` conversion included) captured in a graph and replayed
    on new inputs equals the eager result: nothing on the path synchronises with the host."""
    Hm = pkg().hip_ops
    gen = torch.Generator().manual_seed(9)
    N, H_, hd, Tq, Tk = 2, 2, 48, 64, 96
    E = H_ * hd
    q = torch.randn(N, E, Tq, generator=gen).to(DEV).requires_grad_(True)
    k = torch.randn(N, E, Tk, generator=gen).to(DEV).requires_grad_(True)
    v = torch.randn(N, E, Tk, generator=gen).to(DEV).requires_grad_(True)
    mask = (torch.rand(N, 1, Tq, Tk, generator=gen) > 0.4).float().to(DEV)
    cot = torch.randn(N, E, Tq, generator=gen).to(DEV)

    def step():
        out = Hm.mha_core_ex(q, k, v, H_, mask)
        return (out,) + torch.autograd.grad(out, (q, k, v), cot)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    with torch.no_grad():
        for t in (q, k, v):
            t.mul_(0.5).add_(0.1)
        mask.copy_((torch.rand(N, 1, Tq, Tk, generator=gen) > 0.6).float())
    g.replay()
    torch.cuda.synchronize()
    eager = step()
    for what, x, y in zip(("out", "dq", "dk", "dv"), static, eager):
        assert torch.equal(x, y), what


def test_refusals_write_nothing():
    Hm, L = pkg().hip_ops, pkg()._lib
    M = pkg().model
    mha = M.MultiHeadAttention(16, 2).to(DEV)
    x = torch.randn(2, 12, 16, device=DEV)
    with pytest.raises(L.SeldHipError, match="value_len"):
        mha(x[:, :10], x, x)
    with pytest.raises(L.SeldHipError, match="broadcast"):
        mha(x, x, x, torch.ones(3, 12, 12, device=DEV))             # a 3-D mask's first dim lines up with the 2 heads
    with pytest.raises(L.SeldHipError, match="broadcast"):
        mha(x, x, x, torch.ones(3, 1, 12, 12, device=DEV))
    with pytest.raises(L.SeldHipError, match="broadcast"):
        mha(x, x, x, torch.ones(4, 1, 1, 1, 12, device=DEV))        # would enlarge the energy shape
    with pytest.raises(L.SeldHipError):
        mha(x, x, x, torch.ones(12, 12))                             # mask on the CPU
    with pytest.raises(L.SeldHipError, match="64"):
        Hm.mha_core_ex(*(torch.randn(1, 65, 16, device=DEV) for _ in range(3)), 1)
    # the C ABI: a refused call leaves its outputs untouched
    lib = L.lib()
    q = torch.randn(1, 130, 16, device=DEV)
    out = torch.full_like(q, float("nan"))
    lse = torch.full((1, 2, 16), 7.0, device=DEV)
    neg = (ctypes.c_int64 * 4)(0, 0, -1, 1)
    keep = torch.ones(16, 16, dtype=torch.uint8, device=DEV)
    assert lib.seld_mha_fwd_ex(L.ptr(q), L.ptr(q), L.ptr(q), 1, 16, 16, 2, 65, None, None, L.ptr(out), L.ptr(lse),
                               L.current_stream()) == -4
    assert lib.seld_mha_fwd_ex(L.ptr(q), L.ptr(q), L.ptr(q), 1, 16, 16, 2, 16, L.ptr(keep), neg, L.ptr(out), L.ptr(lse),
                               L.current_stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (lse == 7.0).all()
