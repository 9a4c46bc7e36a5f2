"""Temporal attention on the device (csrc/temporal_attention.hip): the core against the fp64 formulas of tests/at_ref.py on
both dispatch sides, against the independent kernels of hip_ops.mha_core_ex, bit repeatability, guard floats, the error
codes and host refusals, hip_nn.TemporalAttention against fp64 and with an optimiser's gradient slots, the identity at
initialisation, the model against fp64 and the training paths of train.main.

Tolerances are the project's own for fp32 attention against fp64 (tests/test_gpu_mha_mask.py::_close: the largest error
relative to the reference's largest entry, 2e-4 forward and 5e-4 backward; 2e-5 between two fp32 implementations) and for
the model (tests/test_gpu_squeeze_excite.py::test_model_with_se_matches_fp64)."""
import functools

import numpy as np
import pytest
import torch

from tests import at_ref as R
from tests.golden.cases import MODEL_CASES, model_kwargs, train_target
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1234.5
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
CASE = {c["name"]: c for c in MODEL_CASES}
NUMBERED = [pytest.param(i + 1, c, id=f"{i + 1}-{R.case_id(c)}") for i, c in enumerate(R.CASES)]


# ======================================================================================================================
# plumbing
# ======================================================================================================================
def _close(got, ref, rel, what=""):
    got = got.detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    print(f"AT {what}: max err {err:.3e}, scale {scale:.3e}, ratio to the bound {err / (rel * scale):.3f}")
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _out(n, fill=float("nan")):
    """An output buffer of n elements holding `fill`, with sentinel elements around it: (view, whole buffer)."""
    buf = torch.full((n + 16,), SENTINEL)
    buf[8:8 + n] = fill
    buf = buf.to(DEV)
    return buf[8:8 + n], buf


def _guards_intact(buf, n):
    want = _bits(torch.full((8,), SENTINEL))
    return torch.equal(_bits(buf[:8]), want) and torch.equal(_bits(buf[8 + n:]), want)


def _untouched(buf, n):
    return bool(buf[8:8 + n].isnan().all()) and _guards_intact(buf, n)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """fp32 (qkv, dread) of a case on the host (made once, never modified)."""
    return tuple(t.float() for t in R.make_case(case))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """fp64 (read, lse, dqkv) of the fp32 inputs of a case (made once, never modified)."""
    N, K, V, T, mask, W, lengths = case
    qkv, dread = (t.double() for t in _inputs(case))
    f = R.at_forward(qkv, K, V, mask, W, lengths)
    return f["read"], f["lse"], R.at_backward(qkv, dread, K, V, f["p"], f["read"])


def _lengths(case):
    return None if case[6] is None else torch.tensor(case[6], dtype=torch.int32, device=DEV)


def _run(case):
    """hip_ops.at_core forward + backward of a case: (read, lse, dqkv) on the device."""
    H = pkg().hip_ops
    N, K, V, T, mask, W, lengths = case
    qkv, dread = (t.to(DEV) for t in _inputs(case))
    qkv.requires_grad_(True)
    read, lse = H.at_core(qkv, K, V, mask, W, _lengths(case), return_lse=True)
    read.backward(dread)
    torch.cuda.synchronize()
    return read.detach(), lse, qkv.grad


def _labels(case):
    H = pkg().hip_ops
    return [H.at_kernel_label(op, case[3], case[1], case[2]) for op in ("fwd", "bwd_dq", "bwd_dkv")]


# ======================================================================================================================
# the core
# ======================================================================================================================
@pytest.mark.parametrize("number, case", NUMBERED)
def test_core_matches_fp64(number, case):
    """read, lse and dqkv of every case against at_ref; rows with no allowed key are exactly 0 in read and in dq and have
    lse = +inf; excluded positions get exactly nothing (dk, dv behind a sample's length are 0)."""
    N, K, V, T, mask, W, lengths = case
    read, lse, dqkv = _run(case)
    rread, rlse, rdqkv = _reference(case)
    _close(read, rread, 2e-4, f"case {number} read")
    _close(dqkv[:, :K], rdqkv[:, :K], 5e-4, f"case {number} dq")
    _close(dqkv[:, K:2 * K], rdqkv[:, K:2 * K], 5e-4, f"case {number} dk")
    _close(dqkv[:, 2 * K:], rdqkv[:, 2 * K:], 5e-4, f"case {number} dv")
    dead = torch.isinf(rlse)
    assert torch.equal(torch.isinf(lse.cpu()) & (lse.cpu() > 0), dead)
    live_scale = max(float(rlse[~dead].abs().max()), 1e-6)
    assert float((lse.cpu().double()[~dead] - rlse[~dead]).abs().max()) <= 2e-4 * live_scale
    if dead.any():
        sel = dead.unsqueeze(1)
        assert float(read.cpu().masked_select(sel.expand(N, V, T)).abs().max()) == 0.0
        assert float(dqkv[:, :K].cpu().masked_select(sel.expand(N, K, T)).abs().max()) == 0.0
    if lengths is not None:
        for n, ln in enumerate(lengths):
            if ln < T:
                assert float(dqkv[n, K:, ln:].abs().max()) == 0.0


@pytest.mark.parametrize("number, case", NUMBERED)
def test_dispatch_and_mfma_matches_valu(number, case, seld_env):
    """The library names an MFMA form for the cases whose widths are multiples of 16 with T % 16 == 0 and a VALU form for
    the rest; under SELD_MHA_NO_MFMA=1 VALU for all.  Where both exist their results agree to 2e-5."""
    seld_env.unset("SELD_MHA_NO_MFMA")
    want = "mfma" if number in R.MFMA_CASES else "valu"
    labels = _labels(case)
    assert [l.split("_kernel")[0] for l in labels] == [f"at_fwd_{want}", f"at_bwd_dq_{want}", f"at_bwd_dkv_{want}"], labels
    if want == "mfma":
        assert all(l.endswith(f"<{case[1]},{case[2]}>") for l in labels), labels
        a = _run(case)
    seld_env.set("SELD_MHA_NO_MFMA", "1")
    labels = _labels(case)
    assert all("_valu_kernel<" in l for l in labels), labels
    if want == "mfma":
        b = _run(case)
        K = case[1]
        live = ~torch.isinf(a[1])
        assert torch.equal(torch.isinf(a[1]), torch.isinf(b[1]))
        for what, x, y in (("read", a[0], b[0]), ("lse", a[1][live], b[1][live]), ("dq", a[2][:, :K], b[2][:, :K]),
                           ("dk", a[2][:, K:2 * K], b[2][:, K:2 * K]), ("dv", a[2][:, 2 * K:], b[2][:, 2 * K:])):
            _close(x, y, 2e-5, f"case {number} mfma vs valu {what}")


@pytest.mark.parametrize("number, v_cut", [(3, None), (11, None), (7, 16)])
def test_core_matches_the_byte_mask_attention(number, v_cut):
    """Cases 3 and 11, and case 7 with V cut to 16, against hip_ops.mha_core_ex (separate q, k, v, one head, the causal or
    no mask as a bool tensor): read and the three gradients to 2e-5.  No row is fully masked, so the two conventions of
    an excluded key coincide."""
    H = pkg().hip_ops
    N, K, V, T, mask, W, lengths = R.CASES[number - 1]
    qkv, dread = _inputs(R.CASES[number - 1])
    if v_cut is not None:
        qkv, dread, V = qkv[:, :2 * K + v_cut].contiguous(), dread[:, :v_cut].contiguous(), v_cut
    assert K == V and lengths is None and mask in ("causal", "none")
    qkv, dread = qkv.to(DEV), dread.to(DEV)
    leaf = qkv.clone().requires_grad_(True)
    read = H.at_core(leaf, K, V, mask, W)
    read.backward(dread)
    q, k, v = (qkv[:, i * K:(i + 1) * K].contiguous().requires_grad_(True) for i in range(3))
    keep = None if mask == "none" else torch.tril(torch.ones(T, T, dtype=torch.bool, device=DEV))
    out = H.mha_core_ex(q, k, v, 1, keep)
    out.backward(dread)
    torch.cuda.synchronize()
    _close(read, out, 2e-5, f"case {number} read")
    for i, (what, t) in enumerate((("dq", q), ("dk", k), ("dv", v))):
        _close(leaf.grad[:, i * K:(i + 1) * K], t.grad, 2e-5, f"case {number} {what}")


@pytest.mark.parametrize("number", [8, 10])
def test_bitwise_repeatable(number):
    a, b = _run(R.CASES[number - 1]), _run(R.CASES[number - 1])
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("number", [2, 9])
def test_guard_floats_stay_intact(number):
    """The C ABI on NaN-filled outputs with sentinel floats around them: every element of read, lse and dqkv is written and
    nothing beside them; the results equal hip_ops.at_core's."""
    L = pkg()._lib
    lib, st, p = L.lib(), L.current_stream(), L.ptr
    case = R.CASES[number - 1]
    N, K, V, T, mask, W, lengths = case
    kind = pkg().hip_ops.AT_MASKS[mask]
    qkv, dread = (t.to(DEV) for t in _inputs(case))
    ln = _lengths(case)
    read, rbuf = _out(N * V * T)
    lse, lbuf = _out(N * T)
    dqkv, dbuf = _out(N * (2 * K + V) * T)
    nbytes = lib.seld_at_bwd_workspace(N, T)
    assert nbytes == 4 * N * T
    ws, wbuf = _out(N * T)
    L.check(lib.seld_at_fwd(p(qkv), N, T, K, V, kind, W, p(ln), p(read), p(lse), st), "seld_at_fwd")
    L.check(lib.seld_at_bwd(p(qkv), p(read), p(dread), p(lse), N, T, K, V, kind, W, p(ln), p(dqkv), p(ws), nbytes, st),
            "seld_at_bwd")
    torch.cuda.synchronize()
    for name, t, buf in (("read", read, rbuf), ("lse", lse, lbuf), ("dqkv", dqkv, dbuf), ("workspace", ws, wbuf)):
        assert _guards_intact(buf, t.numel()), name
        assert not bool(t.isnan().any()), f"{name}: elements left unwritten"
    want = _run(case)
    assert torch.equal(_bits(read), _bits(want[0].reshape(-1))) and torch.equal(_bits(lse), _bits(want[1].reshape(-1)))
    assert torch.equal(_bits(dqkv), _bits(want[2].reshape(-1)))


@pytest.mark.parametrize("shift", [1, 3])
def test_tensors_off_a_16_byte_boundary_take_the_valu_form(shift):
    """Case 3 (MFMA widths) through the C ABI with qkv, dread, read and dqkv `shift` floats behind a 16-byte boundary: the
    MFMA kernels' 16-byte loads do not apply, the entry points fall back to the VALU form, and the results agree with the
    aligned run to the 2e-5 of two fp32 implementations; guards intact."""
    L = pkg()._lib
    lib, st, p = L.lib(), L.current_stream(), L.ptr
    case = R.CASES[2]
    N, K, V, T, mask, W, _ = case
    kind = pkg().hip_ops.AT_MASKS[mask]

    def shifted(t, fill=None):
        buf = torch.full((t.numel() + 16,), SENTINEL, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[4 + shift:4 + shift + t.numel()]
        v.copy_(t.reshape(-1)) if fill is None else v.fill_(fill)
        return v, buf
    qkv, dread = _inputs(case)
    (qd, _), (gd, _) = shifted(qkv.to(DEV)), shifted(dread.to(DEV))
    (read, rbuf), (dqkv, dbuf) = shifted(torch.empty(N * V * T), float("nan")), shifted(torch.empty(qkv.numel()), float("nan"))
    lse, ws = torch.empty(N * T, device=DEV), torch.empty(N * T, device=DEV)
    L.check(lib.seld_at_fwd(p(qd), N, T, K, V, kind, W, None, p(read), p(lse), st), "seld_at_fwd")
    L.check(lib.seld_at_bwd(p(qd), p(read), p(gd), p(lse), N, T, K, V, kind, W, None, p(dqkv), p(ws), 4 * N * T, st), "seld_at_bwd")
    torch.cuda.synchronize()
    want = _run(case)
    _close(read, want[0].reshape(-1), 2e-5, f"shift {shift} read")
    _close(dqkv, want[2].reshape(-1), 2e-5, f"shift {shift} dqkv")
    sent = _bits(torch.full((1,), SENTINEL))[0]
    for buf, n in ((rbuf, read.numel()), (dbuf, dqkv.numel())):
        guards = torch.cat((_bits(buf[:4 + shift]), _bits(buf[4 + shift + n:])))
        assert bool((guards == sent).all())


def test_element_offsets_past_2_to_the_31():
    """N = 2, K = V = 1, T = 360 M: qkv and dqkv hold 2.16 G floats each (8.6 GB), so sample 1's v and dv rows lie past
    element 2^31.  q = k = 0 makes every score 0 and p uniform over the +-1 band, so no host reference is needed and the
    test stays quick: read[t] is the mean of v over the band (3 keys, 2 at the two ends), with v a small-integer pattern
    that differs between the samples; with dread = 1, dv[s] = sum over the queries in the band of 1 / count(t): 1 inside,
    1/2 + 1/3 at the ends; dq and dk are exactly 0."""
    H = pkg().hip_ops
    N, T = 2, 360_000_000
    assert N * 3 * T > 2 ** 31
    qkv = torch.zeros((N, 3, T), device=DEV)
    pat = (torch.arange(T, device=DEV) % 5).float()
    qkv[0, 2] = pat
    qkv[1, 2] = pat + 100.0
    del pat
    qkv.requires_grad_(True)
    read, lse = H.at_core(qkv, 1, 1, "band", 1, return_lse=True)
    v = qkv.detach()[:, 2]
    want = v.clone()
    want[:, 1:] += v[:, :-1]
    want[:, :-1] += v[:, 1:]
    want /= 3.0
    want[:, 0] = (v[:, 0] + v[:, 1]) / 2.0
    want[:, -1] = (v[:, -1] + v[:, -2]) / 2.0
    err = (read.detach()[:, 0] - want).abs_()
    # exact sums and counts; fl(o * fl(1 / 3)) against fl(o / 3): at most 2 ulp of the value (at most 4 and 104)
    assert float(err[0].max()) <= 2 * 2.0 ** -23 * 4 and float(err[1].max()) <= 2 * 2.0 ** -23 * 104, \
        (float(err[0].max()), float(err[1].max()))
    del want, err
    assert float(lse[:, 1:-1].min()) == float(lse[:, 1:-1].max()) and abs(float(lse[0, 1]) - np.log(3.0)) < 1e-6
    assert abs(float(lse[1, -1]) - np.log(2.0)) < 1e-6
    read.backward(torch.ones_like(read))
    g = qkv.grad
    assert float(g[:, :2].abs().max()) == 0.0
    dv = g[:, 2]
    assert float((dv[:, 2:-2] - 1.0).abs().max()) <= 1e-6
    for n in range(N):
        for at, val in ((0, 1 / 2 + 1 / 3), (1, 1 / 2 + 2 / 3), (T - 2, 1 / 2 + 2 / 3), (T - 1, 1 / 2 + 1 / 3)):
            assert abs(float(dv[n, at]) - val) <= 1e-6, (n, at, float(dv[n, at]))


def test_lengths_are_clamped_into_1_T():
    """lengths of 0, -3 and T + 9 act as 1, 1 and T."""
    H = pkg().hip_ops
    case = (3, 8, 12, 40, "none", 0, None)
    qkv = _inputs(case)[0].to(DEV)
    got = H.at_core(qkv, 8, 12, "none", 0, torch.tensor([0, -3, 49], dtype=torch.int32, device=DEV))
    want = H.at_core(qkv, 8, 12, "none", 0, torch.tensor([1, 1, 40], dtype=torch.int32, device=DEV))
    assert torch.equal(got, want)
    assert torch.equal(got[2], H.at_core(qkv, 8, 12, "none")[2])
    _close(got[0], qkv[0, 16:, :1].expand(12, 40), 1e-6, "length 1 reads v[:, 0]")


def test_graph_capture_and_replay():
    """Forward + backward with lengths captured in a graph and replayed on new inputs equal the eager result: nothing on
    the path synchronises with the host."""
    H = pkg().hip_ops
    case = R.CASES[7]
    N, K, V, T, mask, W, _ = case
    qkv, dread = (t.to(DEV) for t in _inputs(case))
    qkv.requires_grad_(True)
    ln = _lengths(case)

    def step():
        read = H.at_core(qkv, K, V, mask, W, ln)
        return (read,) + torch.autograd.grad(read, (qkv,), dread)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    with torch.no_grad():
        qkv.mul_(0.5).add_(0.1)
        ln.copy_(torch.tensor([100, 128, 3], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    eager = step()
    for what, x, y in zip(("read", "dqkv"), static, eager):
        assert torch.equal(x, y), what


# ======================================================================================================================
# error codes and refusals
# ======================================================================================================================
def test_refused_calls_write_nothing():
    """SELD_EUNSUPPORTED (a width above 64), SELD_EINVAL (NULL tensor, a size <= 0, band < 0, an unknown kind) and
    SELD_EWORKSPACE leave NaN-filled outputs and their guards as they were: nothing was launched."""
    L = pkg()._lib
    lib, st, p = L.lib(), L.current_stream(), L.ptr
    N, K, V, T = 1, 16, 16, 32
    qkv = torch.randn(N, 2 * 65 + 65, T, device=DEV)
    dread = torch.randn(N, 65, T, device=DEV)
    read, rbuf = _out(N * 65 * T)
    lse, lbuf = _out(N * T)
    dqkv, dbuf = _out(N * 3 * 65 * T)
    ws, wbuf = _out(N * T)
    nb = 4 * N * T
    fwd = lambda *a, qkv_=qkv, read_=read, lse_=lse: lib.seld_at_fwd(p(qkv_), *a, None, p(read_), p(lse_), st)
    bwd = lambda *a, ws_=ws, nb_=nb: lib.seld_at_bwd(p(qkv), p(read), p(dread), p(lse), *a, None, p(dqkv), p(ws_), nb_, st)
    assert fwd(N, T, 65, V, 1, 0) == EUNSUPPORTED and fwd(N, T, K, 65, 1, 0) == EUNSUPPORTED
    assert bwd(N, T, 65, V, 1, 0) == EUNSUPPORTED and bwd(N, T, K, 65, 0, 0) == EUNSUPPORTED
    for bad in ((0, T, K, V, 1, 0), (N, 0, K, V, 1, 0), (N, T, 0, V, 1, 0), (N, T, K, -1, 1, 0), (N, T, K, V, 2, -1),
                (N, T, K, V, 1, -5), (N, T, K, V, 3, 0), (N, T, K, V, -1, 0)):
        assert fwd(*bad) == EINVAL, bad
        assert bwd(*bad) == EINVAL, bad
    assert fwd(N, T, K, V, 1, 0, qkv_=None) == EINVAL and fwd(N, T, K, V, 1, 0, read_=None) == EINVAL
    assert fwd(N, T, K, V, 1, 0, lse_=None) == EINVAL
    assert bwd(N, T, K, V, 1, 0, ws_=None) == EWORKSPACE and bwd(N, T, K, V, 1, 0, nb_=nb - 1) == EWORKSPACE
    assert lib.seld_at_bwd_workspace(0, T) == 0 and lib.seld_at_bwd_workspace(N, -1) == 0
    torch.cuda.synchronize()
    for name, t, buf in (("read", read, rbuf), ("lse", lse, lbuf), ("dqkv", dqkv, dbuf), ("workspace", ws, wbuf)):
        assert _untouched(buf, t.numel()), name
    H = pkg().hip_ops
    with pytest.raises(L.SeldHipError):
        H.at_kernel_label("fwd", 32, 65, 16)
    with pytest.raises(L.SeldHipError):
        H.at_kernel_label("fwd", 0, 16, 16)


def test_host_refusals():
    L, H = pkg()._lib, pkg().hip_ops
    qkv = _inputs(R.CASES[1])[0].to(DEV)          # (2, 11, 37): K 3, V 5
    assert H.at_core(qkv, 3, 5).shape == (2, 5, 37)
    with pytest.raises(L.SeldHipError, match="device tensor"):
        H.at_core(qkv.cpu(), 3, 5)
    with pytest.raises(L.SeldHipError, match="float32"):
        H.at_core(qkv.double(), 3, 5)
    with pytest.raises(L.SeldHipError, match="contiguous"):
        H.at_core(qkv.transpose(0, 1).contiguous().transpose(0, 1), 3, 5)
    with pytest.raises(L.SeldHipError, match="qkv must be"):
        H.at_core(qkv, 3, 4)
    with pytest.raises(L.SeldHipError, match="qkv must be"):
        H.at_core(qkv[0], 3, 5)
    with pytest.raises(L.SeldHipError, match="not supported"):
        H.at_core(torch.zeros(1, 2 * 65 + 1, 4, device=DEV), 65, 1)
    with pytest.raises(L.SeldHipError, match="key_size"):
        H.at_core(qkv, 0, 11)
    with pytest.raises(L.SeldHipError, match="mask"):
        H.at_core(qkv, 3, 5, mask="future")
    with pytest.raises(L.SeldHipError, match="band"):
        H.at_core(qkv, 3, 5, mask="band", band=-1)
    for bad in (torch.tensor([37, 5]), torch.tensor([37, 5], device=DEV), torch.tensor([37, 5, 1], dtype=torch.int32, device=DEV),
                [37, 5]):
        with pytest.raises(L.SeldHipError, match="lengths"):
            H.at_core(qkv, 3, 5, lengths=bad)


# ======================================================================================================================
# the module
# ======================================================================================================================
def _module(C, K, V, mask, band, seed):
    m = pkg().hip_nn.TemporalAttention(C, K, V, mask, band)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "weight" in name else 0.2))
    return m.to(DEV)


@pytest.mark.parametrize("shape, K, V, mask, band", [((2, 24, 50), 6, 10, "band", 4), ((2, 32, 64), 16, 32, "causal", 0)])
def test_module_matches_fp64(shape, K, V, mask, band):
    """hip_nn.TemporalAttention forward and backward with random non-zero `out` weights against at_module_apply in fp64:
    2e-4 on the output, 5e-4 on every gradient."""
    m = _module(shape[1], K, V, mask, band, 5)
    g = torch.Generator().manual_seed(6)
    x, dy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    y.backward(dy.to(DEV))
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    ref = R.at_module_apply({"at." + k: v for k, v in sd.items()}, "at", x64, mask, band)
    ref.backward(dy.double())
    _close(y, ref, 2e-4, "module y")
    _close(xd.grad, x64.grad, 5e-4, "module dx")
    for k, p in m.named_parameters():
        _close(p.grad, sd[k].grad, 5e-4, "module d" + k)


def test_module_gradients_land_in_flat_adam_slots():
    """Parameters owned by a FlatAdam: after backward the flat buffer holds the gradients of a stand-alone copy of the
    module, the slots around them are untouched, and every parameter's .grad is a view of its slot."""
    T = pkg().train
    shape, K, V = (2, 24, 50), 6, 10
    free, owned = _module(24, K, V, "band", 4, 5), _module(24, K, V, "band", 4, 5)
    g = torch.Generator().manual_seed(6)
    x, dy = torch.randn(shape, generator=g).to(DEV), torch.randn(shape, generator=g).to(DEV)
    free(x).backward(dy)
    front, back = (torch.nn.Parameter(torch.full((5,), 2.0, device=DEV)) for _ in range(2))
    opt = T.FlatAdam([front] + list(owned.parameters()) + [back], lr=1e-3)
    opt.zero_grad()
    owned(x).backward(dy)
    opt.step()          # flushes deferred weight gradients; the gradients stay in the flat buffer
    torch.cuda.synchronize()
    for (k, p), q in zip(free.named_parameters(), owned.parameters()):
        assert float(p.grad.abs().max()) > 0, k
        _close(q.grad, p.grad, 1e-6, "slot d" + k)
    n_at = sum(p.numel() for p in owned.parameters())
    zeros = torch.zeros(5, device=DEV)
    assert torch.equal(opt.flat_grad[:5], zeros) and torch.equal(opt.flat_grad[5 + n_at:5 + n_at + 5], zeros)
    assert all(p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * off for p, off in zip(opt.params, opt.offsets))


# ======================================================================================================================
# the model
# ======================================================================================================================
def _tiny(name, **kw):
    np.random.seed(1)
    torch.manual_seed(1)
    return pkg().model.SELD_Model(**dict(model_kwargs(CASE[name]), **kw))


def _model_inputs(name):
    from oracle import seld_oracle as O
    case = CASE[name]
    x = O.closed_form_input((case["B"], case["input_channels"], case["freq_dim"], case["time_dim"]))
    return x, train_target(case)


def _step(m, x, target, train):
    """Outputs and (in training mode) every parameter's gradient after one forward + loss + backward."""
    T = pkg().train
    m = m.to(DEV).train(train)
    if not train:
        with torch.no_grad():
            sed, doa = m(x.to(DEV))
        return sed, doa, {}
    opt = T.FlatAdam(m.parameters(), lr=1e-4)
    opt.zero_grad()
    sed, doa = m(x.to(DEV))
    T.seld_loss_fn(sed, doa, target.to(DEV), 42, 1.0, 5.0).backward()
    opt.step()          # flushes deferred weight gradients; the gradients stay in the flat buffer
    torch.cuda.synchronize()
    return sed.detach(), doa.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_fresh_block_leaves_the_model_unchanged(train, seld_env):
    """tiny DQ model (one stack), dropout 0, SELD_DETERMINISTIC=1: at_key_size=8 with its own fresh AT parameters (out
    zero) on top of the AT-off model's state dict gives the same outputs and the same gradient of every non-AT parameter,
    bit for bit; the gradient of out.weight is not zero: the block can grow in."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    H = pkg().hip_ops
    x, target = _model_inputs("tiny_DQ")
    off, on = _tiny("tiny_DQ"), _tiny("tiny_DQ", at_key_size=8)
    sd = {k: v.clone() for k, v in off.state_dict().items()}
    fresh = {k: v.clone() for k, v in on.state_dict().items() if k not in sd}
    assert sorted(fresh) == sorted(f"seld_block.tcn.at.0.{m}.{p}" for m in ("qkv", "out") for p in ("weight", "bias"))
    assert all(float(fresh[k].abs().max()) == 0.0 for k in fresh if ".out." in k)
    on.load_state_dict(dict(sd, **fresh))
    res = []
    for m in (off, on):
        H.philox.set_offset(0)
        H.hcq_weights.reset()
        res.append(_step(m, x, target, train))
    (sed0, doa0, g0), (sed1, doa1, g1) = res
    assert torch.equal(sed0, sed1) and torch.equal(doa0, doa1)
    assert len(g1) == len(g0) + 4 * train
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    if train:
        assert float(g1["seld_block.tcn.at.0.out.weight"].abs().max()) > 0.0
        assert float(g1["seld_block.tcn.at.0.out.bias"].abs().max()) > 0.0


@pytest.mark.parametrize("name, at", [("tiny_Q", dict(at_key_size=8, at_value_size=12, at_mask="band", at_band=5)),
                                      ("tiny_DQ", dict(at_key_size=8, at_value_size=12, at_mask="band", at_band=5)),
                                      ("tiny_R", dict(at_key_size=8, at_value_size=12, at_mask="band", at_band=5)),
                                      ("tiny_DQ", dict(at_key_size=16, at_value_size=16, at_mask="causal"))],
                         ids=["tiny_Q-band", "tiny_DQ-band", "tiny_R-band", "tiny_DQ-causal16"])
def test_model_with_at_matches_fp64(name, at, seld_env):
    """Forward and one backward of the tiny models (the closed-form weights of the model fixtures, random AT weights with
    a non-zero `out`) against the same walk in fp64 on the CPU: the oracle's layers with tests/at_ref.py's block in front
    of the stack.  The project's tolerance: 1e-3 on the SED and DOA outputs; every gradient to 1e-3 of its largest entry
    with the floor of tests/test_gpu_squeeze_excite.py::test_model_with_se_matches_fp64 (a gradient below 1e-4 of the
    largest RMS over the parameters is fp32 cancellation noise in either stack, so the scale is never below 10 floors)."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    from oracle import seld_oracle as O
    H = pkg().hip_ops
    case = CASE[name]
    x, target = _model_inputs(name)
    m = _tiny(name, **at)
    O.closed_form_fill_([(k, v) for k, v in m.state_dict().items() if ".at." not in k])
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".at." in k:
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "weight" in k else 0.2))
    sd64 = {k: v.detach().double().clone() for k, v in m.state_dict().items()}
    for v in sd64.values():
        v.requires_grad_(v.is_floating_point())
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    sed, doa, grads = _step(m, x, target, True)
    cfg = O.SeldConfig(**model_kwargs(case))
    rsed, rdoa = R.seld_forward_at(sd64, cfg, x.double(), True, at["at_mask"], at.get("at_band", 0))
    O.seld_loss(rsed, rdoa, target.double(), 42).backward()
    err = max(float((sed.cpu().double() - rsed.detach()).abs().max()), float((doa.cpu().double() - rdoa.detach()).abs().max()))
    print("AT model", name, at, "max |out - fp64|", err)
    assert err <= 1e-3
    rms = [float(v.grad.pow(2).mean().sqrt()) for v in sd64.values() if v.grad is not None]
    floor = 1e-4 * max(rms)
    worst, worst_at = 0.0, ""
    for k, gr in grads.items():
        ref = sd64[k].grad
        if ref is None:
            assert float(gr.abs().max()) == 0.0, k
            continue
        rel = float((gr.cpu().double() - ref).abs().max()) / max(float(ref.abs().max()), 10 * floor)
        if rel > worst:
            worst, worst_at = rel, k
        assert rel <= 1e-3, (k, rel)
    at_keys = [k for k in grads if ".at." in k]
    assert len(at_keys) == 4 and all(float(sd64[k].grad.abs().max()) > 0 for k in at_keys)
    print("AT model", name, "worst gradient error / largest entry", worst, worst_at)


# ======================================================================================================================
# training paths
# ======================================================================================================================
_runs = {}


def _train(mode, tmp_path_factory):
    """train.main with --at_key_size=8, 2 epochs on write_pickles data: each mode run once and shared."""
    from tests import test_gpu_train_loader as TL
    if "paths" not in _runs:
        _runs["paths"] = TL.write_pickles(tmp_path_factory.mktemp("at_pickles"), 5)
    if mode not in _runs:
        extra = {"off": {}, "resident": dict(resident_loader="True"),
                 "graph": dict(resident_loader="True", graph_step="True")}[mode]
        _runs[mode] = TL._main(_runs["paths"], str(tmp_path_factory.mktemp("at_" + mode)), 2, at_key_size=8, **extra)
    return _runs[mode]


def test_resident_loader_run_equals_the_eager_run_with_at_on(seld_env, tmp_path_factory):
    """train.main --at_key_size=8 under SELD_DETERMINISTIC=1: the --resident_loader run equals the flags-off run bit for
    bit (parameters, BatchNorm buffers, Adam moments, both losses of both epochs); the checkpoint holds the 4 AT tensors
    and each has a non-zero first moment: the slots reached Adam and the block grew in from zero."""
    from tests import test_gpu_train_loader as TL
    seld_env.set("SELD_DETERMINISTIC", "1")
    (h_off, ck_off, _), (h_res, ck_res, _) = _train("off", tmp_path_factory), _train("resident", tmp_path_factory)
    a, b = TL._tensors(ck_off), TL._tensors(ck_res)
    assert a.keys() == b.keys()
    at = [k for k in ck_off["model_state_dict"] if ".at." in k]
    assert len(at) == 4
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert h_res == h_off and len(h_off) == 2, (h_res, h_off)
    params = [k for k in ck_off["model_state_dict"] if "running_" not in k and "num_batches" not in k]
    state = ck_off["optimizer_state_dict"]["state"]
    moved = [k for i, k in enumerate(params) if ".at." in k and float(state[i]["exp_avg"].abs().max()) > 0]
    assert len(moved) == 4, moved
    assert float(ck_off["model_state_dict"]["seld_block.tcn.at.0.out.weight"].abs().max()) > 0.0


def test_graph_step_run_matches_the_eager_run_with_at_on(seld_env, tmp_path_factory):
    """The --graph_step run against the flags-off run at the tolerance of tests/test_gpu_train_loader.py: the AT launches
    record and replay."""
    from tests import test_gpu_train_loader as TL
    seld_env.set("SELD_DETERMINISTIC", "1")
    (h_off, ck_off, _), (h_g, ck_g, _) = _train("off", tmp_path_factory), _train("graph", tmp_path_factory)
    a, c = TL._tensors(ck_off), TL._tensors(ck_g)
    assert a.keys() == c.keys()
    TL._compare_graph_to_eager(a, c)
    assert np.allclose([t for _, t, _ in h_g], [t for _, t, _ in h_off], rtol=1e-6, atol=0), (h_g, h_off)
    assert np.allclose([v for _, _, v in h_g], [v for _, _, v in h_off], rtol=1e-6, atol=0), (h_g, h_off)


def test_checkpoint_with_at_round_trips(seld_env, tmp_path_factory, tmp_path):
    seld_env.set("SELD_DETERMINISTIC", "1")
    T = pkg().train
    _, ck, path = _train("off", tmp_path_factory)
    m = _tiny("tiny_DQ", at_key_size=8).to(DEV)
    T.load_model(m, None, path, True, torch.device(DEV))
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), ck["model_state_dict"][k]), k
    again = str(tmp_path / "again" / "checkpoint")
    T.save_model(m, None, dict(step=1), again)
    back = torch.load(again, map_location="cpu", weights_only=False)["model_state_dict"]
    assert list(back) == list(ck["model_state_dict"]) and all(torch.equal(back[k], ck["model_state_dict"][k]) for k in back)
    with pytest.raises(RuntimeError, match="at"):
        T.load_model(_tiny("tiny_DQ").to(DEV), None, path, True, torch.device(DEV))
