"""Squeeze-and-excitation on the device (csrc/squeeze_excite.hip): every kernel, element by element, against the fp64
formulas of tests/se_ref.py; bit reproducibility; the optimiser's gradient slots; the limits and refusals; the hook
positions in the model (identity gates); the model against fp64; the three training paths of train.main.

The kernels are called through the C ABI into NaN-filled buffers with sentinels behind them; the backward reference is
fed the fp32 z, h, s the forward kernels produced, so only the kernel under test separates the two sides.  Which form
ran is asked of the library (seld_se_kernel_label answers from the selection code the entry points run).

FORMS.  The kernels that sum (squeeze, bwd_reduce): row form (one wave per row, L = 64 lanes) for S < 1024, block form (one
256-thread workgroup per row, L = 256) from 1024 on: cases (1,4,1023) and (1,4,1024) sit on the two sides, (2,8,4099) is
the block form with a misaligned base.  The kernels that write (scale, bwd_apply) have one form, a wave per chunk of 256
floats of a row: (2,16,51) and (3,8,52) are less than one chunk, (1,24,1000) four chunks with a partial last one,
(2,8,4099) seventeen with head and tail elements.  x4: a row is head elements, aligned groups of four, tail elements; x1
(tensors of one call at different offsets from a 16-byte boundary): single elements --
test_misaligned_operands_take_the_element_walk.

BOUNDS.  u = 2^-24, componentwise, times 1 + 2^-10, plus 2^-126.  No credit for cancellation: every sum is charged
c_r u sum |term|, c_r the depth of the summation performed, plus the terms' own errors; a product of k factors given as
(value, error) pairs is charged prod(|v| + e) - prod |v| + (k - 1) u prod(|v| + e).
  rowsum, q rows   c_row = ceil(S / (4 L)) + 3 + 6 (+ 3 block form): the lane's chain of groups with its head and tail
                   element and the two adds inside a group; the xor butterfly; ((w0 + w1) + w2) + w3.
                   x1: ceil(S / L) + 6 (+ 3).  q's terms dy x carry one more u (the product).
  z                fold of the A row sums: A - 1 adds; fl(1 / (A S)) and the product: 2u |z|
  h                c = ceil(Cg / 64) + 6 + 1 (lane chain, butterfly, + b1), + 1 for the products; relu is 1-Lipschitz
  s                c = ceil(Hd / 64) + 6 + 1, + 1; the error of the pre-activation goes through the sigmoid exactly
                   (sigma(p +- e) in fp64), then 4u s (expf 1 ulp = 2u, the add, the division)
  y = x s          |x| e_s + u |x| (s + e_s)
  dp2 = (q s)(1 - s)   q: (c_row + 1 + A - 1) u sum |dy x|;  s exact (fed);  1 - s: u |1 - s|;  2 product roundings
  dh               one thread per column, g in order: c = Cg, + 1;   dz: c = Hd, + 1
  dW2, db2, dW1, db1   n in order: c = N (+ 1 for the products), terms (dp2 | dh with their errors) x (h | z exact, fed)
  dx = dy s + dz fl(1 / (A S))    (e_dz + 2u (|dz| + e_dz)) / (A S) + u |dy s| + u (|dy s| + |b| + e_b)
  slot after a second backward    both bounds + 2u |sum|

LARGEST ERROR / BOUND ON THE MI355X (printed by the tests; above 1 is a defect, not a reason to widen)
  case (form of the sums)  rowsum z     h     s     y     q     dp2   dh    dz    dw1   db1   dw2   db2   dx
  3x8x1     A1 H1  row     0.000 0.000 0.023 0.178 0.197 0.068 0.125 0.027 0.043 0.022 0.001 0.070 0.080 0.482
  2x16x51   A4 H2  row     0.156 0.089 0.021 0.071 0.127 0.068 0.037 0.020 0.029 0.017 0.009 0.017 0.036 0.207
  3x8x52    A8 H1  row     0.111 0.021 0.026 0.032 0.045 0.114 0.032 0.038 0.033 0.000 0.010 0.005 0.002 0.090
  1x24x1000 A1 H3  row     0.081 0.125 0.013 0.041 0.069 0.035 0.083 0.023 0.022 0.025 0.023 0.081 0.080 0.083
  2x8x4099  A4 H2  block   0.066 0.007 0.009 0.008 0.011 0.053 0.022 0.025 0.026 0.005 0.003 0.010 0.022 0.358
  2x320x20  A1 H40 row     0.178 0.194 0.012 0.033 0.051 0.129 0.183 0.003 0.001 0.003 0.003 0.180 0.119 0.002
  2x16x5x13 A8 H2  row     0.149 0.037 0.023 0.025 0.041 0.059 0.014 0.012 0.012 0.004 0.004 0.006 0.005 0.107
  5x12x260  A4 H3  row     0.112 0.049 0.038 0.029 0.044 0.067 0.049 0.028 0.029 0.018 0.012 0.034 0.031 0.074
  1x4x1023  A1 H1  row     0.068 0.050 0.004 0.056 0.134 0.021 0.049 0.005 0.011 0.010 0.005 0.043 0.048 0.193
  1x4x1024  A4 H1  block   0.079 0.010 0.009 0.090 0.184 0.070 0.044 0.031 0.023 0.021 0.031 0.045 0.043 0.254
  x shifted by 1 / 3 floats (x1 scale and bwd_reduce), worst of the four runs:  rowsum 0.157 | q 0.178 | y 0.127 | dx 0.333
  gradient slots after the second backward:  dw1 0.009 | db1 0.006 | dw2 0.016 | db2 0.015 | dx 0.074
  model against fp64 (outputs, absolute | worst gradient by the criterion of the test, and where):
    tiny_Q   1.5e-07 | 0.69e-3  tcn.attention.keys.weight        tiny_DQ  3.0e-07 | 0.53e-3  cnn.2.5.fc1.weight
    tiny_R   9.3e-08 | 0.02e-3  cnn.2.0.weight
No ratio is above 1.  The elementwise quantities use up to half of their bounds (dx at S = 1, where the bound is a handful
of roundings), the sums a tenth to a fifth: c_r u sum |term| charges every rounding with the same sign.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import se_ref as R
from tests.golden.cases import MODEL_CASES, model_kwargs, train_target
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TINY = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -10
SENTINEL = -1234.5
EUNSUPPORTED = -4
BLOCK_MIN_S = 1024
CASE = {c["name"]: c for c in MODEL_CASES}


# ======================================================================================================================
# plumbing
# ======================================================================================================================
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


def _B(e):
    return SLACK * e + TINY


def _ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (both fp64 on the host)."""
    err = (got.double().cpu() - ref).abs()
    assert torch.isfinite(err).all()
    return float((err / _B(bound)).max())


def _prod(*pairs):
    """Error bound of a product of (value, error) factors evaluated left to right in fp32."""
    hi = functools.reduce(lambda a, b: a * b, [v.abs() + e for v, e in pairs])
    lo = functools.reduce(lambda a, b: a * b, [v.abs() for v, _ in pairs])
    return hi - lo + (len(pairs) - 1) * U * hi


def _c_row(S, vec=True):
    L = 256 if S >= BLOCK_MIN_S else 64
    c = (math.ceil(S / (4 * L)) + 3 if vec else math.ceil(S / L)) + 6
    return c + (3 if S >= BLOCK_MIN_S else 0)


def _fold_abs(t, N, A, Cg):
    return t.abs().reshape(N, A, Cg, -1).sum(dim=(1, 3))


def _per_channel(t, A, shape):
    """(N, Cg) -> broadcastable over x (N, C, *spatial): channel k Cg + g takes column g."""
    return t.repeat(1, A).reshape(shape[0], shape[1], *([1] * (len(shape) - 2)))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """fp32 inputs of a case on the host (made once, never modified)."""
    return tuple(t.float() for t in R.make_case(case))


def _shifted(t, shift):
    """A device copy of `t` whose first element sits `shift` floats behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _run_kernels(case, x_shift=0, accumulate_into=None):
    """All six entry points on a case through the C ABI.  Returns dict(name -> device view), dict(name -> (buffer, n))."""
    L = pkg()._lib
    lib, st = L.lib(), L.current_stream()
    N, C, spatial, A, Hd = case
    Cg, S = C // A, int(np.prod(spatial))
    x, dy, w1, b1, w2, b2 = _inputs(case)
    xd = _shifted(x, x_shift)
    dyd, w1d, b1d, w2d, b2d = (t.to(DEV) for t in (dy, w1, b1, w2, b2))
    sizes = dict(rowsum=N * C, z=N * Cg, h=N * Hd, s=N * Cg, y=N * C * S, q=N * C, dp2=N * Cg, dh=N * Hd, dz=N * Cg,
                 dw1=Hd * Cg, db1=Hd, dw2=Cg * Hd, db2=Cg, dx=N * C * S)
    o, bufs = {}, {}
    for k, n in sizes.items():
        o[k], buf = _out(n)
        bufs[k] = (buf, n)
    p = L.ptr
    L.check(lib.seld_se_squeeze(p(xd), N * C, S, p(o["rowsum"]), st), "squeeze")
    L.check(lib.seld_se_excite_fwd(p(o["rowsum"]), N, C, S, A, Hd, p(w1d), p(b1d), p(w2d), p(b2d), p(o["z"]), p(o["h"]),
                                   p(o["s"]), st), "excite_fwd")
    L.check(lib.seld_se_scale(p(xd), N, C, S, A, p(o["s"]), p(o["y"]), st), "scale")
    L.check(lib.seld_se_bwd_reduce(p(dyd), p(xd), N * C, S, p(o["q"]), st), "bwd_reduce")
    acc = 0
    if accumulate_into is not None:
        for k in ("dw1", "db1", "dw2", "db2"):
            o[k].copy_(accumulate_into[k].reshape(-1))
        acc = 1
    L.check(lib.seld_se_excite_bwd(p(o["q"]), N, C, A, Hd, p(w1d), p(w2d), p(o["z"]), p(o["h"]), p(o["s"]), p(o["dp2"]),
                                   p(o["dh"]), p(o["dz"]), p(o["dw1"]), p(o["db1"]), p(o["dw2"]), p(o["db2"]), acc, st),
            "excite_bwd")
    L.check(lib.seld_se_bwd_apply(p(dyd), N, C, S, A, p(o["s"]), p(o["dz"]), p(o["dx"]), st), "bwd_apply")
    torch.cuda.synchronize()
    return o, bufs


def _check_all(case, o, vec_reduce=True, prior=None):
    """Every output of `_run_kernels` against its bound; returns {quantity: largest error / bound}."""
    N, C, spatial, A, Hd = case
    Cg, S = C // A, int(np.prod(spatial))
    x, dy, w1, b1, w2, b2 = (t.double() for t in _inputs(case))
    shape = x.shape
    inv = 1.0 / (A * S)
    rat = {}
    # ---- forward ----
    absx = x.abs().reshape(N * C, S).sum(1)
    c_sq = _c_row(S)
    rat["rowsum"] = _ratio(o["rowsum"], x.reshape(N * C, S).sum(1), c_sq * U * absx)
    f = R.se_forward(x, w1, b1, w2, b2, A)
    absx_g = _fold_abs(x, N, A, Cg)
    e1 = (c_sq + A - 1) * U * absx_g * inv
    e_z = e1 + 2 * U * (f["z"].abs() + e1)
    rat["z"] = _ratio(o["z"].view(N, Cg), f["z"], e_z)
    c_h = math.ceil(Cg / 64) + 6 + 1
    e_h = e_z @ w1.abs().T + (c_h + 1) * U * ((f["z"].abs() + e_z) @ w1.abs().T + b1.abs())
    rat["h"] = _ratio(o["h"].view(N, Hd), f["h"], e_h)
    c_s = math.ceil(Hd / 64) + 6 + 1
    e_p = e_h @ w2.abs().T + (c_s + 1) * U * ((f["h"] + e_h) @ w2.abs().T + b2.abs())
    pre = f["h"] @ w2.T + b2
    sig = lambda t: 1.0 / (1.0 + torch.exp(-t))
    e_s = torch.maximum(sig(pre + e_p) - f["s"], f["s"] - sig(pre - e_p)) + 4 * U * f["s"]
    rat["s"] = _ratio(o["s"].view(N, Cg), f["s"], e_s)
    e_sx = _per_channel(e_s, A, shape)
    s_x = _per_channel(f["s"], A, shape)
    rat["y"] = _ratio(o["y"].view(shape), f["y"], x.abs() * e_sx + U * x.abs() * (s_x + e_sx))
    # ---- backward, from the fp32 z, h, s of the forward kernels ----
    z32, h32, s32 = (o[k].double().cpu().view(N, -1) for k in ("z", "h", "s"))
    b = R.se_backward(x, dy, w1, w2, z32, h32, s32, A)
    c_q = _c_row(S, vec_reduce)
    absq = (dy * x).abs().reshape(N * C, S).sum(1)
    rat["q"] = _ratio(o["q"], (dy * x).reshape(N * C, S).sum(1), (c_q + 1) * U * absq)
    e_q = (c_q + A) * U * _fold_abs(dy * x, N, A, Cg)
    zero = torch.zeros_like(s32)
    e_dp2 = _prod((b["q"], e_q), (s32, zero), (1 - s32, U * (1 - s32).abs()))
    rat["dp2"] = _ratio(o["dp2"].view(N, Cg), b["dp2"], e_dp2)
    live = (h32 > 0).double()
    e_dh = (e_dp2 @ w2.abs() + (Cg + 1) * U * ((b["dp2"].abs() + e_dp2) @ w2.abs())) * live
    rat["dh"] = _ratio(o["dh"].view(N, Hd), b["dh"], e_dh)
    e_dz = e_dh @ w1.abs() + (Hd + 1) * U * ((b["dh"].abs() + e_dh) @ w1.abs())
    rat["dz"] = _ratio(o["dz"].view(N, Cg), b["dz"], e_dz)
    dp2a, dha = b["dp2"].abs() + e_dp2, b["dh"].abs() + e_dh
    bounds = dict(dw1=e_dh.T @ z32.abs() + (N + 1) * U * (dha.T @ z32.abs()), db1=e_dh.sum(0) + N * U * dha.sum(0),
                  dw2=e_dp2.T @ h32.abs() + (N + 1) * U * (dp2a.T @ h32.abs()), db2=e_dp2.sum(0) + N * U * dp2a.sum(0))
    for k, e in bounds.items():
        ref = b[k]
        if prior is not None:           # the sum was added to what the slot held: both bounds + 2u |sum|
            ref = ref + prior[k].double().cpu().view(ref.shape)
            e = 2 * e + 2 * U * ref.abs()
        rat[k] = _ratio(o[k].view(ref.shape), ref, e)
    add = b["dz"] * inv
    e_b = (e_dz + 2 * U * (b["dz"].abs() + e_dz)) * inv
    dys = (dy * _per_channel(s32, A, shape)).abs()
    e_dx = _per_channel(e_b, A, shape) + U * dys + U * (dys + _per_channel(add.abs() + e_b, A, shape))
    rat["dx"] = _ratio(o["dx"].view(shape), b["dx"], e_dx)
    return rat


def _label(op, S, same_phase=1):
    return pkg().hip_ops.se_kernel_label(op, S, same_phase)


# ======================================================================================================================
# the kernels against their bounds
# ======================================================================================================================
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_kernels_hold_their_bounds(case):
    N, C, spatial, A, Hd = case
    S = int(np.prod(spatial))
    form = "block" if S >= BLOCK_MIN_S else "row"
    for op in ("squeeze", "bwd_reduce"):
        assert _label(op, S) == f"se_{op}_{form}_kernel[x4]"
    for op in ("scale", "bwd_apply"):
        assert _label(op, S) == f"se_{op}_chunk_kernel[x4]"
    o, bufs = _run_kernels(case)
    for k, (buf, n) in bufs.items():
        assert _guards_intact(buf, n), k
        assert not bool(buf[8:8 + n].isnan().any()), f"{k}: elements left unwritten"
    rat = _check_all(case, o)
    print("SE", R.case_id(case), form, " ".join(f"{k} {v:.3f}" for k, v in rat.items()))
    assert max(rat.values()) <= 1.0, rat


@pytest.mark.parametrize("case", [R.CASES[1], R.CASES[4]], ids=R.case_id)
@pytest.mark.parametrize("shift", [1, 3])
def test_misaligned_operands_take_the_element_walk(case, shift):
    """x `shift` floats behind a 16-byte boundary, every other tensor on one: the squeeze still uses 16-byte loads (its
    heads move), scale and bwd_reduce walk single elements, bwd_apply (dy, dx) keeps the x4 form."""
    S = int(np.prod(case[2]))
    form = "block" if S >= BLOCK_MIN_S else "row"
    assert _label("scale", S, 0) == "se_scale_chunk_kernel[x1]"
    assert _label("bwd_reduce", S, 0) == f"se_bwd_reduce_{form}_kernel[x1]"
    assert _label("squeeze", S, 0) == f"se_squeeze_{form}_kernel[x4]"
    o, bufs = _run_kernels(case, x_shift=shift)
    for k, (buf, n) in bufs.items():
        assert _guards_intact(buf, n) and not bool(buf[8:8 + n].isnan().any()), k
    rat = _check_all(case, o, vec_reduce=False)
    print("SE shifted", shift, R.case_id(case), " ".join(f"{k} {v:.3f}" for k, v in rat.items()))
    assert max(rat.values()) <= 1.0, rat


def test_element_offsets_past_2_to_the_31():
    """Three rows of 2^30 floats (12.9 GB, the block form; row 2 starts at element 2^31): ones, the last 128 elements of
    the last row 2.0.  Every partial sum of the kernels' order is an integer that fp32 holds exactly (the 32 groups of twos
    fall to lanes 32..63 of wave 3: + 4 a lane, 2^28 + 128 for the wave), so the row sums are exactly 2^30, 2^30, 2^30 + 128,
    and q of (dy, x) = (x, x) is 2^30, 2^30, 2^30 + 384.  y = x s with gates 1/2, 1/4, 1/8 is exact too and compared whole.
    No host reference is needed, so the test stays quick."""
    L = pkg()._lib
    lib, st, p = L.lib(), L.current_stream(), L.ptr
    S = 1 << 30
    x = torch.ones((1, 3, S), device=DEV)
    x[0, 2, -128:] = 2.0
    rowsum, rbuf = _out(3)
    q, qbuf = _out(3)
    L.check(lib.seld_se_squeeze(p(x), 3, S, p(rowsum), st), "squeeze")
    L.check(lib.seld_se_bwd_reduce(p(x), p(x), 3, S, p(q), st), "bwd_reduce")
    assert rowsum.tolist() == [2.0 ** 30, 2.0 ** 30, 2.0 ** 30 + 128] and _guards_intact(rbuf, 3)
    assert q.tolist() == [2.0 ** 30, 2.0 ** 30, 2.0 ** 30 + 384] and _guards_intact(qbuf, 3)
    gates = torch.tensor([0.5, 0.25, 0.125], device=DEV)
    y = torch.full_like(x, float("nan"))
    L.check(lib.seld_se_scale(p(x), 1, 3, S, 1, p(gates), p(y), st), "scale")
    y.div_(gates.view(1, 3, 1))          # exact: powers of two
    assert torch.equal(y, x)
    dz = torch.tensor([float(S), 2.0 * S, 4.0 * S], device=DEV)         # dz / (A S) = 1, 2, 4
    L.check(lib.seld_se_bwd_apply(p(x), 1, 3, S, 1, p(gates), p(dz), p(y), st), "bwd_apply")
    want = [(0.5 + 1, 0.5 + 1), (0.25 + 2, 0.25 + 2), (0.125 + 4, 0.25 + 4)]
    for c, (first, last) in enumerate(want):
        row = y[0, c]
        assert float(row[0]) == first and float(row[-1]) == last and float(row.min()) == first and float(row.max()) == last
    assert int((y[0, 2] == 4.25).sum()) == 128


def _autograd_run(case):
    H = pkg().hip_ops
    x, dy, w1, b1, w2, b2 = (t.to(DEV) for t in _inputs(case))
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = H.squeeze_excite(*leaves, components=case[3])
    y.backward(dy)
    torch.cuda.synchronize()
    return [y.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_autograd_function_returns_the_kernels_results_bit_for_bit(case, seld_env):
    """hip_ops.squeeze_excite / se_gates against the raw calls above (which the bounds hold), and two runs of forward and
    backward with and two without SELD_DETERMINISTIC: all equal."""
    H = pkg().hip_ops
    o, _ = _run_kernels(case)
    names = ("y", "dx", "dw1", "db1", "dw2", "db2")
    runs = [_autograd_run(case), _autograd_run(case)]
    seld_env.set("SELD_DETERMINISTIC", "1")
    runs += [_autograd_run(case), _autograd_run(case)]
    for run in runs:
        for name, got in zip(names, run):
            assert torch.equal(got.reshape(-1), o[name]), name
    x, _, w1, b1, w2, b2 = (t.to(DEV) for t in _inputs(case))
    s = H.se_gates(x, w1, b1, w2, b2, components=case[3])
    assert s.shape == (case[0], case[1] // case[3]) and torch.equal(s.reshape(-1), o["s"])


def test_gradient_slots_of_a_flat_adam_accumulate():
    """Parameters owned by a FlatAdam: backward returns no parameter gradient and adds into the flat buffer; a second
    backward adds again (both bounds + 2u |sum|); the buffer's other slots and the sentinel parameter around are untouched."""
    T, H, NN = pkg().train, pkg().hip_ops, pkg().hip_nn
    case = R.CASES[7]
    N, C, spatial, A, Hd = case
    x, dy, w1, b1, w2, b2 = (t.to(DEV) for t in _inputs(case))
    m = NN.SqueezeExcite(C, (C // A) // Hd, A).to(DEV)
    assert m.hidden == Hd
    front, back = (torch.nn.Parameter(torch.full((5,), 2.0, device=DEV)) for _ in range(2))
    opt = T.FlatAdam([front] + list(m.parameters()) + [back], lr=1e-3)
    with torch.no_grad():
        for p, v in zip(m.parameters(), (w1, b1, w2, b2)):
            p.copy_(v)
    opt.zero_grad()
    xg = x.clone().requires_grad_(True)
    for rounds in (1, 2):
        y = m(xg)
        grads = torch.autograd.grad(y, [xg] + list(m.parameters()), dy, allow_unused=True)
        assert all(g is None for g in grads[1:]), "parameter gradients go to the slots, not through autograd"
        torch.cuda.synchronize()
        once, _ = _run_kernels(case)
        got = {k: p.grad.reshape(-1) for k, p in zip(("dw1", "db1", "dw2", "db2"), m.parameters())}
        if rounds == 1:
            for k in got:
                assert torch.equal(got[k], once[k]), k
            first = {k: v.clone() for k, v in got.items()}
        else:
            twice, _ = _run_kernels(case, accumulate_into=first)
            for k in got:
                assert torch.equal(got[k], twice[k]), k
            rat = _check_all(case, twice, prior=first)
            print("SE slots", " ".join(f"{k} {rat[k]:.3f}" for k in ("dw1", "db1", "dw2", "db2", "dx")))
            assert max(rat.values()) <= 1.0, rat
        assert torch.equal(grads[0].reshape(-1), once["dx"])
    n_se = sum(p.numel() for p in m.parameters())
    assert torch.equal(opt.flat_grad[:5], torch.zeros(5, device=DEV)) and torch.equal(opt.flat_grad[5 + n_se:], torch.zeros(5, device=DEV))
    assert all(p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * off for p, off in zip(opt.params, opt.offsets))


# ======================================================================================================================
# limits and refusals
# ======================================================================================================================
@pytest.mark.parametrize("Cg, Hd", [(4097, 1), (4, 1025)], ids=["gated", "hidden"])
def test_over_the_limits_is_unsupported_and_writes_nothing(Cg, Hd):
    L, H = pkg()._lib, pkg().hip_ops
    assert (H.SE_MAX_GATED, H.SE_MAX_HIDDEN) == (4096, 1024)
    lib, st, p = L.lib(), L.current_stream(), L.ptr
    N, S, A, C = 1, 2, 1, Cg
    ins = {k: torch.zeros(n, device=DEV) for k, n in dict(rowsum=N * C, w1=Hd * Cg, b1=Hd, w2=Cg * Hd, b2=Cg, q=N * C).items()}
    outs = {k: _out(n) for k, n in dict(z=N * Cg, h=N * Hd, s=N * Cg, dp2=N * Cg, dh=N * Hd, dz=N * Cg, dw1=Hd * Cg, db1=Hd,
                                        dw2=Cg * Hd, db2=Cg).items()}
    v = {k: t[0] for k, t in outs.items()}
    rc = lib.seld_se_excite_fwd(p(ins["rowsum"]), N, C, S, A, Hd, p(ins["w1"]), p(ins["b1"]), p(ins["w2"]), p(ins["b2"]),
                                p(v["z"]), p(v["h"]), p(v["s"]), st)
    assert rc == EUNSUPPORTED
    # the backward reads z, h, s as inputs: NaN-filled buffers do, nothing is launched
    rc = lib.seld_se_excite_bwd(p(ins["q"]), N, C, A, Hd, p(ins["w1"]), p(ins["w2"]), p(v["z"]), p(v["h"]), p(v["s"]),
                                p(v["dp2"]), p(v["dh"]), p(v["dz"]), p(v["dw1"]), p(v["db1"]), p(v["dw2"]), p(v["db2"]), 0, st)
    assert rc == EUNSUPPORTED
    torch.cuda.synchronize()
    for k, (view, buf) in outs.items():
        assert _untouched(buf, view.numel()), k
    x = torch.zeros((N, C, S), device=DEV)
    with pytest.raises(L.SeldHipError, match="LDS"):
        H.squeeze_excite(x, ins["w1"].view(Hd, Cg), ins["b1"], ins["w2"].view(Cg, Hd), ins["b2"], 1)


def test_host_refusals():
    L, H = pkg()._lib, pkg().hip_ops
    x, _, w1, b1, w2, b2 = (t.to(DEV) for t in _inputs(R.CASES[1]))        # (2, 16, 51), A 4, Hd 2
    good = (x, w1, b1, w2, b2)
    assert H.squeeze_excite(*good, components=4).shape == x.shape
    with pytest.raises(L.SeldHipError, match="multiple"):
        H.squeeze_excite(x[:, :14].contiguous(), w1, b1, w2, b2, components=4)
    with pytest.raises(L.SeldHipError, match="device tensor"):
        H.squeeze_excite(x.cpu(), w1, b1, w2, b2, components=4)
    with pytest.raises(L.SeldHipError, match="device tensor"):
        H.squeeze_excite(x, w1.cpu(), b1, w2, b2, components=4)
    with pytest.raises(L.SeldHipError, match="contiguous"):
        H.squeeze_excite(x.transpose(0, 1).contiguous().transpose(0, 1), w1, b1, w2, b2, components=4)
    with pytest.raises(L.SeldHipError, match="float32"):
        H.squeeze_excite(x.double(), w1, b1, w2, b2, components=4)
    with pytest.raises(L.SeldHipError, match="components"):
        H.squeeze_excite(*good, components=2)
    with pytest.raises(L.SeldHipError, match="w1"):
        H.squeeze_excite(x, w1[:, :3].contiguous(), b1, w2, b2, components=4)
    with pytest.raises(L.SeldHipError, match="expected b1"):
        H.squeeze_excite(x, w1, b1, w2.T.contiguous(), b2, components=4)
    with pytest.raises(L.SeldHipError):
        H.se_gates(x.cpu(), w1, b1, w2, b2, components=4)


# ======================================================================================================================
# identity gates: the hook positions in the model
# ======================================================================================================================
def test_saturated_gate_is_exactly_one():
    H = pkg().hip_ops
    x, _, w1, b1, w2, b2 = (t.to(DEV) for t in _inputs(R.CASES[3]))
    s = H.se_gates(x, w1, b1, torch.zeros_like(w2), torch.full_like(b2, 30.0), components=1)
    assert torch.equal(s, torch.ones_like(s))
    y = H.squeeze_excite(x, w1, b1, torch.zeros_like(w2), torch.full_like(b2, 30.0), components=1)
    assert torch.equal(y, x)


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
def test_identity_gates_leave_the_model_unchanged(train, seld_env):
    """tiny DQ model, dropout 0, SELD_DETERMINISTIC=1: se_reduction=4 with fc2.weight = 0, fc2.bias = 30 (s == 1.0f
    exactly) on top of the se_reduction=0 model's state dict gives the same outputs and the same gradient of every non-SE
    parameter, bit for bit: the hooks multiply the right tensors and nothing else moved."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    H = pkg().hip_ops
    x, target = _model_inputs("tiny_DQ")
    off, on = _tiny("tiny_DQ"), _tiny("tiny_DQ", se_reduction=4)
    sd = {k: v.clone() for k, v in off.state_dict().items()}
    for k, v in on.state_dict().items():
        if k not in sd:
            sd[k] = torch.zeros_like(v) if k.endswith("fc2.weight") else torch.full_like(v, 30.0) if k.endswith("fc2.bias") else v
    on.load_state_dict(sd)
    res = []
    for m in (off, on):
        H.philox.set_offset(0)
        H.hcq_weights.reset()
        res.append(_step(m, x, target, train))
    (sed0, doa0, g0), (sed1, doa1, g1) = res
    assert torch.equal(sed0, sed1) and torch.equal(doa0, doa1)
    assert len(g1) == len(g0) + 52 * train
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ======================================================================================================================
# the model against fp64
# ======================================================================================================================
@pytest.mark.parametrize("name", ["tiny_Q", "tiny_DQ", "tiny_R"])
def test_model_with_se_matches_fp64(name, seld_env):
    """Forward and one backward of the tiny models (the closed-form weights of the model fixtures, random SE weights,
    se_reduction=2) against the same walk in fp64 on the CPU: the oracle's layers with tests/se_ref.py's
    squeeze-and-excitation at the two hook points.  The project's tolerance: 1e-3 on the SED and DOA outputs; gradients
    by the criterion of tests/test_gpu_model.py (below).  SELD_DETERMINISTIC=1: the figures are the same in every run."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    from oracle import seld_oracle as O
    H = pkg().hip_ops
    case = CASE[name]
    x, target = _model_inputs(name)
    m = _tiny(name, se_reduction=2)
    O.closed_form_fill_([(k, v) for k, v in m.state_dict().items() if ".fc1." not in k and ".fc2." not in k])
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".fc2." in k or ".fc1." in k:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 if "weight" in k else 0.5))
    sd64 = {k: v.detach().double().clone() for k, v in m.state_dict().items()}
    for v in sd64.values():
        v.requires_grad_(v.is_floating_point())
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    sed, doa, grads = _step(m, x, target, True)
    cfg = O.SeldConfig(**model_kwargs(case))
    rsed, rdoa = R.seld_forward_se(sd64, cfg, x.double(), train=True)
    O.seld_loss(rsed, rdoa, target.double(), 42).backward()
    err = max(float((sed.cpu().double() - rsed.detach()).abs().max()), float((doa.cpu().double() - rdoa.detach()).abs().max()))
    print("SE model", name, "max |out - fp64|", err)
    assert err <= 1e-3
    # the criterion of tests/test_gpu_model.py: every gradient to 1e-3 of its largest entry, with the floor used there --
    # a gradient below 1e-4 of the largest RMS over the parameters is fp32 cancellation noise in either stack (the
    # attention's keys.weight, whose gradient vanishes by the softmax's shift invariance), so the scale is never below
    # 10 floors
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
    se_grads = [k for k in grads if ".fc2.bias" in k]       # never zero; a hidden unit's ReLU may be off for the whole batch
    assert len(se_grads) == 13 and all(float(sd64[k].grad.abs().max()) > 0 for k in se_grads)
    assert any(float(sd64[k].grad.abs().max()) > 0 for k in grads if ".fc1.weight" in k)
    print("SE model", name, "worst gradient error / largest entry", worst, worst_at)


# ======================================================================================================================
# training paths
# ======================================================================================================================
_runs = {}


def _run(mode, tmp_path_factory):
    """train.main with --se_reduction=4, 2 epochs on write_pickles data: each mode run once and shared."""
    from tests import test_gpu_train_loader as TL
    if "paths" not in _runs:
        _runs["paths"] = TL.write_pickles(tmp_path_factory.mktemp("se_pickles"), 5)
    if mode not in _runs:
        extra = {"off": {}, "resident": dict(resident_loader="True"),
                 "graph": dict(resident_loader="True", graph_step="True")}[mode]
        _runs[mode] = TL._main(_runs["paths"], str(tmp_path_factory.mktemp("se_" + mode)), 2, se_reduction=4, **extra)
    return _runs[mode]


def test_resident_loader_run_equals_the_eager_run_with_se_on(seld_env, tmp_path_factory):
    """train.main --se_reduction=4 under SELD_DETERMINISTIC=1: the --resident_loader run equals the flags-off run bit for
    bit (parameters, BatchNorm buffers, Adam moments, both losses of both epochs); the checkpoint holds the 52 SE tensors,
    and every fc2.bias (whose gradient is never zero) has a non-zero first moment: the slots reached Adam."""
    from tests import test_gpu_train_loader as TL
    seld_env.set("SELD_DETERMINISTIC", "1")
    (h_off, ck_off, _), (h_res, ck_res, _) = _run("off", tmp_path_factory), _run("resident", tmp_path_factory)
    a, b = TL._tensors(ck_off), TL._tensors(ck_res)
    assert a.keys() == b.keys()
    se = [k for k in ck_off["model_state_dict"] if ".fc1." in k or ".fc2." in k]
    assert len(se) == 52
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert h_res == h_off and len(h_off) == 2, (h_res, h_off)
    params = [k for k in ck_off["model_state_dict"] if "running_" not in k and "num_batches" not in k]
    state = ck_off["optimizer_state_dict"]["state"]
    moved = [k for i, k in enumerate(params) if k.endswith("fc2.bias") and ("cnn" in k or ".se." in k)
             and float(state[i]["exp_avg"].abs().max()) > 0]
    assert len(moved) == 13, moved


def test_graph_step_run_matches_the_eager_run_with_se_on(seld_env, tmp_path_factory):
    """The --graph_step run against the flags-off run at the tolerance of tests/test_gpu_train_loader.py: the SE launches
    record and replay."""
    from tests import test_gpu_train_loader as TL
    seld_env.set("SELD_DETERMINISTIC", "1")
    (h_off, ck_off, _), (h_g, ck_g, _) = _run("off", tmp_path_factory), _run("graph", tmp_path_factory)
    a, c = TL._tensors(ck_off), TL._tensors(ck_g)
    assert a.keys() == c.keys()
    TL._compare_graph_to_eager(a, c)
    assert np.allclose([t for _, t, _ in h_g], [t for _, t, _ in h_off], rtol=1e-6, atol=0), (h_g, h_off)
    assert np.allclose([v for _, _, v in h_g], [v for _, _, v in h_off], rtol=1e-6, atol=0), (h_g, h_off)


def test_checkpoint_with_se_round_trips(seld_env, tmp_path_factory, tmp_path):
    seld_env.set("SELD_DETERMINISTIC", "1")
    T = pkg().train
    _, ck, path = _run("off", tmp_path_factory)
    m = _tiny("tiny_DQ", se_reduction=4).to(DEV)
    T.load_model(m, None, path, True, torch.device(DEV))
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), ck["model_state_dict"][k]), k
    again = str(tmp_path / "again" / "checkpoint")
    T.save_model(m, None, dict(step=1), again)
    back = torch.load(again, map_location="cpu", weights_only=False)["model_state_dict"]
    assert list(back) == list(ck["model_state_dict"]) and all(torch.equal(back[k], ck["model_state_dict"][k]) for k in back)
    with pytest.raises(RuntimeError, match="fc1"):
        T.load_model(_tiny("tiny_DQ").to(DEV), None, path, True, torch.device(DEV))
