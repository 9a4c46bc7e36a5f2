"""The permutation-invariant SELD loss (csrc/train_step.hip: loss_pit_kernel; hip_ops.seld_loss_pit; train.py --pit_loss)
against the fp64 brute force of tests/pit_loss_ref.py, which also makes the inputs.

Bounds, those tests/test_gpu_train_step.py holds the plain loss to (u = 2^-24, floor of one fp32 denormal):
    |loss - ref| <= 1e-5 max(1, |ref|)         |parts[0] + parts[1] - loss| : the same bound
    |dsed - ref| <= 8u |ref|                    |ddoa - ref| <= 4u |ref|
perm equals the reference's wherever the cell's target slots are pairwise distinct.  Cells the reference marks ambiguous
(another target within 1e-4 of the summed pair costs of the best: an fp32 evaluation may choose it) are left out of the
gradient and perm checks; the reference must find none at the four small shapes and at most 0.1 % of the cells with a
choice at (4700, 14, 3), and a target other than the given one must win in at least 20 % of the cells with a choice, so a
kernel that never permutes cannot pass.

Largest error / bound seen on the MI355X (printed by the tests; a ratio above 1 is a defect, not a reason to widen), and
what the reference found in the inputs (cells with a choice / of them won by another target / ambiguous):

  case                 dsed   ddoa   loss   parts    cells            case                    dsed   ddoa   loss   parts
  1x14x3    w1,5       0.219  0.352  0.003  0.009    4 / 3 / 0        1x14x3    w0.25,3       0.219  0.620  0.003  0.003
  37x14x3   w1,5       0.282  0.274  0.001  0.000    202 / 165 / 0    37x14x3   w0.25,3       0.282  0.291  0.004  0.004
  64x1x3    w1,5       0.321  0.436  0.008  0.006    21 / 16 / 0      64x1x3    w0.25,3       0.321  0.331  0.000  0.000
  37x14x2   w1,5       0.345  0.274  0.007  0.011    204 / 93 / 0     37x14x2   w0.25,3       0.345  0.415  0.003  0.001
  4700x14x3 w1,5       0.432  0.683  0.002  0.003    26374 / 20361 / 16   4700x14x3 w0.25,3   0.432  0.414  0.002  0.001
  edge values          0.259  0.427"""
import collections
import math
import os

import numpy as np
import pytest
import torch

from oracle import seld_oracle as O
from tests import pit_loss_ref as R
from tests.golden.cases import MODEL_CASES
from tests.helpers import build_model, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
DENORM = 2.0 ** -149
SENTINEL = -1234.5
SHAPES = [(1, 14, 3), (37, 14, 3), (64, 1, 3), (37, 14, 2), (4700, 14, 3)]      # the last: more cells than 256 x 256 threads
WEIGHTS = [(1.0, 5.0), (0.25, 3.0)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _guarded(x, extra=4):
    """x on the device, followed by `extra` sentinel elements: (view of the first x.numel(), whole buffer)."""
    buf = torch.full((x.numel() + extra,), SENTINEL, dtype=x.dtype)
    buf[:x.numel()] = x.reshape(-1)
    buf = buf.to(DEV)
    return buf[:x.numel()], buf


def _guards_intact(buf, n):
    return torch.equal(buf[n:].cpu(), torch.full((buf.numel() - n,), SENTINEL).to(buf.dtype))


_cases = {}


def case(shape, weights):
    """Inputs and fp64 reference of a case, computed once and shared (read only)."""
    key = (shape, weights)
    if key not in _cases:
        if ("inputs", shape) not in _cases:
            _cases[("inputs", shape)] = R.pit_inputs(*shape, seed=sum(shape))
        inputs = _cases[("inputs", shape)]
        _cases[key] = (inputs, R.pit_reference(*inputs, shape[1], shape[2], *weights))
    return _cases[key]


def check(got, ref, overlaps, what):
    """Asserts the bounds of the module docstring on (loss, dsed, ddoa, perm, parts); returns the largest error / bound
    of (dsed, ddoa)."""
    loss, dsed, ddoa, perm, parts = got
    rows, C = ref["perm"].shape
    bound = 1e-5 * max(1.0, abs(ref["loss"]))
    assert abs(loss - ref["loss"]) <= bound, f"{what}: loss {loss!r}, fp64 reference {ref['loss']!r}"
    if parts is not None:
        assert abs(parts[0] + parts[1] - loss) <= bound, f"{what}: parts {parts!r} against loss {loss!r}"
        assert abs(parts[0] - ref["parts"][0]) <= bound and abs(parts[1] - ref["parts"][1]) <= bound, (parts, ref["parts"])
    keep = ~ref["ambiguous"]
    worst = []
    for name, x, r, k, per in (("dsed", dsed, ref["dsed"], 8, overlaps), ("ddoa", ddoa, ref["ddoa"], 4, 3 * overlaps)):
        err, lim = (x.double() - r).abs(), k * U * r.abs() + DENORM
        ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
        ratio = ratio * keep[..., None].expand(rows, C, per).reshape(rows, -1)
        i = int(ratio.argmax())
        worst.append(float(ratio.view(-1)[i]))
        assert worst[-1] <= 1.0, (f"{what}: {name}[{i}] = {float(x.view(-1)[i])!r}, fp64 reference "
                                  f"{float(r.view(-1)[i])!r}, error / bound = {worst[-1]:.3f}")
    if perm is not None:
        m = keep & ref["distinct"]
        assert torch.equal(perm.long()[m], ref["perm"][m]), f"{what}: perm differs in {int((perm.long() != ref['perm'])[m].sum())} cells"
        assert int(perm.min()) >= 0 and int(perm.max()) < math.factorial(overlaps)
    return worst


def c_abi(sed, doa, tgt, rows, C, overlaps, weights, grads=True, perm=True, parts=True):
    """seld_loss_pit_fwd_bwd on device tensors into NaN-poisoned (perm: -1) outputs with guard elements behind them.
    Returns {name: (view, whole buffer, elements)}; an output not asked for is passed as NULL."""
    L = pkg()._lib
    n = rows * C * overlaps
    out = {"loss": _guarded(torch.full((1,), float("nan"))) + (1,)}
    if grads:
        out["dsed"] = _guarded(torch.full((n,), float("nan"))) + (n,)
        out["ddoa"] = _guarded(torch.full((3 * n,), float("nan"))) + (3 * n,)
    if perm:
        out["perm"] = _guarded(torch.full((rows * C,), -1, dtype=torch.int32)) + (rows * C,)
    if parts:
        out["parts"] = _guarded(torch.full((2,), float("nan"))) + (2,)
    p = {k: L.ptr(v[0]) for k, v in out.items()}
    L.check(L.lib().seld_loss_pit_fwd_bwd(L.ptr(sed), L.ptr(doa), L.ptr(tgt), rows, C, overlaps, *weights, p["loss"],
                                          p.get("dsed"), p.get("ddoa"), p.get("perm"), p.get("parts"), L.current_stream()),
            "seld_loss_pit_fwd_bwd")
    torch.cuda.synchronize()
    for k, (_, buf, count) in out.items():
        assert _guards_intact(buf, count), f"{k}: written past its end"
    return out


_IDS = [f"{'x'.join(map(str, s))}-w{w[0]:g},{w[1]:g}" for s in SHAPES for w in WEIGHTS]


# ======================================================================================================================
# 1. per element
# ======================================================================================================================
@pytest.mark.parametrize("shape,weights", [(s, w) for s in SHAPES for w in WEIGHTS], ids=_IDS)
def test_pit_loss_per_element(shape, weights):
    H = pkg().hip_ops
    (sed, doa, tgt), ref = case(shape, weights)
    rows, C, overlaps = shape
    what = f"pit[{'x'.join(map(str, shape))}-w{weights[0]:g},{weights[1]:g}]"
    choice, ambiguous = int(ref["choice"].sum()), int(ref["ambiguous"].sum())
    moved = int((ref["moved"] & ref["choice"]).sum())
    assert ambiguous <= (1e-3 * choice if rows == 4700 else 0), (ambiguous, choice)
    assert choice > 0 and moved >= 0.2 * choice, (moved, choice)

    # through autograd, (batch, frames, channels) as the training step calls it
    a, b = sed[None].to(DEV).requires_grad_(True), doa[None].to(DEV).requires_grad_(True)
    td = tgt.to(DEV)
    loss, perm = H.seld_loss_pit(a, b, td[None], overlaps, *weights, return_perm=True)
    loss.backward()
    assert not perm.requires_grad and perm.dtype == torch.int32 and tuple(perm.shape) == (rows, C)
    r_sed, r_doa = check((loss.item(), a.grad[0].cpu(), b.grad[0].cpu(), perm.cpu(), None), ref, overlaps, what)
    a2, b2 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    loss2 = H.seld_loss_pit(a2, b2, td[None], overlaps, *weights)          # without perm: a plain scalar, the same bits
    H.backward_from_loss(loss2)
    assert _bits(loss2.reshape(1)).item() == _bits(loss.reshape(1)).item()
    assert torch.equal(_bits(a2.grad), _bits(a.grad)) and torch.equal(_bits(b2.grad), _bits(b.grad))
    l3, parts3, perm3 = H.seld_loss_pit_parts(a.detach(), b.detach(), td[None], overlaps, *weights)
    assert _bits(l3.reshape(1)).item() == _bits(loss.reshape(1)).item() and torch.equal(perm3, perm)

    # the C ABI, with guard elements behind all five outputs: the same bits
    a, b = a.detach()[0], b.detach()[0]
    out = c_abi(a, b, td, rows, C, overlaps, weights)
    assert _bits(out["loss"][0]).item() == _bits(loss.reshape(1)).item()
    assert torch.equal(_bits(out["dsed"][0]), _bits(a2.grad.reshape(-1))) and torch.equal(_bits(out["ddoa"][0]), _bits(b2.grad.reshape(-1)))
    assert torch.equal(out["perm"][0].cpu(), perm.reshape(-1).cpu())
    assert torch.equal(_bits(out["parts"][0]), _bits(parts3))
    parts = tuple(out["parts"][0].tolist())
    check((out["loss"][0].item(), out["dsed"][0].cpu().view(rows, -1), out["ddoa"][0].cpu().view(rows, -1),
           out["perm"][0].cpu().view(rows, C), parts), ref, overlaps, what + " (C ABI)")
    # forward only: the same loss bits, and nothing else written anywhere
    idle = [torch.full((k,), SENTINEL, device=DEV) for k in (sed.numel(), doa.numel(), rows * C, 2)]
    fwd = c_abi(a, b, td, rows, C, overlaps, weights, grads=False, perm=False, parts=False)
    assert _bits(fwd["loss"][0]).item() == _bits(loss.reshape(1)).item()
    assert all(_guards_intact(t, 0) for t in idle)
    print(f"\n{what} error/bound: dsed {r_sed:.3f} | ddoa {r_doa:.3f} | loss "
          f"{abs(loss.item() - ref['loss']) / (1e-5 * max(1.0, abs(ref['loss']))):.3f} | parts sum "
          f"{abs(parts[0] + parts[1] - loss.item()) / (1e-5 * max(1.0, abs(ref['loss']))):.3f} | cells with a choice {choice}, "
          f"moved {moved}, ambiguous {ambiguous}")


# ======================================================================================================================
# 2. exact ties
# ======================================================================================================================
def _one_cell(sed, doa, t_sed, t_doa):
    flat = lambda rows: [v for row in rows for v in row]
    return (torch.tensor([sed], dtype=torch.float32), torch.tensor([flat(doa)], dtype=torch.float32),
            torch.tensor([t_sed + flat(t_doa)], dtype=torch.float32))


TIES = {
    # prediction slots 0 and 1 bit-identical, targets 0 and 1 active and different: indices 0 and 2 cost the same
    "slots 0 = 1": (_one_cell([0.7, 0.7, 0.1], [[0.3, -0.2, 0.5]] * 2 + [[0.0, 0.1, 0.0]], [1.0, 1.0, 0.0],
                              [[0.5, 0.25, -0.75], [-0.5, 0.5, 0.125], [0.0, 0.0, 0.0]]), 0, (0, 2)),
    # the same predictions in slots 0 and 1, slot 2's on target 0, all targets active: 3 = (1,2,0) and 5 = (2,1,0) tie
    # below every other index
    "slots 0 = 1, slot 2 on target 0": (_one_cell([0.7, 0.7, 0.9], [[-0.4, 0.6, 0.2]] * 2 + [[0.5, 0.25, -0.75]],
                                                  [1.0, 1.0, 1.0],
                                                  [[0.5, 0.25, -0.75], [-0.5, 0.5, 0.125], [-0.375, 0.75, 0.25]]), 3, (3, 5)),
    "all-zero target": (_one_cell([0.2, 0.6, 0.4], [[0.3, -0.2, 0.5], [0.1, 0.9, -0.3], [-0.6, 0.2, 0.0]], [0.0] * 3,
                                  [[0.0] * 3] * 3), 0, (0, 1, 2, 3, 4, 5)),
}


@pytest.mark.parametrize("name", list(TIES))
def test_ties_go_to_the_lowest_index(name):
    H = pkg().hip_ops
    (sed, doa, tgt), want, tied = TIES[name]
    ref = R.pit_reference(sed, doa, tgt, 1, 3)
    costs = ref["costs"][0, 0]
    # the case is what it claims to be: the tied indices are the minimum (in fp64 to rounding), every other one is above
    assert all(abs(float(costs[k] - costs[want])) <= 1e-15 for k in tied)
    assert all(float(costs[k]) > float(costs[want]) + 1e-6 for k in range(6) if k not in tied)
    loss, parts, perm = H.seld_loss_pit_parts(sed.to(DEV), doa.to(DEV), tgt.to(DEV), 3)
    assert perm.cpu().tolist() == [[want]], (name, perm.cpu().tolist())
    assert abs(loss.item() - float(costs[want])) <= 1e-5 * max(1.0, float(costs[want]))


# ======================================================================================================================
# 3. bit-level properties
# ======================================================================================================================
def test_target_slot_order_does_not_change_a_bit():
    """Every cell's target slots permuted at random: the same loss bits, the same gradient tensors."""
    H = pkg().hip_ops
    shape = (37, 14, 3)
    (sed, doa, tgt), ref = case(shape, WEIGHTS[0])
    assert not ref["ambiguous"].any()
    order = R.random_orders(*shape, torch.Generator().manual_seed(11))
    assert int((order != torch.arange(3)).any(-1).sum()) > 37 * 14 // 2
    runs = []
    for t in (tgt, R.permute_target(tgt, 14, 3, order)):
        a, b = sed.to(DEV).requires_grad_(True), doa.to(DEV).requires_grad_(True)
        loss = H.seld_loss_pit(a, b, t.to(DEV), 3)
        loss.backward()
        runs.append((_bits(loss.reshape(1)).item(), _bits(a.grad), _bits(b.grad)))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_one_slot_gives_the_plain_kernels_gradients_bit_for_bit():
    """overlaps = 1 on the same data viewed as C * O classes: dsed and ddoa of seld_loss_fwd_bwd, perm all zero."""
    H = pkg().hip_ops
    for weights in WEIGHTS:
        (sed, doa, tgt), _ = case((37, 14, 3), weights)
        grads = []
        for fn in (lambda a, b, t: H.seld_loss(a, b, t, *weights), lambda a, b, t: H.seld_loss_pit(a, b, t, 1, *weights, return_perm=True)):
            a, b = sed.to(DEV).requires_grad_(True), doa.to(DEV).requires_grad_(True)
            out = fn(a, b, tgt.to(DEV))
            loss, perm = out if isinstance(out, tuple) else (out, None)
            loss.backward()
            grads.append((loss.item(), _bits(a.grad), _bits(b.grad), perm))
        assert torch.equal(grads[0][1], grads[1][1]) and torch.equal(grads[0][2], grads[1][2])
        assert abs(grads[0][0] - grads[1][0]) <= 1e-5 * max(1.0, abs(grads[0][0]))
        assert tuple(grads[1][3].shape) == (37, 42) and not grads[1][3].any()


# ======================================================================================================================
# 4. edge values
# ======================================================================================================================
def test_edge_values():
    """sed in {0, 1, 1e-30, 1 - 2^-24} against target 0 and target 1, and a DOA at +-1 against -+1, each in a cell of
    its own whose three target slots are identical, so that the pairing cannot move the value away from its target."""
    H = pkg().hip_ops
    rows, C, overlaps = 2, 14, 3
    sed, doa, tgt = (t.clone() for t in R.pit_inputs(rows, C, overlaps, seed=77))
    s3, d3 = sed.view(rows, C, 3), doa.view(rows, C, 3, 3)
    ts, td = tgt[:, :C * 3].view(rows, C, 3), tgt[:, C * 3:].view(rows, C, 3, 3)
    hand = [(s, t) for s in (0.0, 1.0, 1e-30, 1.0 - U) for t in (0.0, 1.0)]
    for i, (s, t) in enumerate(hand):
        r, c = divmod(i, C)
        s3[r, c, 0] = s
        ts[r, c, :] = t
        td[r, c, :, :] = torch.tensor([0.25, -0.5, 0.75]) * t
    for i, sign in ((len(hand), 1.0), (len(hand) + 1, -1.0)):
        r, c = divmod(i, C)
        ts[r, c, :] = 1.0
        td[r, c, :, :] = -sign * torch.tensor([1.0, -1.0, 1.0])
        d3[r, c, 0, :] = sign * torch.tensor([1.0, -1.0, 1.0])
    ref = R.pit_reference(sed, doa, tgt, C, overlaps)
    assert not ref["ambiguous"].any() and not ref["perm"].view(-1)[:len(hand) + 2].any()
    assert float(ref["dsed"].abs().max()) > 1e8          # sed = 0 against target 1: the 1e-12 denominator
    a, b = sed.to(DEV).requires_grad_(True), doa.to(DEV).requires_grad_(True)
    loss, perm = H.seld_loss_pit(a, b, tgt.to(DEV), overlaps, return_perm=True)
    loss.backward()
    assert math.isfinite(loss.item()) and bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all())
    r_sed, r_doa = check((loss.item(), a.grad.cpu(), b.grad.cpu(), perm.cpu(), None), ref, overlaps, "edge values")
    assert not perm.cpu().view(-1)[:len(hand) + 2].any()
    print(f"\nedge values error/bound: dsed {r_sed:.3f} | ddoa {r_doa:.3f}")


# ======================================================================================================================
# 5. refusals
# ======================================================================================================================
def test_error_codes():
    H, L = pkg().hip_ops, pkg()._lib
    sed, doa = torch.full((2, 8), 0.5, device=DEV), torch.zeros(2, 24, device=DEV)
    tgt, loss = torch.zeros(2, 32, device=DEV), torch.full((1,), SENTINEL, device=DEV)

    def call(rows=2, classes=2, overlaps=4, loss_=loss):
        return L.lib().seld_loss_pit_fwd_bwd(L.ptr(sed), L.ptr(doa), L.ptr(tgt), rows, classes, overlaps, 1.0, 5.0, L.ptr(loss_),
                                             None, None, None, None, L.current_stream())
    assert call(overlaps=4) == -4                                   # SELD_EUNSUPPORTED
    assert call(rows=0, classes=4, overlaps=2) == -1                # SELD_EINVAL
    assert call(classes=4, overlaps=2, loss_=None) == -1
    assert call(classes=0, overlaps=2) == -1 and call(classes=4, overlaps=0) == -1
    torch.cuda.synchronize()
    assert loss.item() == SENTINEL                                  # refused before anything was written
    with pytest.raises(L.SeldHipError):
        H.seld_loss_pit(sed, doa, torch.zeros(2, 33, device=DEV), 2)         # target width
    with pytest.raises(L.SeldHipError):
        H.seld_loss_pit(sed, doa, tgt, 3)                                    # 8 outputs are no multiple of 3 slots
    with pytest.raises(L.SeldHipError):
        H.seld_loss_pit(sed, doa, tgt, 4)                                    # SELD_EUNSUPPORTED from the library
    assert call(classes=4, overlaps=2) == 0


# ======================================================================================================================
# 6. the training step
# ======================================================================================================================
TINY = next(c for c in MODEL_CASES if c["name"] == "tiny_DQ")
N_SED = 42


def swapped_targets():
    """Two (B, T/8, 168) targets with two events of class 3 in every frame and nothing else: the same two events, in
    slots (0, 1) and in slots (1, 0)."""
    B, frames = TINY["B"], TINY["time_dim"] // 8
    n = torch.arange(B * frames, dtype=torch.float32).view(B, frames, 1)
    ev = [torch.cat((0.8 * torch.sin(0.3 * n + p), 0.7 * torch.cos(0.2 * n + p), 0.5 * torch.sin(0.5 * n - p)), 2) for p in (0.0, 2.0)]
    out = []
    for first, second in ((0, 1), (1, 0)):
        t = torch.zeros(B, frames, 4 * N_SED)
        t[:, :, 3 * 3 + 0] = t[:, :, 3 * 3 + 1] = 1.0
        t[:, :, N_SED + (3 * 3 + 0) * 3:N_SED + (3 * 3 + 0) * 3 + 3] = ev[first]
        t[:, :, N_SED + (3 * 3 + 1) * 3:N_SED + (3 * 3 + 1) * 3 + 3] = ev[second]
        out.append(t)
    return out


def _train(steps, mode, pit, target=None):
    """tests/test_gpu_deterministic.py's run on the tiny DQ model, with the loss chosen by `pit`."""
    from tests.golden.cases import train_target
    T, H = pkg().train, pkg().hip_ops
    torch.manual_seed(5)
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    m = build_model(TINY)
    O.closed_form_fill_(list(m.state_dict().items()))
    m = m.to(DEV).train()
    opt = T.FlatAdam(m.parameters(), lr=1e-3)
    x = O.closed_form_input((TINY["B"], TINY["input_channels"], TINY["freq_dim"], TINY["time_dim"])).to(DEV)
    target = (train_target(TINY) if target is None else target).to(DEV)
    losses = []
    if mode == "graph":
        runner = T.GraphedTrainStep(m, opt, x, target, N_SED, 1.0, 5.0, warmup=1, pit_overlaps=pit)
        for _ in range(steps - 1):
            losses.append(float(runner().item()))
    else:
        for _ in range(steps):
            opt.zero_grad()
            sed, doa = m(x)
            loss = T.seld_loss_fn(sed, doa, target, N_SED, 1.0, 5.0, pit_overlaps=pit)
            loss.backward()
            opt.step()
            losses.append(float(loss.item()))
    torch.cuda.synchronize()
    return losses, opt.flat_param.detach().clone(), {k: v.clone() for k, v in m.state_dict().items() if "running" in k}


def test_recorded_pit_step_matches_eager(seld_env):
    """One warm-up step and three replays of GraphedTrainStep(pit_overlaps=3) against four eager steps, deterministic
    mode, at the tolerances tests/test_gpu_deterministic.py holds the plain loss's recorded step to."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    target = swapped_targets()[1]
    le, pe, re_ = _train(4, "eager", 3, target)
    lg, pg, rg = _train(4, "graph", 3, target)
    assert len(lg) == 3 and np.allclose(lg, le[1:], rtol=1e-6, atol=0), (lg, le)
    scale = float(pe.abs().max())
    assert float((pg - pe).abs().max()) <= 1e-6 * scale, float((pg - pe).abs().max())
    for k in re_:
        assert torch.allclose(rg[k], re_[k], rtol=1e-6, atol=1e-7 * float(re_[k].abs().max()) + 1e-12), k


def test_pit_step_does_not_see_the_slot_order(seld_env):
    """One step on two same-class events given in slots (0, 1) and in slots (1, 0): the plain loss trains two different
    models, the permutation-invariant one the same model bit for bit, which therefore differs from the plain one."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    ta, tb = swapped_targets()
    (la, pa, _), (lb, pb, _) = _train(1, "eager", 3, ta), _train(1, "eager", 3, tb)
    (ma, qa, _), (mb, qb, _) = _train(1, "eager", 0, ta), _train(1, "eager", 0, tb)
    assert la == lb and torch.equal(pa, pb)
    assert not torch.equal(qa, qb)
    assert not torch.equal(pa, qa) or not torch.equal(pb, qb)
    assert la[0] <= min(ma[0], mb[0]) * (1 + 1e-6), (la, ma, mb)


def test_pit_step_launches_what_the_plain_step_launches():
    """torch.profiler on one eager dp_train_step with the permutation-invariant loss and one with the plain loss, both
    counted here: the same number of kernels, no kernel outside this library that the plain step does not launch as well
    (on this 16-wide model autograd adds 21 gradients with ATen's add under either loss; tests/test_gpu_launches.py holds
    the config-3 widths to none at all), and the only name that changes is the loss kernel's."""
    import functools
    from torch.profiler import ProfilerActivity, profile
    from tests.golden.cases import train_target
    T, DP = pkg().train, pkg().dp
    torch.manual_seed(5)
    m = build_model(TINY).to(DEV).train()
    opt = T.FlatAdam(m.parameters(), lr=1e-4)
    x = O.closed_form_input((TINY["B"], TINY["input_channels"], TINY["freq_dim"], TINY["time_dim"])).to(DEV)
    target = train_target(TINY).to(DEV)
    sync = DP.BucketedGradSync(opt, m)
    counts = {}
    for pit in (0, 3):
        loss_fn = functools.partial(T.seld_loss_fn, pit_overlaps=pit) if pit else T.seld_loss_fn
        step = lambda: DP.dp_train_step(m, opt, sync, x, target, N_SED, loss_fn)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        counts[pit] = collections.Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    foreign = {pit: {k: v for k, v in names.items() if "seld::" not in k} for pit, names in counts.items()}
    print("\nkernels per step: plain", sum(counts[0].values()), "pit", sum(counts[3].values()), "foreign", foreign)
    assert sum(counts[3].values()) == sum(counts[0].values())
    assert foreign[3] == foreign[0], foreign
    changed = {k for k in set(counts[0]) | set(counts[3]) if counts[0][k] != counts[3][k]}
    assert len(changed) == 2 and all("loss" in k for k in changed) and any("loss_pit_kernel" in k for k in changed), changed


# ======================================================================================================================
# 7. a whole run
# ======================================================================================================================
def test_main_with_pit_loss_resident_and_recorded(tmp_path):
    """train.main with --pit_loss on the device-resident loader with recorded steps (pickled arrays: the resident loader
    does not read --synthetic data): three steps, then the validation pass with the same loss."""
    from tests.test_gpu_train_loader import MODEL_FLAGS, write_pickles
    T, H = pkg().train, pkg().hip_ops
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    flags = dict(MODEL_FLAGS, **write_pickles(tmp_path, 5), results_path=os.path.join(str(tmp_path), "res"),
                 checkpoint_dir=os.path.join(str(tmp_path), "ck"), batch_size=2, epochs=1, min_n_epochs=1, max_steps=3,
                 resident_loader="True", graph_step="True", pit_loss="True")
    history = []
    state = T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]), history=history)
    torch.cuda.synchronize()
    assert state["step"] == 3 and len(history) == 1
    _, train_loss, val_loss = history[0]
    assert math.isfinite(train_loss) and math.isfinite(val_loss) and train_loss > 0 and val_loss > 0
