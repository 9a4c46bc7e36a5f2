"""The optimiser's extras (csrc/optim.hip: grad_norm_kernel, adam_ex_kernel, adam_ex_state_kernel) against the fp64
chain of tests/optim_ref.py, and train.FlatAdam with them on: eager, recorded, data parallel.

Both sides start from the same fp32 inputs and the same fp32-rounded hyper-parameters.  u = 2^-24 (half an fp32 ulp).

Norm.  The kernel forms x = fl32(g * grad_scale) as the reference does, squares and sums in fp64 and rounds once, after
the square root.  An fp32 value squared is exact in fp64 (48 bits); a sum of n positive fp64 terms and its square root are
off by at most (n + 1) 2^-53 relative, below 2^-32 for n < 2^21; the cast to fp32 adds u.  So
         |clip[0] - ref| <= 2u ref                         (1 rounding and the fp64 dust; 2u leaves a whole rounding spare)
The coefficient is fl(max_norm / fl(clip[0] + 1e-6f)), clamped: the norm's own u (times norm / (norm + 1e-6) <= 1), the
sum's u and the quotient's u, 3u to first order;
         |clip[1] - ref| <= 4u ref,   ref = min(1, max_norm / (ref_norm + 1e-6f)) in fp64.
A clamped coefficient is exactly 1 on both sides, or within 4u of it on one.

Update.  With c the coefficient as fp32 holds it and k = 1 with a coefficient, 0 without, g' = fl(fl(g grad_scale) c)
carries k roundings more than adam_kernel's gradient.  On top of the bounds of tests/test_gpu_train_step.py (mag =
|b1 m0| + |(1 - b1) g'|, tol(step) = u (12 + 4 / bc1 + 2 / bc2)):
         |m - m_ref| <= 4u mag + k u (1 - b1) |g gs c|
         |v - v_ref| <= 6u (b2 v0 + (1 - b2) g'^2) + 2k u (1 - b2) |g gs c| |g'|          (+ one fp32 denormal)
         |p - p_ref| <= (tol + 2k u) (lr / bc1) mag / denom_ref + u |p_ref| + [decoupled] 3u |p0|
  one rounding for the coefficient: u |g gs c| enters m directly, v through the square (twice), and the update through
  m / sqrt(v) (k u from each, 2k u in all).  Decoupled decay: p0 is replaced by fl(p0 fl(1 - fl(lr wd))), two roundings
  for the factor and one for applying it, 3u |p0|; g' gets no decay term.
  The moving average is evaluated as e0 + fl(1 - d) (p - e0), with d = min(decay, fl((1 + step) / (10 + step))); with
  D = |p_ref| + |e0|, the magnitudes of the difference's terms,
         |ema - ema_ref| <= 4u (1 - d) D + [quotient taken] u d D + u |ema_ref| + (1 - d) bound_p
  the difference, 1 - d and the product round once each ((1 - d) D; the fourth u covers second-order terms), the
  quotient's rounding shifts 1 - d by d u, the sum rounds to u |ema_ref|, and p arrives with its own error.  About four
  roundings, as for m.  No credit for cancellation anywhere.

FlatAdam, 5 steps from step 1.  The fp64 chain is given the coefficient the device computed (itself held to the 4u bound
above), and after step t the kernel's buffers are within the SUM over s <= t of the per-step bounds, evaluated on the
chain's state.  Errors carried from step to step do not grow: p carries its own with factor 1 - lr wd, m and v with b1 and
b2, the average with d and (1 - d) of p's; the update reacts to the few u of relative error that m and v carry, which the
summed tol(s) >= 422u of steps 1..5 (bc2 <= 0.005) covers hundreds of times over.

Largest error / bound on the MI355X (printed by the tests; a ratio above 1 is a defect, not a reason to widen):

  norm, all sizes and scales     clip[0] 0.398   clip[1] 0.245

  update variant    p      m      v      ema      largest of the four by step (1, 2, 1000)
  clip              0.948  0.463  0.470  -        0.948  0.836  0.885
  adamw             0.541  0.450  0.450  -        0.493  0.541  0.507
  ema               0.875  0.450  0.450  0.391    0.875  0.830  0.832
  all               0.541  0.463  0.470  0.316    0.522  0.541  0.505

  FlatAdam, 5 steps, summed bounds     p 0.060   m 0.327   v 0.388   ema 0.051   clip[0] 0.262   clip[1] 0.222

As in tests/test_gpu_train_step.py the p column is near 1 by construction where the update is small against p's own
rounding term u |p_ref| (clip and ema draw p ~ 1e-3 N(0,1) and an element just above a power of two uses that term up);
with decay (adamw, all) p ~ N(0,1), the decoupled term 3u |p0| is the budget and about half of it is used.  No per-launch
bound is looser than 10x everywhere, so none was tightened; none had to be widened.  The five-step figures are against sums
of upper bounds, of which independent roundings use 5 to 40 %.
"""
import collections
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import seld_oracle as O
from tests import optim_ref as R
from tests.golden.cases import MODEL_CASES, train_target
from tests.helpers import build_model, pkg
from tests.test_gpu_train_step import (ADAM_NS, B1, B2, BASE, DENORM, DEV, DRAWS, U, _bits, _guarded, _guards_intact, _lr_bits,
                                       _ratio, _state, adam_hyper, adam_inputs, f32)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = next(c for c in MODEL_CASES if c["name"] == "tiny_DQ")      # the smallest model case (12040 parameters)


# ======================================================================================================================
# the norm
# ======================================================================================================================
NORM_GRID = 256                                 # NORM_BLOCKS of csrc/optim.hip: the cap of the grid
NORM_UNROLL = 16                                # NORM_UNROLL: elements a thread loads per round
# the last two: one thread takes a second element (same round of loads), one thread takes a second round
NORM_NS = (1, 255, 256, 257, 4099, NORM_GRID * 256 + 1, NORM_GRID * 256 * NORM_UNROLL + 1)
NORM_SCALES = (1.0, 0.25, 1.0 / 3.0)
_norm_cases = {}


def norm_case(n, gs):
    """(gradient, fp64 norm) of a size and a grad_scale, made once and shared (read only).  The gradient is
    adam_inputs': N(0,1) 10^k, k in -12..3, about 5 % exact zeros."""
    if (n, gs) not in _norm_cases:
        g = adam_inputs(n, 2, 0.0, seed=31 * n + 7)[1]
        _norm_cases[(n, gs)] = (g, R.grad_norm(g, f32(gs)))
    return _norm_cases[(n, gs)]


def norm_run(g, gs, max_norm, clip0=(0.0, 0.0, 0.0, 0.0)):
    """One seld_grad_norm launch on guarded buffers; the four floats, on the host."""
    H = pkg().hip_ops
    gv, gbuf = _guarded(g)
    cv, cbuf = _guarded(torch.tensor(clip0, dtype=torch.float32))
    H.grad_norm(gv, f32(gs), f32(max_norm), cv)
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, g.numel()) and _guards_intact(cbuf, 4), f"elements behind a buffer were written (n = {g.numel()})"
    assert torch.equal(_bits(gv), _bits(g)), "the gradient buffer was written"
    return cv.cpu()


def norm_ratios(clip, ref_norm, max_norm):
    ref_c = R.clip_coefficient(ref_norm, f32(max_norm))
    r0 = abs(float(clip[0]) - ref_norm) / (2 * U * ref_norm) if ref_norm else float(clip[0] != 0)
    r1 = abs(float(clip[1]) - ref_c) / (4 * U * ref_c)
    return r0, r1, ref_c


def test_grad_norm_against_fp64():
    worst = [0.0, 0.0]
    for n in NORM_NS:
        for gs in NORM_SCALES:
            g, ref = norm_case(n, gs)
            for max_norm in (1.0, 1e6):                     # clipped (all but the tiniest norms) and not
                clip = norm_run(g, gs, max_norm)
                r0, r1, ref_c = norm_ratios(clip, ref, max_norm)
                what = f"grad_norm n={n} gs={gs:g} max_norm={max_norm:g}"
                assert r0 <= 1.0, f"{what}: norm {float(clip[0])!r}, fp64 reference {ref!r}, error / bound = {r0:.3f}"
                assert r1 <= 1.0, f"{what}: coefficient {float(clip[1])!r}, fp64 reference {ref_c!r}, error / bound = {r1:.3f}"
                assert float(clip[2]) == float(clip[0]) and float(clip[3]) == float(float(clip[1]) < 1.0), (what, clip)
                worst = [max(worst[0], r0), max(worst[1], r1)]
    assert any(R.clip_coefficient(norm_case(n, 1.0)[1], 1e6) == 1.0 for n in NORM_NS)
    assert any(R.clip_coefficient(norm_case(n, 1.0)[1], 1.0) < 1.0 for n in NORM_NS)
    print(f"\ngrad_norm error/bound: clip[0] {worst[0]:.3f} | clip[1] {worst[1]:.3f}")


def test_grad_norm_of_zeros_is_zero_and_one():
    for n in (1, 257):
        clip = norm_run(torch.zeros(n), 0.25, 1.0)
        assert clip.tolist() == [0.0, 1.0, 0.0, 0.0]


def test_grad_norm_of_huge_elements_is_finite():
    """Eight elements of 1e30: the squares overflow fp32 (an fp32 accumulator gives inf), the norm 2.83e30 does not."""
    g = torch.full((8,), 1e30)
    clip = norm_run(g, 1.0, 1.0)
    ref = R.grad_norm(g, 1.0)
    assert np.isfinite(float(clip[0])) and abs(ref - 8 ** 0.5 * float(np.float32(1e30))) <= 1e-15 * ref
    r0, r1, _ = norm_ratios(clip, ref, 1.0)
    assert r0 <= 1.0 and r1 <= 1.0, (clip, ref, r0, r1)
    assert float(clip[1]) > 0.0 and float(clip[3]) == 1.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_grad_norm_propagates_non_finite_as_torch_does(bad):
    g = torch.tensor([1.0, bad, -2.0, 0.5])
    clip = norm_run(g, 1.0, 1.0)
    q = torch.nn.Parameter(torch.zeros(4))
    q.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([q], 1.0)
    coef = q.grad[0]                                       # what torch multiplied the gradient 1.0 by
    assert _bits(clip[0:1]).item() == _bits(total.reshape(1).float()).item() or (np.isnan(float(clip[0])) and bool(torch.isnan(total)))
    assert float(clip[1]) == float(coef) or (np.isnan(float(clip[1])) and bool(torch.isnan(coef)))
    if np.isnan(bad):                                      # a NaN norm is neither kept as the largest nor counted as clipped
        assert float(clip[2]) == 0.0 and float(clip[3]) == 0.0
    else:
        assert float(clip[1]) == 0.0 and float(clip[2]) == float("inf") and float(clip[3]) == 1.0


def test_grad_norm_twice_gives_the_same_bits():
    n = NORM_NS[-1]
    g, _ = norm_case(n, 1.0 / 3.0)
    a, b = norm_run(g, 1.0 / 3.0, 1.0), norm_run(g, 1.0 / 3.0, 1.0)
    assert torch.equal(_bits(a), _bits(b)), (a, b)


def test_grad_norm_keeps_the_largest_norm_and_counts_clipped_steps():
    """Norms 5, 10 and 0.5 against max_norm 1: the largest is 10, two of the three were clipped; the host's zeroes start it."""
    H = pkg().hip_ops
    clip = torch.zeros(4, device=DEV)
    for pair in ((3.0, 4.0), (6.0, 8.0), (0.3, 0.4)):
        H.grad_norm(torch.tensor(pair, device=DEV), 1.0, 1.0, clip)
    torch.cuda.synchronize()
    got = clip.cpu().tolist()
    assert got[2] == 10.0 and got[3] == 2.0 and abs(got[0] - 0.5) <= 2 * U * 0.5 and got[1] == 1.0, got


def test_grad_norm_refusals_and_the_empty_buffer():
    H, L = pkg().hip_ops, pkg()._lib
    g, clip = torch.ones(8, device=DEV), torch.full((4,), 7.0, device=DEV)
    st = L.current_stream()
    for args in ((None, 8, 1.0, 1.0, L.ptr(clip)), (L.ptr(g), 8, 1.0, 1.0, None), (L.ptr(g), -1, 1.0, 1.0, L.ptr(clip)),
                 (L.ptr(g), 8, 1.0, 0.0, L.ptr(clip)), (L.ptr(g), 8, 1.0, -1.0, L.ptr(clip)),
                 (L.ptr(g), 8, 1.0, float("nan"), L.ptr(clip))):
        rc = L.lib().seld_grad_norm(*args, st)
        assert rc == -1 and L._ERRORS[rc] == "SELD_EINVAL", args
    torch.cuda.synchronize()
    assert clip.cpu().tolist() == [7.0] * 4
    with pytest.raises(L.SeldHipError):
        H.grad_norm(g, 1.0, 0.0, clip)
    with pytest.raises(L.SeldHipError):
        H.grad_norm(g.cpu(), 1.0, 1.0, clip)
    clip.zero_()
    assert L.lib().seld_grad_norm(None, 0, 1.0, 2.0, L.ptr(clip), st) == L.SELD_OK
    torch.cuda.synchronize()
    assert clip.cpu().tolist() == [0.0, 1.0, 0.0, 0.0]


# ======================================================================================================================
# the update, per element
# ======================================================================================================================
EX_STEPS = (1, 2, 1000)
COEF, DECAY = f32(0.37), f32(0.999)
EX_VARIANTS = {
    "clip": dict(coef=COEF),
    "adamw": dict(wd=1e-2, decoupled=True),
    "ema": dict(ema_decay=DECAY),
    "all": dict(coef=COEF, wd=1e-2, decoupled=True, ema_decay=DECAY),
}


def ex_inputs(n, step, wd, seed, with_ema):
    """adam_inputs' (p, g, m, v) and an average a percent and 1e-4 away from p (None without one)."""
    p, g, m, v = adam_inputs(n, step, wd, seed)
    if not with_ema:
        return p, g, m, v, None
    gen = torch.Generator().manual_seed(seed + 1)
    return p, g, m, v, p * (1.0 + 0.01 * torch.randn(n, generator=gen)) + 1e-4 * torch.randn(n, generator=gen)


def ex_reference(inputs, step, lr, eps, wd, gs, coef=None, decoupled=False, ema_decay=0.0):
    """fp64 (p, m, v, ema) after the step and the componentwise bounds of the module docstring (ema: None, None without one).
    `inputs` may be fp32 or fp64 tensors."""
    p, g, m, v = (t.double() for t in inputs[:4])
    ema = None if inputs[4] is None else inputs[4].double()
    k, c = (0, 1.0) if coef is None else (1, coef)
    pr, mr, vr, er = R.adam_ex_step(p, g, m, v, ema, step, lr=lr, b1=B1, b2=B2, eps=eps, weight_decay=wd, decoupled=decoupled,
                                    grad_scale=gs, coef=c, ema_decay=ema_decay)
    gc = (g * gs) * c
    gp = gc if decoupled else gc + wd * p
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    mag = (B1 * m).abs() + ((1.0 - B1) * gp).abs()
    bound_m = 4 * U * mag + k * U * (1.0 - B1) * gc.abs()
    bound_v = 6 * U * (B2 * v + (1.0 - B2) * gp * gp) + 2 * k * U * (1.0 - B2) * gc.abs() * gp.abs() + DENORM
    denom = (vr / bc2).sqrt() + eps
    tol = U * (12.0 + 4.0 / bc1 + 2.0 / bc2 + 2 * k)
    bound_p = tol * (lr / bc1) * mag / denom + U * pr.abs() + (3 * U * p.abs() if decoupled else 0.0)
    bound_e = None
    if ema is not None:
        d = R.ema_decay_at(step, ema_decay)
        D = pr.abs() + ema.abs()
        quotient = U * d * D if (1.0 + step) / (10.0 + step) < ema_decay else 0.0
        bound_e = 4 * U * (1.0 - d) * D + quotient + U * er.abs() + (1.0 - d) * bound_p
    return (pr, mr, vr, er), (bound_p, bound_m, bound_v, bound_e)


def ex_check(got, refs, bounds, what):
    """Asserts the bounds; the largest error / bound of (p, m, v, ema), 0.0 for an absent average."""
    worst = []
    for name, x, r, b in zip(("p", "m", "v", "ema"), got, refs, bounds):
        if r is None:
            worst.append(0.0)
            continue
        ratio = _ratio((x.double() - r).abs(), b)
        i = int(ratio.argmax())
        worst.append(float(ratio[i]))
        assert ratio[i] <= 1.0, (f"{what}: {name}[{i}] = {float(x[i])!r}, fp64 reference {float(r[i])!r}, error / bound = "
                                 f"{float(ratio[i]):.3f}")
    return worst


def ex_run(inputs, launch, coef=None):
    """Upload (p, g, m, v, ema) with guard elements and the coefficient as clip[1], call launch(p, g, m, v, ema, clip) on the
    views, return (p, m, v, ema) from the device.  The gradient and the clip buffer must come back as they went."""
    views, bufs = zip(*((None, None) if t is None else _guarded(t) for t in inputs))
    clip0 = None if coef is None else torch.tensor([5.0, coef, 6.0, 7.0], dtype=torch.float32)
    clip, clip_buf = (None, None) if coef is None else _guarded(clip0)
    launch(*views, clip)
    torch.cuda.synchronize()
    n = inputs[0].numel()
    for name, buf in zip(("p", "g", "m", "v", "ema"), bufs):
        assert buf is None or _guards_intact(buf, n), f"{name}: the elements behind the buffer were written (n = {n})"
    assert torch.equal(_bits(views[1]), _bits(inputs[1])), "the gradient buffer was written"
    if coef is not None:
        assert _guards_intact(clip_buf, 4) and torch.equal(_bits(clip), _bits(clip0)), "the clip buffer was written"
    return tuple(None if views[i] is None else views[i].cpu() for i in (0, 2, 3, 4))


def ex_launch(H, step, hyper, coef=None, decoupled=False, ema_decay=0.0, state=None):
    """The launch of a variant for ex_run: the host entry at `step`, or the state entry with `state`."""
    kw = dict(beta1=B1, beta2=B2, eps=hyper["eps"], weight_decay=hyper["wd"], grad_scale=hyper["gs"], decoupled=decoupled,
              ema_decay=ema_decay)
    if state is not None:
        return lambda p, g, m, v, ema, clip: H.adam_flat_step_state_ex(p, g, m, v, state, clip=clip, ema=ema, **kw)
    return lambda p, g, m, v, ema, clip: H.adam_flat_step_ex(p, g, m, v, step, lr=hyper["lr"], clip=clip, ema=ema, **kw)


@pytest.mark.parametrize("variant", list(EX_VARIANTS))
def test_adam_ex_per_element(variant):
    H = pkg().hip_ops
    var = dict(EX_VARIANTS[variant])
    extras = dict(coef=var.pop("coef", None), decoupled=var.pop("decoupled", False), ema_decay=var.pop("ema_decay", 0.0))
    hyper = adam_hyper(gs=0.25, **var)
    worst = {s: [0.0] * 4 for s in EX_STEPS}
    for n in ADAM_NS:
        for step in EX_STEPS:
            inputs = ex_inputs(n, step, hyper["wd"], seed=2000 * n + step, with_ema=extras["ema_decay"] > 0)
            got = ex_run(inputs, ex_launch(H, step, hyper, **extras), extras["coef"])
            refs, bounds = ex_reference(inputs, step, **hyper, **extras)
            w = ex_check(got, refs, bounds, f"adam_ex[{variant}] n={n} step={step}")
            worst[step] = [max(a, b) for a, b in zip(worst[step], w)]
    print(f"\nadam_ex[{variant}] error/bound: " + " | ".join(
        f"{name} {max(w[i] for w in worst.values()):.3f}" for i, name in enumerate(("p", "m", "v", "ema"))) +
        " | by step " + " ".join(f"{s}:{max(worst[s]):.3f}" for s in EX_STEPS))


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_ex_idle_elements_do_not_move(step):
    """Zero gradient, zero moments, no decay, the average on the weight: every buffer keeps its bits, with the
    coefficient, the decoupled form (a factor of exactly 1) and the average all on."""
    H = pkg().hip_ops
    n = 257
    p = torch.randn(n, generator=torch.Generator().manual_seed(9))
    zero = torch.zeros(n)
    inputs = (p, zero, zero, zero, p.clone())
    hyper = adam_hyper(gs=0.25)
    got = ex_run(inputs, ex_launch(H, step, hyper, coef=COEF, decoupled=True, ema_decay=DECAY), COEF)
    for name, x, x0 in zip(("p", "m", "v", "ema"), got, (p, zero, zero, p)):
        assert torch.equal(_bits(x), _bits(x0)), f"{name} moved"


EXTRAS_OFF = {"default": dict(), "gs=0.25,wd=1e-2": dict(gs=0.25, wd=1e-2), "eps=1e-3": dict(eps=1e-3)}


@pytest.mark.parametrize("variant", list(EXTRAS_OFF))
def test_extras_off_is_the_old_kernel(variant):
    """clip NULL, ema NULL, decoupled 0: seld_adam_flat_ex is seld_adam_flat and seld_adam_flat_state_ex is
    seld_adam_flat_state, bit for bit, the advance of state[0] included."""
    H = pkg().hip_ops
    hyper = adam_hyper(**EXTRAS_OFF[variant])
    kw = dict(beta1=B1, beta2=B2, eps=hyper["eps"], weight_decay=hyper["wd"], grad_scale=hyper["gs"])
    for n in ADAM_NS:
        for step in EX_STEPS:
            inputs = ex_inputs(n, step, hyper["wd"], seed=3000 * n + step, with_ema=False)
            old = ex_run(inputs, lambda p, g, m, v, ema, clip: H.adam_flat_step(p, g, m, v, step, lr=hyper["lr"], **kw))
            new = ex_run(inputs, ex_launch(H, step, hyper))
            s_old, s_new = _state(step, hyper["lr"]), _state(step, hyper["lr"])
            old_s = ex_run(inputs, lambda p, g, m, v, ema, clip: H.adam_flat_step_state(p, g, m, v, s_old, **kw))
            new_s = ex_run(inputs, ex_launch(H, step, hyper, state=s_new))
            for name, a, b, c, d in zip("pmv", old, new, old_s, new_s):
                assert torch.equal(_bits(a), _bits(b)), f"{variant} n={n} step={step}: {name} differs from seld_adam_flat"
                assert torch.equal(_bits(c), _bits(d)), f"{variant} n={n} step={step}: {name} differs from seld_adam_flat_state"
                assert torch.equal(_bits(a), _bits(c))
            assert s_new.tolist() == s_old.tolist() == [BASE + DRAWS, step, _lr_bits(hyper["lr"]), DRAWS]


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", [1, 257])
def test_state_entry_is_the_host_entry_with_all_extras(n, step):
    H = pkg().hip_ops
    hyper = adam_hyper(lr=3e-5, wd=1e-2, gs=0.25)
    extras = dict(coef=COEF, decoupled=True, ema_decay=DECAY)
    inputs = ex_inputs(n, step, hyper["wd"], seed=4000 * n + step, with_ema=True)
    host = ex_run(inputs, ex_launch(H, step, hyper, **extras), COEF)
    ex_check(host, *ex_reference(inputs, step, **hyper, **extras), f"adam_ex host entry n={n} step={step}")
    state = _state(step, hyper["lr"], high=0x7FC0FFEE)             # only the low word of state[2] is the learning rate
    dev = ex_run(inputs, ex_launch(H, step, hyper, state=state, **extras), COEF)
    for name, a, b in zip(("p", "m", "v", "ema"), host, dev):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: the state entry differs from the host entry"
    assert state.tolist() == [BASE + DRAWS, step, _lr_bits(hyper["lr"]) | (0x7FC0FFEE << 32), DRAWS]


def test_state_entry_without_elements_still_ends_the_step():
    L = pkg()._lib
    bufs = [torch.full((4,), -1234.5, device=DEV) for _ in range(5)]
    clip = torch.tensor([0.0, 0.5, 0.0, 0.0], device=DEV)
    state = _state(3, 1e-4)
    rc = L.lib().seld_adam_flat_state_ex(*(L.ptr(b) for b in bufs), 0, B1, B2, f32(1e-8), f32(1e-2), 1, 1.0, L.ptr(clip), DECAY,
                                         L.ptr(state), L.current_stream())
    assert rc == L.SELD_OK
    assert L.lib().seld_adam_flat_ex(*(L.ptr(b) for b in bufs), 0, f32(1e-4), B1, B2, f32(1e-8), 0.0, 0, 1, 1.0, None, 0.0,
                                     L.current_stream()) == L.SELD_OK
    # refusals: a step below 1, a decay outside [0, 1) with an average, a missing state
    assert L.lib().seld_adam_flat_ex(*(L.ptr(b) for b in bufs), 4, f32(1e-4), B1, B2, f32(1e-8), 0.0, 0, 0, 1.0, None, 0.0,
                                     L.current_stream()) == -1
    assert L.lib().seld_adam_flat_ex(*(L.ptr(b) for b in bufs), 4, f32(1e-4), B1, B2, f32(1e-8), 0.0, 0, 1, 1.0, None, 1.0,
                                     L.current_stream()) == -1
    assert L.lib().seld_adam_flat_state_ex(*(L.ptr(b) for b in bufs), 4, B1, B2, f32(1e-8), 0.0, 0, 1.0, None, 0.5, None,
                                           L.current_stream()) == -1
    torch.cuda.synchronize()
    assert state.tolist() == [BASE + DRAWS, 3, _lr_bits(1e-4), DRAWS]
    for b in bufs:
        assert _guards_intact(b, 0)


# ======================================================================================================================
# train.FlatAdam
# ======================================================================================================================
FA = dict(lr=f32(1e-2), wd=f32(1e-2), eps=f32(1e-8), gs=0.5, max_norm=1.0)
FA_SIZES = ((5,), (8, 8), (3, 100))
FA_SCALES = (10.0, 1.0, 0.1, 0.01, 3.0)         # norms of about 350, 35, 3.5, 0.35, 100 times grad_scale 0.5: the fourth is not clipped


def hand_gradient(shape, index, step):
    n = int(np.prod(shape))
    i = torch.arange(n, dtype=torch.float64)
    g = torch.sin(0.37 * i + step + index) * 10.0 ** ((i % 4) - 2) * FA_SCALES[step - 1]
    return g.float().view(shape)


def _flat_adam():
    T = pkg().train
    params = [torch.nn.Parameter((0.5 * torch.cos(0.11 * torch.arange(float(np.prod(s))) + k)).view(s).to(DEV))
              for k, s in enumerate(FA_SIZES)]
    opt = T.FlatAdam(params, lr=FA["lr"], eps=FA["eps"], weight_decay=FA["wd"], decoupled=True, max_grad_norm=FA["max_norm"],
                     ema_decay=DECAY)
    return params, opt


def test_flat_adam_five_steps_within_the_summed_bounds():
    params, opt = _flat_adam()
    n = sum(p.numel() for p in params)
    assert opt.clip is not None and opt.ema is not None and torch.equal(opt.ema, opt.flat_param) and n == 369
    chain = [opt.flat_param.cpu().double(), None, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64),
             opt.ema.cpu().double()]
    total = [torch.zeros(n, dtype=torch.float64) for _ in range(4)]
    worst, worst_clip, norms = [0.0] * 4, [0.0, 0.0], []
    for step in range(1, 6):
        opt.zero_grad()
        for k, p in enumerate(params):
            p.grad.copy_(hand_gradient(p.shape, k, step))
        g = opt.flat_grad.cpu()
        assert torch.equal(g, torch.cat([hand_gradient(s, k, step).reshape(-1) for k, s in enumerate(FA_SIZES)]))
        opt.step(grad_scale=FA["gs"])
        torch.cuda.synchronize()
        clip = opt.clip.cpu()
        ref_norm = R.grad_norm(g, FA["gs"])
        r0, r1, ref_c = norm_ratios(clip, ref_norm, FA["max_norm"])
        assert r0 <= 1.0 and r1 <= 1.0, (step, clip, ref_norm, ref_c)
        assert (ref_c < 1.0) == (step != 4)
        worst_clip = [max(worst_clip[0], r0), max(worst_clip[1], r1)]
        norms.append(float(clip[0]))
        chain[1] = g.double()
        refs, bounds = ex_reference(chain, step, FA["lr"], FA["eps"], FA["wd"], FA["gs"], coef=float(clip[1]), decoupled=True,
                                    ema_decay=DECAY)
        total = [t + b for t, b in zip(total, bounds)]
        got = (opt.flat_param.cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu(), opt.ema.cpu())
        w = ex_check(got, refs, total, f"FlatAdam step {step}")
        worst = [max(a, b) for a, b in zip(worst, w)]
        chain = [refs[0], None, refs[1], refs[2], refs[3]]
    assert opt.step_count == 5
    largest, clipped = opt.clip_stats()
    assert largest == max(norms) and clipped == 4
    assert opt.clip_stats() == (0.0, 0) and opt.clip.cpu()[:2].tolist() == [norms[-1], float(clip[1])]
    print("\nFlatAdam 5 steps error/summed bound: " + " | ".join(f"{k} {v:.3f}" for k, v in zip(("p", "m", "v", "ema"), worst)) +
          f" | clip[0] {worst_clip[0]:.3f} | clip[1] {worst_clip[1]:.3f}")


def test_ema_weights_lends_the_average_and_gives_the_weights_back():
    params, opt = _flat_adam()
    for step in (1, 2):
        opt.zero_grad()
        for k, p in enumerate(params):
            p.grad.copy_(hand_gradient(p.shape, k, step))
        opt.step()
    torch.cuda.synchronize()
    train_bits, ema_bits = _bits(opt.flat_param), _bits(opt.ema)
    assert not torch.equal(train_bits, ema_bits)
    per_param = [_bits(p.detach()) for p in params]
    with opt.ema_weights():
        assert torch.equal(_bits(opt.flat_param), ema_bits) and torch.equal(_bits(opt.ema), train_bits)
        off = 0
        for p in params:                                    # the parameters are views of flat_param
            assert torch.equal(_bits(p.detach()).view(-1), ema_bits[off:off + p.numel()])
            off += p.numel()
        with pytest.raises(RuntimeError):
            opt.step()
    assert torch.equal(_bits(opt.flat_param), train_bits) and torch.equal(_bits(opt.ema), ema_bits)
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("the body raised")
    assert torch.equal(_bits(opt.flat_param), train_bits) and torch.equal(_bits(opt.ema), ema_bits)
    assert all(torch.equal(_bits(p.detach()), b) for p, b in zip(params, per_param))
    opt.ema_reset()
    assert torch.equal(_bits(opt.ema), train_bits)


def _tiny(lr=1e-2, **extras):
    """The tiny model on the device in training mode, its FlatAdam, a batch."""
    T, H = pkg().train, pkg().hip_ops
    torch.manual_seed(5)
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    m = build_model(TINY)
    O.closed_form_fill_(list(m.state_dict().items()))
    m = m.to(DEV).train()
    opt = T.FlatAdam(m.parameters(), lr=lr, **extras)
    x = O.closed_form_input((TINY["B"], TINY["input_channels"], TINY["freq_dim"], TINY["time_dim"])).to(DEV)
    return m, opt, x, train_target(TINY).to(DEV), int(TINY["output_classes"] * 3)


ALL_ON = dict(weight_decay=1e-2, decoupled=True, max_grad_norm=0.05, ema_decay=0.999)


def _eager_steps(m, opt, x, target, n_sed, steps):
    T = pkg().train
    for _ in range(steps):
        opt.zero_grad()
        sed, doa = m(x)
        T.seld_loss_fn(sed, doa, target, n_sed, 1.0, 5.0).backward()
        opt.step()


def test_ema_weights_refresh_the_packed_weight_forms():
    """A forward inside the context computes with the average: it differs from the forward outside and equals that of a
    second model loaded with the average.  The fast-product convolutions cache packed forms of their weights; a context
    that did not mark them stale would compute the outer forward again."""
    m, opt, x, target, n_sed = _tiny(**ALL_ON)
    _eager_steps(m, opt, x, target, n_sed, 3)
    m.eval()
    with torch.no_grad():
        out = [t.clone() for t in m(x)]
        with opt.ema_weights():
            inside = [t.clone() for t in m(x)]
        again = [t.clone() for t in m(x)]
    average = opt.ema_state_dict(m.named_parameters())
    m2 = build_model(TINY)
    m2.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})      # BatchNorm buffers are shared by both weight sets
    with torch.no_grad():
        for name, p in m2.named_parameters():
            p.copy_(average[name].cpu())
    m2 = m2.to(DEV).eval()
    with torch.no_grad():
        loaded = m2(x)
    torch.cuda.synchronize()
    for a, b, c, d in zip(out, inside, again, loaded):
        same, moved = float((b - d).abs().max()), float((b - a).abs().max())
        assert same <= 1e-6, same
        assert moved > 1e-4, moved
        assert torch.equal(a, c)


def test_recorded_steps_equal_eager_steps_with_all_extras(seld_env):
    """Three replays of the recorded step against three eager steps from the same state, SELD_DETERMINISTIC=1, clipping,
    AdamW decay and the average on: parameters, moments, average and the norm of the last step, bit for bit.  The
    recording's warm-up step is undone by training_snapshot / training_restore, average and clip statistics included."""
    T = pkg().train
    seld_env.set("SELD_DETERMINISTIC", "1")
    m, opt, x, target, n_sed = _tiny(lr=1e-3, **ALL_ON)
    _eager_steps(m, opt, x, target, n_sed, 3)
    torch.cuda.synchronize()
    eager = [t.clone() for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.clip)]
    print(f"\ntiny model: gradient norm at step 3 = {float(opt.clip[0]):.4g}, largest {float(opt.clip[2]):.4g}")
    assert float(opt.clip[3]) == 3.0        # max_grad_norm = 0.05 is below the tiny model's gradient norm: every step is clipped

    m, opt, x, target, n_sed = _tiny(lr=1e-3, **ALL_ON)
    snap = T.training_snapshot(m, opt)
    assert "ema" in snap and "clip" in snap
    runner = T.GraphedTrainStep(m, opt, x, target, n_sed, 1.0, 5.0, warmup=1)
    torch.cuda.synchronize()
    assert float(opt.clip[3]) == 1.0 and not torch.equal(opt.ema, snap["ema"])        # the warm-up trained ...
    T.training_restore(m, opt, snap)
    assert opt.clip.cpu().tolist() == [0.0] * 4 and torch.equal(opt.ema, snap["ema"]) and opt.step_count == 0     # ... and left no trace
    for _ in range(3):
        runner()
    torch.cuda.synchronize()
    assert opt.step_count == 3
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "ema", "clip"), eager,
                          (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.clip)):
        assert torch.equal(_bits(a), _bits(b)), (name, float((a - b).abs().max()))


def _launches_of_a_step(extras):
    T, DP = pkg().train, pkg().dp
    case = dict(next(c for c in MODEL_CASES if c["name"] == "c3w_train"), dropout_perc=0.3, spatial_dropout_rate=0.5)
    torch.manual_seed(5)
    m = build_model(case).to(DEV).train()
    opt = T.FlatAdam(m.parameters(), lr=1e-4, **extras)
    x = O.closed_form_input((case["B"], case["input_channels"], case["freq_dim"], case["time_dim"])).to(DEV)
    target = train_target(case).to(DEV)
    sync = DP.BucketedGradSync(opt, m)

    def step():
        DP.dp_train_step(m, opt, sync, x, target, int(case["output_classes"] * 3), T.seld_loss_fn)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return collections.Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)


def test_all_extras_cost_one_launch():
    """The step tests/test_gpu_launches.py counts, with clipping, AdamW decay and the average on: one launch more, the
    norm; the average rides in the update's launch; every launch is this library's."""
    plain, full = _launches_of_a_step({}), _launches_of_a_step(ALL_ON)
    assert sum(full.values()) == sum(plain.values()) + 1, (sum(plain.values()), sum(full.values()), full - plain, plain - full)
    assert not {k: v for k, v in full.items() if "seld::" not in k}
    assert sum(v for k, v in full.items() if "grad_norm_kernel" in k) == 1
    assert sum(v for k, v in full.items() if "adam_ex_kernel" in k) == 1 and not any("adam_kernel" in k for k in full)
    assert sum(v for k, v in plain.items() if "adam_kernel" in k) == 1 and not any("adam_ex" in k or "grad_norm" in k for k in plain)


# ======================================================================================================================
# data parallel, and the flags through train.main
# ======================================================================================================================
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
def test_two_ranks_clip_and_average_alike(tmp_path):
    """Two ranks (gloo, both on the one device), the tiny model, three steps with clipping, AdamW decay and the average:
    the norm is computed after the exchange, from the same averaged gradient on both ranks, so norm, parameters and average
    agree bit for bit without a collective of their own."""
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                   LOCAL_RANK=str(rank), SELD_DP_BACKEND="gloo", SELD_DP_SINGLE_DEVICE="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "optim_dp_worker.py"), str(tmp_path), "3"],
                                      env=env, cwd=ROOT))
    try:
        for p in procs:
            assert p.wait(timeout=420) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    assert r0["step_count"] == r1["step_count"] == 3
    for key in ("clip", "param", "ema", "exp_avg"):
        assert torch.equal(_bits(r0[key]), _bits(r1[key])), key
    assert float(r0["clip"][0]) > 0 and float(r0["clip"][3]) == 3.0 and not torch.equal(r0["param"], r0["ema"])
    assert r0["losses"] != r1["losses"]             # each rank trained on its own half of the batch


def test_main_with_the_flags_on(tmp_path, capsys):
    """train.main with every new flag, resident loader and recorded steps: the epoch line reports the clipping, validation
    runs under the average and hands the training weights back, the checkpoint carries both, and a resume restores the
    average it saved."""
    from tests.test_gpu_train_loader import MODEL_FLAGS, write_pickles
    T, H = pkg().train, pkg().hip_ops
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    made = []
    adam = T.FlatAdam

    def spy(*a, **k):
        made.append(adam(*a, **k))
        return made[-1]
    T.FlatAdam = spy
    scales, warmup_scale = [], T.warmup_scale
    T.warmup_scale = lambda step, n: (scales.append(warmup_scale(step, n)), scales[-1])[1]
    try:
        flags = dict(MODEL_FLAGS, **write_pickles(tmp_path, 5), results_path=str(tmp_path / "res"),
                     checkpoint_dir=str(tmp_path / "ck"), batch_size=2, epochs=2, min_n_epochs=2, resident_loader="True",
                     graph_step="True", grad_clip=1.0, weight_decay=0.01, decoupled_weight_decay="True", ema_decay=0.999,
                     warmup_steps=4)
        state = T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]))
        torch.cuda.synchronize()
        opt = made[0]
        assert state["step"] == 6 and opt.step_count == 6 and opt.decoupled and opt.max_grad_norm == 1.0
        assert opt.lr_scale == 1.0                  # steps 5 and 6 are past the warm-up of 4
        lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith("epoch ")]
        assert len(lines) == 2 and all("grad norm max" in line and "clipped" in line for line in lines), lines
        ck_root = str(tmp_path / "ck")
        path = os.path.join(ck_root, os.listdir(ck_root)[0], "checkpoint")
        ck = torch.load(path, map_location="cpu", weights_only=False)
        names = list(ck["ema_state_dict"])          # the model's parameters, in the model's order, and no buffer
        assert names == [k for k in ck["model_state_dict"] if k in ck["ema_state_dict"]] and len(names) == len(opt.params)
        assert not any("running_" in k or "num_batches" in k for k in names)
        differ = 0
        for name in names:                          # the training weights and the average, each where it belongs
            differ += int(not torch.equal(ck["ema_state_dict"][name], ck["model_state_dict"][name]))
        assert differ > len(names) // 2
        assert scales == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0], scales
        assert ck["optimizer_state_dict"]["param_groups"][0]["weight_decay"] == 0.01
        flat_ema = opt.ema.cpu()
        flags.update(load_model=path, epochs=3, min_n_epochs=3)
        state = T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]))
        assert state["step"] == 9 and made[1].step_count == 9 and not torch.equal(made[1].ema.cpu(), flat_ema)
    finally:
        T.FlatAdam, T.warmup_scale = adam, warmup_scale


def test_main_scores_the_test_leg_under_the_average(tmp_path):
    """--test_step=1 with --ema_decay: inside evaluate_test the model's parameters are the moving average of the checkpoint
    the test leg loaded; afterwards the model trains on with the training weights of the live checkpoint."""
    from tests.test_gpu_ensemble import _write_pickles
    from tests.test_gpu_train_loader import MODEL_FLAGS
    T, H = pkg().train, pkg().hip_ops
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    seen, made = {}, []
    adam, evaluate_test = T.FlatAdam, T.evaluate_test

    def spy_adam(*a, **k):
        made.append(adam(*a, **k))
        return made[-1]

    def spy_test(model, *a, **k):
        seen["lent"] = made[0]._ema_lent
        seen["params"] = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        seen["model"] = model
        return evaluate_test(model, *a, **k)
    T.FlatAdam, T.evaluate_test = spy_adam, spy_test
    try:
        flags = dict(MODEL_FLAGS, **_write_pickles(tmp_path), results_path=str(tmp_path / "res"),
                     checkpoint_dir=str(tmp_path / "ck"), batch_size=2, epochs=1, min_n_epochs=1, ema_decay=0.999,
                     grad_clip=1.0)
        flags.update(test_step=1, test_mode="test_best")
        T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]))
        torch.cuda.synchronize()
    finally:
        T.FlatAdam, T.evaluate_test = adam, evaluate_test
    assert seen["lent"] is True and made[0]._ema_lent is False
    ck_root = str(tmp_path / "ck")
    md = os.path.join(ck_root, os.listdir(ck_root)[0])
    best = torch.load(os.path.join(md, "checkpoint_best_model"), map_location="cpu", weights_only=False)
    live = torch.load(os.path.join(md, "checkpoint"), map_location="cpu", weights_only=False)
    moved = 0
    for name, p in seen["params"].items():
        assert torch.equal(p, best["ema_state_dict"][name]), name
        moved += int(not torch.equal(p, best["model_state_dict"][name]))
    assert moved > len(seen["params"]) // 2
    for name, p in seen["model"].named_parameters():
        assert torch.equal(p.detach().cpu(), live["model_state_dict"][name]), name
